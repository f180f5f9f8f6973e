// The covisibility graph and the spanning tree in device memory (include/orbm.h, "The covisibility graph on the device"):
//   orbm_update_connections_device    KeyFrame::updateConnections behind the refresh's d_covis (KeyFrame.cpp:244-290) with addConnection /
//                                     updateBestCovisibles of the neighbours (:293-337)
//   orbm_erase_connections_device     the graph part of KeyFrame::setBad (:403-405, :419-460) behind the culling's d_code
//   orbm_fuse_targets_device          the target key frames and the fuseMapPoints list of LocalMapping::searchInNeighbors (LocalMapping.cpp:263-300)
//   orbm_connected_keyframes_device   getConnectedKFs / getBestCovisibleKFs(num) as an array (KeyFrame.cpp:339-350)
//
// A list is its row sorted: descending weight, ascending slot among equal weights.  The key of an entry is 64 bits, the weight's
// order-preserving complement above the slot, so all keys of a row are distinct and an ascending bitonic sort in LDS (4096 keys, 32 KB)
// gives the same bytes whatever the schedule.  k_graph_update and k_graph_erase are ONE workgroup each (the edits are sequential and
// small); they mark in d_work the rows whose list has to be rebuilt, and k_graph_resort, launched behind them with one workgroup per
// key frame, rebuilds the marked ones: a workgroup reads its own mark and its own row and writes its own list, nothing another writes.
// k_graph_fuse_targets is one workgroup: wave 0 walks the lists (the marks decide who is appended, so the walk is sequential; the
// lanes share a second-neighbour list) while the other waves clear d_work; then the targets' rows in first-occurrence order
// (map_first_rows, orbm_map.h).
// Integer only.  No scratch memory, no handle scratch, no allocation, no host wait.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orbm_internal.h"
#include "orbm_map.h"

namespace {

typedef unsigned long long u64;

constexpr int GR_T = 1024;                       // the workgroup of every kernel but k_graph_connected
constexpr int GR_WAVES = GR_T / 64;
constexpr u64 GR_NO_KEY = ~0ull;                 // sorts behind every entry

// descending weight on the full int32, ascending slot: ascending in this key
__device__ __forceinline__ u64 graph_key(int w, int slot) { return (u64)(~((uint32_t)w ^ 0x80000000u)) << 32 | (uint32_t)slot; }

__device__ __forceinline__ int pow2_at_least(int n)
{
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

// ascending bitonic sort of s[0 .. n_pow2) by the whole workgroup; ends behind a barrier
__device__ __forceinline__ void sort_keys(u64 *s, int n_pow2)
{
    for (int k = 2; k <= n_pow2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < n_pow2; i += GR_T) {
                const int x = i ^ j;
                if (x <= i) continue;
                const u64 a = s[i], b = s[x];
                if ((a > b) == ((i & k) == 0)) s[i] = b, s[x] = a;
            }
        }
    }
    __syncthreads();
}

// updateBestCovisibles of key frame j: list j = the non-zero entries of row j in list order.  Every thread of the workgroup.
__device__ __forceinline__ void rebuild_list(const GraphView &g, int j, u64 *s_key, int *s_n)
{
    const int n2 = pow2_at_least(g.n_kf);
    if (threadIdx.x == 0) *s_n = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < n2; i += GR_T) {
        const int w = i < g.n_kf ? g.weight[(size_t)j * g.cap + i] : 0;
        s_key[i] = w ? graph_key(w, i) : GR_NO_KEY;
        mine += w != 0;
    }
    block_add(s_n, 0, mine);
    sort_keys(s_key, n2);
    const int n = *s_n;
    for (int i = threadIdx.x; i < n; i += GR_T) g.ord_kf[(size_t)j * g.cap + i] = (int32_t)(uint32_t)s_key[i];
    if (threadIdx.x == 0) g.ord_n[j] = n;
}

__global__ __launch_bounds__(GR_T) void k_graph_resort(GraphView g, const int32_t *__restrict__ work)
{
    __shared__ u64 s_key[ORBM_GRAPH_MAX_KF];
    __shared__ int s_n;
    const int j = blockIdx.x;
    if (work[j] == 0) return;                                      // the same word for every thread
    rebuild_list(g, j, s_key, &s_n);
}

enum { U_N = 0, U_NOTHING = 1, U_FALLBACK = 2, U_REBUILT = 3, U_PARENT = 4, U_BAD = 5, U_JUNK = 6 };

// c[j] of the header: the count of key frame j that takes part
__device__ __forceinline__ int covis_count(const int32_t *covis, const uint8_t *bad, int K, int j)
{
    const int v = covis[j];
    return j != K && v > 0 && !bad[j] ? v : 0;
}

__global__ __launch_bounds__(GR_T) void k_graph_update(GraphView g, const uint8_t *__restrict__ bad, const int32_t *__restrict__ covis, int K,
                                                       int first_kf, int th, int32_t *work, int32_t *result)
{
    __shared__ u64 s_key[ORBM_GRAPH_MAX_KF];
    __shared__ int s_count[8];
    __shared__ int s_max, s_least;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 8) s_count[tid] = 0;
    if (tid == 0) s_max = 0, s_least = MAP_NONE;
    __syncthreads();
    int on_bad = 0, junk = 0, over = 0, top = 0;
    for (int j = tid; j < g.n_kf; j += GR_T) {
        const int v = covis[j], c = covis_count(covis, bad, K, j);
        junk += j == K ? v != 0 : v < 0;
        on_bad += j != K && v > 0 && bad[j];
        over += c >= th;
        top = max(top, c);
    }
    top = wave_max(top);
    block_add(s_count, {U_BAD, U_JUNK, U_N}, {on_bad, junk, over});
    if (lane == 0 && top) atomicMax(&s_max, top);
    __syncthreads();
    const int c_max = s_max, n_over = s_count[U_N];
    if (c_max == 0) {                                              // kfCounter.empty(): nothing is written (KeyFrame.cpp:244)
        for (int j = tid; j < g.n_kf; j += GR_T) work[j] = 0;
        if (tid < 8) result[tid] = tid == U_NOTHING ? 1 : tid == U_BAD || tid == U_JUNK ? s_count[tid] : 0;
        return;
    }
    if (n_over == 0) {                                             // the fallback (:265-268): the least slot among the maxima
        for (int j = tid; j < g.n_kf; j += GR_T)
            if (covis_count(covis, bad, K, j) == c_max) atomicMin(&s_least, j);
        __syncthreads();
    }
    const int least = s_least, n_s = n_over ? n_over : 1;
    const int n2 = pow2_at_least(g.n_kf);
    int rebuilt = 0;
    for (int j = tid; j < n2; j += GR_T) {
        u64 key = GR_NO_KEY;
        if (j < g.n_kf) {
            const int c = covis_count(covis, bad, K, j);
            if (n_over ? c >= th : j == least) {                   // addConnection (:293-304)
                key = graph_key(c, j);
                int32_t *back = &g.weight[(size_t)j * g.cap + K];
                const bool changed = *back != c;
                if (changed) *back = c;
                work[j] = changed, rebuilt += changed;
            } else work[j] = 0;
            g.weight[(size_t)K * g.cap + j] = c;                   // connected_kf_weights = kfCounter (:281)
        }
        s_key[j] = key;
    }
    block_add(s_count, U_REBUILT, rebuilt);
    sort_keys(s_key, n2);
    for (int i = tid; i < n_s; i += GR_T) g.ord_kf[(size_t)K * g.cap + i] = (int32_t)(uint32_t)s_key[i];
    if (tid == 0) {
        g.ord_n[K] = n_s;
        const bool first = g.parent[K] < 0 && K != first_kf;       // be_first_connection && id != 0 (:285-289)
        if (first) g.parent[K] = (int32_t)(uint32_t)s_key[0];
        result[U_N] = n_s, result[U_NOTHING] = 0, result[U_FALLBACK] = n_over == 0, result[U_REBUILT] = s_count[U_REBUILT];
        result[U_PARENT] = first, result[U_BAD] = s_count[U_BAD], result[U_JUNK] = s_count[U_JUNK], result[7] = 0;
    }
}

enum { E_ERASED = 0, E_CONNECTIONS = 1, E_CHILDREN = 2, E_NO_PARENT = 3, E_LISTS = 4 };

__global__ __launch_bounds__(GR_T) void k_graph_erase(GraphView g, RecentList recent, int n_recent, const int32_t *__restrict__ code, int32_t *work,
                                                      int32_t *result)
{
    __shared__ int s_count[8];
    const int tid = threadIdx.x;
    if (tid < 8) s_count[tid] = 0;
    for (int j = tid; j < g.n_kf; j += GR_T) work[j] = 0;
    int connections = 0, children = 0;
    for (int idx = 0; idx < n_recent; ++idx) {
        __syncthreads();                                           // a candidate sees what the ones before it wrote
        if (code && code[idx] != 3) continue;
        const int c = recent.kf[idx];
        const int P = g.parent[c];
        for (int j = tid; j < g.n_kf; j += GR_T) {                 // eraseConnection in every neighbour (KeyFrame.cpp:403-405)
            if (j == c || g.weight[(size_t)c * g.cap + j] <= 0) continue;
            int32_t *back = &g.weight[(size_t)j * g.cap + c];
            if (*back > 0) *back = 0, st(&work[j], 1), ++connections;
        }
        __syncthreads();
        for (int j = tid; j < g.n_kf; j += GR_T) {
            g.weight[(size_t)c * g.cap + j] = 0;                   // connected_kf_weights.clear() (:419)
            if (P >= 0 && g.parent[j] == c) g.parent[j] = P, ++children;   // what :423-460 amount to: changeParent(parent) for every child
        }
        if (tid == 0) {
            g.ord_n[c] = 0;                                        // ordered_connected_kfs.clear() (:420)
            ++s_count[E_ERASED];
            s_count[E_NO_PARENT] += P < 0;
        }
    }
    __syncthreads();
    int lists = 0;
    for (int j = tid; j < g.n_kf; j += GR_T) lists += work[j] != 0;
    block_add(s_count, {E_CONNECTIONS, E_CHILDREN, E_LISTS}, {connections, children, lists});
    __syncthreads();
    if (tid < 8) result[tid] = s_count[tid];
}

enum { T_TARGETS = 0, T_ROWS = 1, T_REFUSED = 2, T_BAD = 3, T_INVALID = 4, T_DROPPED = 5, T_DUPLICATES = 6 };

__global__ __launch_bounds__(GR_T) void k_graph_fuse_targets(GraphView g, const int32_t *__restrict__ kf_n, const uint8_t *__restrict__ bad,
                                                             const int32_t *__restrict__ slots, int stride, const uint8_t *__restrict__ valid,
                                                             int cap_points, int cur, int n_first, int n_second, int cap_targets, int cap_rows,
                                                             int32_t *work, int32_t *targets, int32_t *rows, int32_t *result)
{
    __shared__ int32_t s_targets[ORBM_GRAPH_MAX_KF];               // marked key frames are distinct: never more than n_kf
    __shared__ uint32_t s_mark[ORBM_GRAPH_MAX_KF / 32];            // fuse_target_for_kf == current_kf->id, per call
    __shared__ int s_wave[GR_WAVES];
    __shared__ int s_count[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    const MapReadView map = {g.n_kf, stride, cap_points, 0, kf_n, bad, slots, valid, nullptr, nullptr, nullptr};   // the arguments keep their __restrict__
    if (tid < 8) s_count[tid] = 0;
    bits_zero<GR_T>(s_mark, ORBM_GRAPH_MAX_KF);
    __syncthreads();
    if (wave == 0) {
        // ---- the targets (LocalMapping.cpp:263-277): sequential, because the marks decide; the lanes share a second-neighbour list
        int nt = 0, n_bad = 0, dropped = 0;                        // the same in every lane
        const int nf = min(max(n_first, 0), graph_list_length(g, cur));
        for (int i = 0; i < nf; ++i) {
            const int a = uniform(g.ord_kf[(size_t)cur * g.cap + i]);
            if (a < 0 || a >= g.n_kf) {
                ++dropped;
                continue;
            }
            if (bit_test(s_mark, a)) continue;
            if (lane == 0) bit_set(s_mark, a), s_targets[nt] = a;
            wave_order();                                          // lane 0's mark, before any lane tests the second neighbours
            ++nt, n_bad += map.bad[a] != 0;
            const int ns = min(max(n_second, 0), graph_list_length(g, a));
            for (int t0 = 0; t0 < ns; t0 += 64) {
                const int t = t0 + lane;
                const int b = t < ns ? g.ord_kf[(size_t)a * g.cap + t] : -1;
                const bool out = t < ns && (b < 0 || b >= g.n_kf);
                dropped += __popcll(__ballot(out));
                bool cand = t < ns && !out && b != cur;
                if (cand) cand = !bit_test(s_mark, b);
                bool twice = false;                                // an earlier entry of this tile names the same key frame
                for (u64 m = __ballot(cand); m; m &= m - 1) {
                    const int l = __builtin_ctzll(m);
                    twice |= l < lane && __builtin_amdgcn_readlane(b, l) == b;
                }
                cand = cand && !twice;
                const u64 keep = __ballot(cand);
                if (cand) bit_set(s_mark, b), s_targets[nt + __popcll(keep & ((1ull << lane) - 1))] = b;
                wave_order();                                      // the tile's marks, before the next tile's and the next entry's tests
                nt +=__popcll(keep), n_bad += __popcll(__ballot(cand && map.bad[b] != 0));
            }
        }
        if (lane == 0) s_count[T_TARGETS] = nt, s_count[T_BAD] = n_bad, s_count[T_DROPPED] = dropped;
    } else {
        for (int p = tid - 64; p < map.cap_points; p += GR_T - 64) work[p] = MAP_NONE;
    }
    __syncthreads();
    const int nt = s_count[T_TARGETS];
    for (int t = tid; t < min(nt, cap_targets); t += GR_T) targets[t] = s_targets[t];
    // ---- the rows (:287-300), "kf has bad map-point" (:292) counted as invalid
    int invalid = 0, duplicates = 0;
    const int n_rows = map_first_rows<GR_T>(s_targets, nt, map, work, rows, cap_rows, s_wave, invalid, duplicates);
    block_add(s_count, {T_INVALID, T_DUPLICATES}, {invalid, duplicates});
    __syncthreads();
    if (tid == 0) s_count[T_ROWS] = n_rows, s_count[T_REFUSED] = (nt > cap_targets ? 1 : 0) | (n_rows > cap_rows ? 2 : 0);
    __syncthreads();
    if (tid < 8) result[tid] = s_count[tid];
}

__global__ __launch_bounds__(256) void k_graph_connected(GraphView g, int kf, int include_self, int max_n, int32_t *out, int n_out, int32_t *n_written)
{
    const int self = include_self != 0;
    const int n = min(self + min(max(max_n, 0), graph_list_length(g, kf)), n_out);
    for (int i = threadIdx.x; i < n_out; i += 256) out[i] = i >= n ? -1 : i < self ? kf : g.ord_kf[(size_t)kf * g.cap + i - self];
    if (threadIdx.x == 0) *n_written = n;
}

} // namespace

extern "C" int orbm_update_connections_device(orbm_t *h, const orbm_covis_graph *graph, int n_kf, const uint8_t *d_bad, const int32_t *d_covis,
                                              int kf_self, int first_kf, int connect_th, int32_t *d_work, int32_t *d_result, void *stream)
{
    GraphView g;
    if (int rc = orbm_graph_view(&g, graph, n_kf)) return rc;
    if (!d_bad || !d_covis || !d_work || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (kf_self < 0 || kf_self >= n_kf) return orbx_set_error(ORBX_E_ARG, "kf_self is not a key frame of the graph");
    if (first_kf < -1 || first_kf >= n_kf) return orbx_set_error(ORBX_E_ARG, "first_kf must be -1 or a key frame of the graph");
    if (connect_th < 1) return orbx_set_error(ORBX_E_ARG, "connect_th must be positive");
    if (int rc = orbm_graph_check_limit(graph)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    hipLaunchKernelGGL(k_graph_update, dim3(1), dim3(GR_T), 0, s, g, d_bad, d_covis, kf_self, first_kf, connect_th, d_work, d_result);
    ORB_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_graph_resort, dim3(n_kf), dim3(GR_T), 0, s, g, (const int32_t *)d_work);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_erase_connections_device(orbm_t *h, const orbm_covis_graph *graph, int n_kf, const int32_t *recent, int n_recent,
                                             const int32_t *d_code, int32_t *d_work, int32_t *d_result, void *stream)
{
    GraphView g;
    if (int rc = orbm_graph_view(&g, graph, n_kf)) return rc;
    if (n_recent < 0 || n_recent > MAP_MAX_RECENT) return orbx_set_error(ORBX_E_ARG, "n_recent must lie in [0, 32]");
    if (!d_result || (n_kf > 0 && !d_work) || (n_recent > 0 && !recent)) return orbx_set_error(ORBX_E_ARG, "null argument");
    RecentList list = {};
    for (int i = 0; i < n_recent; ++i) {
        if (recent[i] < 0 || recent[i] >= n_kf) return orbx_set_error(ORBX_E_ARG, "an entry of recent is not a key frame of the graph");
        list.kf[i] = recent[i];
    }
    if (int rc = orbm_graph_check_limit(graph)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    hipLaunchKernelGGL(k_graph_erase, dim3(1), dim3(GR_T), 0, s, g, list, n_recent, d_code, d_work, d_result);
    ORB_TRY(hipGetLastError());
    if (n_kf > 0) {
        hipLaunchKernelGGL(k_graph_resort, dim3(n_kf), dim3(GR_T), 0, s, g, (const int32_t *)d_work);
        ORB_TRY(hipGetLastError());
    }
    return ORBX_OK;
}

extern "C" int orbm_fuse_targets_device(orbm_t *h, const orbm_covis_graph *graph, int n_kf, const int32_t *d_n, const uint8_t *d_bad,
                                        const int32_t *d_slots, int stride, const uint8_t *d_valid, int cap_points, int cur, int n_first,
                                        int n_second, int cap_targets, int cap_rows, int32_t *d_work, int32_t *d_targets, int32_t *d_rows,
                                        int32_t *d_result, void *stream)
{
    GraphView g;
    if (int rc = orbm_graph_view(&g, graph, n_kf)) return rc;
    if (int rc = orbm_check_slots(n_kf, d_n, d_bad, d_slots, stride, d_valid, cap_points)) return rc;
    if (n_first < 0 || n_second < 0 || cap_targets < 0 || cap_rows < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (cur < 0 || cur >= n_kf) return orbx_set_error(ORBX_E_ARG, "cur is not a key frame of the graph");
    if (!d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (cap_points > 0 && !d_work) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if ((cap_targets > 0 && !d_targets) || (cap_rows > 0 && !d_rows)) return orbx_set_error(ORBX_E_ARG, "null output array");
    if (int rc = orbm_graph_check_limit(graph)) return rc;
    if (int rc = orbm_check_stride(stride)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    hipLaunchKernelGGL(k_graph_fuse_targets, dim3(1), dim3(GR_T), 0, s, g, d_n, d_bad, d_slots, stride, d_valid, cap_points, cur,
                       n_first, n_second, cap_targets, cap_rows, d_work, d_targets, d_rows, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_connected_keyframes_device(orbm_t *h, const orbm_covis_graph *graph, int n_kf, int kf, int include_self, int max_n,
                                               int32_t *d_out, int n_out, int32_t *d_n_out, void *stream)
{
    GraphView g;
    if (int rc = orbm_graph_view(&g, graph, n_kf)) return rc;
    if (kf < 0 || kf >= n_kf) return orbx_set_error(ORBX_E_ARG, "kf is not a key frame of the graph");
    if (max_n < 0 || n_out < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (!d_n_out || (n_out > 0 && !d_out)) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (int rc = orbm_graph_check_limit(graph)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    hipLaunchKernelGGL(k_graph_connected, dim3(1), dim3(256), 0, s, g, kf, include_self, max_n, d_out, n_out, d_n_out);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
