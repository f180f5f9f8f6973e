// The tracker's local map in device memory (include/orbm.h, "The tracker's local map on the device"):
//   orbm_local_map_device            Tracking::updateLocalKeyFrames + updateLocalMapPoints (modules/Frontend/Tracking.cpp:429-537)
//   orbm_track_counters_device       the increaseVisible / increaseFound loops of one tracked frame (:388-398, :403-412, :362-364)
//   orbm_num_tracked_points_device   KeyFrame::getNumTrackedMapPoint (modules/BasicObject/KeyFrame.cpp:146-152)
//
// k_local_map is ONE workgroup of 1024 threads, the shape of k_graph_fuse_targets and k_lba_problem: the work is a few thousand slots
// and a sequential walk, latency not throughput.  The votes are an LDS array filled by LDS atomics, a thread per frame slot walking its
// row's list; the marks are one bit per key frame in LDS; the voted key frames are appended behind a block scan over the slots in
// order; wave 0 then runs the expansion (the marks decide who is appended, so it is sequential; the lanes share a neighbour list and
// search the first child by ballot) while the other waves clear d_work; then the rows' first occurrences by atomicMin and the slots in
// order, a tile of 1024 at a time, numbered by a block scan, so the order never depends on the atomics.  The two small calls are a
// thread per slot / per query.
// Integer only.  No scratch memory, no handle scratch, no allocation, no host wait.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orbm_internal.h"

namespace {

typedef unsigned long long u64;

constexpr int LM_T = 1024;                       // the workgroup of k_local_map
constexpr int LM_WAVES = LM_T / 64;
constexpr int LM_MAX_RECENT = 32;
constexpr int LM_NONE = 0x7fffffff;
constexpr int LM_KEY_SHIFT = 13;                 // a slot position (< ORBM_MEDIAN_MAX_STRIDE = 8192) below the key frame's position (< 4096)
constexpr int LM_SMALL_T = 256;                  // the workgroup of the two small kernels

// the map as orbm_build_observations_device takes and leaves it
struct MapView {
    int n_kf, stride, cap_points, n_obs;
    const int32_t *kf_n, *slots, *obs_off, *obs_kf, *obs_kp;
    const uint8_t *bad, *valid;
};

struct GraphView {
    int cap, n_kf;
    const int32_t *ord_kf, *ord_n, *parent;
};

struct RecentList {
    int32_t kf[LM_MAX_RECENT];
};

// values other threads of the workgroup (or lanes of the wave) write in the same phase: relaxed atomics, plain loads and stores in the ISA
__device__ __forceinline__ int ld(const int32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

// exclusive scan of v over the workgroup in thread order and the total; s_wave is LM_WAVES ints; two barriers
__device__ __forceinline__ int block_scan(int v, int *s_wave, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = wave_scan(v);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = inc - v;
    total = 0;
#pragma unroll 1
    for (int w = 0; w < LM_WAVES; ++w) {
        const int x = s_wave[w];
        if (w < wave) before += x;
        total += x;
    }
    __syncthreads();
    return before;
}

// The expansion runs in ONE wave whose lanes write marks that other lanes of the same wave read in the next step.  The LDS pipe serves a
// wave's accesses in issue order, so the hardware needs nothing; this keeps the COMPILER from moving a later read above an earlier
// write (a fence at wavefront scope and a wave barrier emit no instruction).
__device__ __forceinline__ void wave_order()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ bool marked(const uint32_t *s_mark, int k)
{
    return __hip_atomic_load(&s_mark[k >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> (k & 31) & 1;
}
__device__ __forceinline__ void mark(uint32_t *s_mark, int k) { atomicOr(&s_mark[k >> 5], 1u << (k & 31)); }

// the list of row p, distrusted: offsets that do not describe a list inside [0, n_obs] give an empty one
__device__ __forceinline__ void row_list(const MapView &m, int p, int &b, int &e)
{
    b = m.obs_off[p], e = m.obs_off[p + 1];
    if (b < 0 || e < b || e > m.n_obs) b = e = 0;
}

// CSR entry j of row p: 1 live, 0 stale, -1 an index out of range (dropped, never dereferenced)
__device__ __forceinline__ int entry_state(const MapView &m, int j, int p, int &k)
{
    k = m.obs_kf[j];
    const int i = m.obs_kp[j];
    if (k < 0 || k >= m.n_kf) return -1;
    if (i < 0 || i >= min(max(m.kf_n[k], 0), m.stride)) return -1;
    return m.slots[(size_t)k * m.stride + i] == p && m.bad[k] == 0;
}

// d_result of orbm_local_map_device, as the header lists it
enum { R_KF = 0, R_ROWS = 1, R_REFUSED = 2, R_MAX_KF = 3, R_MAX_VOTES = 4, R_CLEARED = 5, R_CSR_DROPPED = 6, R_CSR_STALE = 7, R_VOTED = 8,
       R_RECENT_BAD = 9, R_LIST_DROPPED = 10, R_END = 11, R_INVALID = 12, R_DUPLICATES = 13 };
enum { END_RAN_OUT = 0, END_SIZE_LIMIT = 1, END_PARENT = 2 };

__global__ __launch_bounds__(LM_T) void k_local_map(MapView m, GraphView g, RecentList recent, int n_recent, int32_t *frame_mp, int n2, int n_neigh,
                                                    int max_kf, int cap_local_kf, int cap_rows, int32_t *work, int32_t *local_kf, int32_t *rows,
                                                    uint8_t *local_mask, int32_t *ref, int32_t *result)
{
    __shared__ int s_votes[ORBM_GRAPH_MAX_KF];
    __shared__ int32_t s_list[ORBM_GRAPH_MAX_KF];                  // marked key frames are distinct: never more than n_kf
    __shared__ uint32_t s_mark[ORBM_GRAPH_MAX_KF / 32];            // track_frame_id == current_frame->id, per call
    __shared__ int s_wave[LM_WAVES];
    __shared__ int s_count[16];
    __shared__ int s_least;
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    if (tid < 16) s_count[tid] = 0;
    if (tid == 0) s_least = LM_NONE;
    for (int i = tid; i < ORBM_GRAPH_MAX_KF / 32; i += LM_T) s_mark[i] = 0;
    for (int k = tid; k < m.n_kf; k += LM_T) s_votes[k] = 0;
    __syncthreads();
    // ---- the votes (Tracking.cpp:431-460): a thread per frame slot walks its row's list
    int cleared = 0, csr_dropped = 0, stale = 0;
    for (int i = tid; i < n2; i += LM_T) {
        const int p = frame_mp[i];
        if (p < 0 || p >= m.cap_points) continue;
        if (!m.valid[p]) {                                         // :441-443
            frame_mp[i] = -1, ++cleared;
            continue;
        }
        int b, e;
        row_list(m, p, b, e);
        for (int j = b; j < e; ++j) {
            int k;
            const int state = entry_state(m, j, p, k);
            if (state > 0) atomicAdd(&s_votes[k], 1);
            else if (state < 0) ++csr_dropped;
            else ++stale;
        }
    }
    int recent_bad = 0;                                            // the recent key frames, each marked (:466-470); not tested for bad
    for (int idx = 0; idx < n_recent; ++idx) {
        const int k = recent.kf[idx];                              // the same for every thread
        if (tid == 0) s_list[idx] = k, mark(s_mark, k);
        recent_bad += m.bad[k] != 0;
    }
    if (tid == 0) s_count[R_RECENT_BAD] = recent_bad;
    __syncthreads();
    // ---- the voted key frames in ascending slot order (:474-487), and maxKF: the least slot among the maxima
    int nl = n_recent, top = 0, voted = 0;
    for (int k0 = 0; k0 < m.n_kf; k0 += LM_T) {
        const int k = k0 + tid, v = k < m.n_kf ? s_votes[k] : 0;
        const bool add = v > 0 && !marked(s_mark, k);
        top = max(top, v), voted += v > 0;
        int tile;
        const int at = nl + block_scan(add, s_wave, tile);
        if (add) s_list[at] = k, mark(s_mark, k);
        nl += tile;
    }
    top = wave_max(top), voted = wave_sum(voted);
    cleared = wave_sum(cleared), csr_dropped = wave_sum(csr_dropped), stale = wave_sum(stale);
    if (lane == 0) {
        if (top) atomicMax(&s_count[R_MAX_VOTES], top);
        if (voted) atomicAdd(&s_count[R_VOTED], voted);
        if (cleared) atomicAdd(&s_count[R_CLEARED], cleared);
        if (csr_dropped) atomicAdd(&s_count[R_CSR_DROPPED], csr_dropped);
        if (stale) atomicAdd(&s_count[R_CSR_STALE], stale);
    }
    __syncthreads();
    const int max_votes = s_count[R_MAX_VOTES];
    if (max_votes > 0)
        for (int k = tid; k < m.n_kf; k += LM_T)
            if (s_votes[k] == max_votes) atomicMin(&s_least, k);
    if (wave == 0) {
        // ---- the expansion (:490-519): sequential, because the marks decide; end0 is taken once, as iterEnd is
        const int end0 = nl;
        int end = END_RAN_OUT, dropped = 0;                        // the same in every lane
        for (int pos = 0; pos < end0; ++pos) {
            if (nl > max_kf) {                                     // :492
                end = END_SIZE_LIMIT;
                break;
            }
            const int kf = uniform(s_list[pos]);
            const int nn = min(max(n_neigh, 0), min(max(g.ord_n[kf], 0), g.n_kf));
            for (int t0 = 0; t0 < nn; t0 += 64) {                  // getBestCovisibleKFs(10) (:495-502)
                const int t = t0 + lane;
                const int b = t < nn ? g.ord_kf[(size_t)kf * g.cap + t] : -1;
                const bool out = t < nn && (b < 0 || b >= g.n_kf);
                dropped += __popcll(__ballot(out));
                bool cand = t < nn && !out;
                if (cand) cand = !m.bad[b] && !marked(s_mark, b);
                bool twice = false;                                // an earlier entry of this tile names the same key frame
                for (u64 c = __ballot(cand); c; c &= c - 1) {
                    const int l = __builtin_ctzll(c);
                    twice |= l < lane && __builtin_amdgcn_readlane(b, l) == b;
                }
                cand = cand && !twice;
                const u64 keep = __ballot(cand);
                if (cand) {
                    mark(s_mark, b);
                    s_list[nl + __popcll(keep & ((1ull << lane) - 1))] = b;
                }
                wave_order();                                      // the tile's marks, before the next tile's tests and the child's
                nl += __popcll(keep);
            }
            for (int j0 = 0; j0 < g.n_kf; j0 += 64) {              // the first child not bad and not marked, in ascending slot (:504-511)
                const int j = j0 + lane;
                const bool child = j < g.n_kf && g.parent[j] == kf && !m.bad[j] && !marked(s_mark, j);
                const u64 c = __ballot(child);
                if (c == 0) continue;
                const int first = j0 + __builtin_ctzll(c);
                if (lane == 0) mark(s_mark, first), s_list[nl] = first;
                wave_order();
                ++nl;
                break;
            }
            const int P = uniform(g.parent[kf]);                   // :513-518: not tested for bad, and the break leaves the whole walk
            if (P >= 0 && P < g.n_kf && !marked(s_mark, P)) {
                if (lane == 0) mark(s_mark, P), s_list[nl] = P;
                wave_order();
                ++nl, end = END_PARENT;
                break;
            }
        }
        if (lane == 0) s_count[R_KF] = nl, s_count[R_LIST_DROPPED] = dropped, s_count[R_END] = end;
    } else {
        for (int p = tid - 64; p < m.cap_points; p += LM_T - 64) work[p] = LM_NONE;
    }
    __syncthreads();
    nl = s_count[R_KF];
    for (int t = tid; t < min(nl, cap_local_kf); t += LM_T) local_kf[t] = s_list[t];
    // ---- the points (:525-537): a row's first occurrence in (key frame, slot) order is the least key naming it, whatever the atomics' order
    int invalid = 0, duplicates = 0;
    for (int t = 0; t < nl; ++t) {
        const int k = s_list[t], nk = min(max(m.kf_n[k], 0), m.stride);
        for (int i = tid; i < nk; i += LM_T) {
            const int p = m.slots[(size_t)k * m.stride + i];
            if (p < 0 || p >= m.cap_points) continue;
            if (!m.valid[p]) ++invalid;
            else atomicMin(&work[p], t << LM_KEY_SHIFT | i);
        }
    }
    __syncthreads();
    int n_rows = 0;
    for (int t = 0; t < nl; ++t) {
        const int k = s_list[t], nk = min(max(m.kf_n[k], 0), m.stride);
        for (int i0 = 0; i0 < nk; i0 += LM_T) {
            const int i = i0 + tid;
            int p = -1;
            bool first = false;
            if (i < nk) {
                p = m.slots[(size_t)k * m.stride + i];
                if (p >= 0 && p < m.cap_points && m.valid[p]) {
                    first = ld(&work[p]) == (t << LM_KEY_SHIFT | i);
                    duplicates += !first;
                }
            }
            int tile;
            const int at = n_rows + block_scan(first, s_wave, tile);
            if (first && at < cap_rows) rows[at] = p;
            n_rows += tile;
        }
    }
    invalid = wave_sum(invalid), duplicates = wave_sum(duplicates);
    if (lane == 0) {
        if (invalid) atomicAdd(&s_count[R_INVALID], invalid);
        if (duplicates) atomicAdd(&s_count[R_DUPLICATES], duplicates);
    }
    const int refused = (nl > cap_local_kf ? 1 : 0) | (n_rows > cap_rows ? 2 : 0);
    for (int p = tid; p < m.cap_points; p += LM_T) local_mask[p] = !refused && ld(&work[p]) != LM_NONE;
    __syncthreads();
    if (tid == 0) {
        const int max_kf_slot = max_votes > 0 ? s_least : -1;
        s_count[R_ROWS] = n_rows, s_count[R_REFUSED] = refused, s_count[R_MAX_KF] = max_kf_slot;
        if (max_kf_slot >= 0 && !refused) *ref = max_kf_slot;     // if (maxKF) reference_kf = maxKF (:522)
    }
    __syncthreads();
    if (tid < 16) result[tid] = s_count[tid];
}

enum { C_VISIBLE_FRAME = 0, C_VISIBLE_QUERIES = 1, C_FOUND = 2, C_CLEARED = 3 };

// a thread per frame slot and per query; result was cleared ahead of the launch
__global__ __launch_bounds__(LM_SMALL_T) void k_track_counters(int32_t *frame_mp, int n2, const uint8_t *__restrict__ valid, int cap_points,
                                                               const uint8_t *__restrict__ q_ok, int nq, int what, int32_t *visible,
                                                               int32_t *found, int32_t *result)
{
    const int idx = blockIdx.x * LM_SMALL_T + threadIdx.x;
    int seen = 0, in_view = 0, hit = 0, cleared = 0;
    if (idx < n2) {
        int p = frame_mp[idx];
        if (p >= 0 && p < cap_points) {
            if (what & 1) {                                        // Tracking.cpp:388-398
                if (!valid[p]) frame_mp[idx] = p = -1, cleared = 1;
                else atomicAdd(&visible[p], 1), seen = 1;
            }
            if ((what & 4) && p >= 0) atomicAdd(&found[p], 1), hit = 1;   // :362-364: no test for bad
        }
    }
    if ((what & 2) && idx < nq && q_ok[idx]) atomicAdd(&visible[idx], 1), in_view = 1;   // :406-408
    seen = wave_sum(seen), in_view = wave_sum(in_view), hit = wave_sum(hit), cleared = wave_sum(cleared);
    if ((threadIdx.x & 63) == 0) {
        if (seen) atomicAdd(&result[C_VISIBLE_FRAME], seen);
        if (in_view) atomicAdd(&result[C_VISIBLE_QUERIES], in_view);
        if (hit) atomicAdd(&result[C_FOUND], hit);
        if (cleared) atomicAdd(&result[C_CLEARED], cleared);
    }
}

// a thread per slot of the key frame *d_kf; count was cleared ahead of the launch
__global__ __launch_bounds__(LM_SMALL_T) void k_num_tracked(MapView m, const int32_t *__restrict__ d_kf, int min_obs, int32_t *count)
{
    const int kf = *d_kf, i = blockIdx.x * LM_SMALL_T + threadIdx.x;
    if (kf < 0 || kf >= m.n_kf) {                                  // the same word for every thread
        if (i == 0) count[1] = 1;
        return;
    }
    int tracked = 0, dropped = 0;
    if (i < min(max(m.kf_n[kf], 0), m.stride)) {
        const int p = m.slots[(size_t)kf * m.stride + i];
        if (p >= 0 && p < m.cap_points) {                          // if (mp && mp->getNumObs() >= minObs): no test for bad
            int b, e, n_live = 0;
            row_list(m, p, b, e);
            for (int j = b; j < e; ++j) {
                int k;
                const int state = entry_state(m, j, p, k);
                n_live += state > 0, dropped += state < 0;
            }
            tracked = n_live >= min_obs;
        }
    }
    tracked = wave_sum(tracked), dropped = wave_sum(dropped);
    if ((threadIdx.x & 63) == 0) {
        if (tracked) atomicAdd(&count[0], tracked);
        if (dropped) atomicAdd(&count[2], dropped);
    }
}

// the map's arguments: ORBX_E_ARG here, the limits behind the other arguments' checks
int map_check(int n_kf, const int32_t *d_n, const uint8_t *d_bad, const int32_t *d_slots, int stride, const uint8_t *d_valid, int cap_points,
              const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs)
{
    if (n_kf < 0 || stride < 0 || cap_points < 0 || n_obs < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (n_kf > 0 && (!d_n || !d_bad)) return orbx_set_error(ORBX_E_ARG, "null key-frame array");
    if (n_kf > 0 && stride > 0 && !d_slots) return orbx_set_error(ORBX_E_ARG, "null slot array");
    if (!d_obs_off || (cap_points > 0 && !d_valid)) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if (n_obs > 0 && (!d_obs_kf || !d_obs_kp)) return orbx_set_error(ORBX_E_ARG, "null observation array");
    return ORBX_OK;
}

int frame_check_limit(int n2)
{
    return n2 > ORBM_MEDIAN_MAX_STRIDE ? orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBM_MEDIAN_MAX_STRIDE (8192) key points in the frame") : ORBX_OK;
}

} // namespace

extern "C" int orbm_local_map_device(orbm_t *h, int32_t *d_frame_mp, int n2, const uint8_t *d_valid, int cap_points, const int32_t *d_obs_off,
                                     const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs, int n_kf, const int32_t *d_n,
                                     const uint8_t *d_bad, const int32_t *d_slots, int stride, const orbm_covis_graph *graph,
                                     const int32_t *recent, int n_recent, int n_neigh, int max_kf, int cap_local_kf, int cap_rows,
                                     int32_t *d_work, int32_t *d_local_kf, int32_t *d_rows, uint8_t *d_local_mask, int32_t *d_ref,
                                     int32_t *d_result, void *stream)
{
    if (!graph) return orbx_set_error(ORBX_E_ARG, "null graph");
    if (!graph->d_weight || !graph->d_ord_kf || !graph->d_ord_n || !graph->d_parent) return orbx_set_error(ORBX_E_ARG, "null graph array");
    if (graph->cap_kf < 0 || n_kf < 0 || n_kf > graph->cap_kf) return orbx_set_error(ORBX_E_ARG, "n_kf must lie in [0, cap_kf]");
    if (int rc = map_check(n_kf, d_n, d_bad, d_slots, stride, d_valid, cap_points, d_obs_off, d_obs_kf, d_obs_kp, n_obs)) return rc;
    if (n2 < 0 || n_neigh < 0 || max_kf < 0 || cap_local_kf < 0 || cap_rows < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (n_recent < 0 || n_recent > LM_MAX_RECENT) return orbx_set_error(ORBX_E_ARG, "n_recent must lie in [0, 32]");
    if ((n2 > 0 && !d_frame_mp) || (n_recent > 0 && !recent) || !d_ref || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if ((cap_points > 0 && (!d_work || !d_local_mask)) || (cap_local_kf > 0 && !d_local_kf) || (cap_rows > 0 && !d_rows))
        return orbx_set_error(ORBX_E_ARG, "null output array");
    RecentList list = {};
    for (int i = 0; i < n_recent; ++i) {
        if (recent[i] < 0 || recent[i] >= n_kf) return orbx_set_error(ORBX_E_ARG, "an entry of recent is not a key frame of the graph");
        for (int j = 0; j < i; ++j)
            if (recent[j] == recent[i]) return orbx_set_error(ORBX_E_ARG, "a key frame occurs twice in recent");
        list.kf[i] = recent[i];
    }
    if (graph->cap_kf > ORBM_GRAPH_MAX_KF) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBM_GRAPH_MAX_KF (4096) key frames in the graph");
    if (int rc = orbm_check_stride(stride)) return rc;
    if (int rc = frame_check_limit(n2)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    const MapView m = {n_kf, stride, cap_points, n_obs, d_n, d_slots, d_obs_off, d_obs_kf, d_obs_kp, d_bad, d_valid};
    const GraphView g = {graph->cap_kf, n_kf, graph->d_ord_kf, graph->d_ord_n, graph->d_parent};
    hipLaunchKernelGGL(k_local_map, dim3(1), dim3(LM_T), 0, s, m, g, list, n_recent, d_frame_mp, n2, n_neigh, max_kf, cap_local_kf, cap_rows, d_work,
                       d_local_kf, d_rows, d_local_mask, d_ref, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_track_counters_device(orbm_t *h, int32_t *d_frame_mp, int n2, const uint8_t *d_valid, int cap_points, const uint8_t *d_q_ok,
                                          int nq, int what, int32_t *d_visible, int32_t *d_found, int32_t *d_result, void *stream)
{
    if (n2 < 0 || cap_points < 0 || nq < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (what < 0 || what > 7) return orbx_set_error(ORBX_E_ARG, "what must be a mask of the bits 1, 2 and 4");
    if ((what & 2) && (!d_q_ok || nq > cap_points)) return orbx_set_error(ORBX_E_ARG, "bit 2 needs d_q_ok and nq <= cap_points");
    if ((n2 > 0 && !d_frame_mp) || (cap_points > 0 && !d_valid) || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (cap_points > 0 && (((what & 3) && !d_visible) || ((what & 4) && !d_found))) return orbx_set_error(ORBX_E_ARG, "null counter array");
    if (int rc = frame_check_limit(n2)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    ORB_TRY(hipMemsetAsync(d_result, 0, 8 * sizeof(int32_t), s));
    const int n = max(n2, (what & 2) ? nq : 0);
    if (n == 0) return ORBX_OK;
    hipLaunchKernelGGL(k_track_counters, dim3((n + LM_SMALL_T - 1) / LM_SMALL_T), dim3(LM_SMALL_T), 0, s, d_frame_mp, n2, d_valid, cap_points, d_q_ok,
                       nq, what, d_visible, d_found, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_num_tracked_points_device(orbm_t *h, const int32_t *d_kf, int min_obs, int n_kf, const int32_t *d_n, const uint8_t *d_bad,
                                              const int32_t *d_slots, int stride, int cap_points, const int32_t *d_obs_off,
                                              const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs, int32_t *d_count, void *stream)
{
    if (int rc = map_check(n_kf, d_n, d_bad, d_slots, stride, nullptr, 0, d_obs_off, d_obs_kf, d_obs_kp, n_obs)) return rc;
    if (cap_points < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (!d_kf || !d_count) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (int rc = orbm_check_stride(stride)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    ORB_TRY(hipMemsetAsync(d_count, 0, 4 * sizeof(int32_t), s));
    const MapView m = {n_kf, stride, cap_points, n_obs, d_n, d_slots, d_obs_off, d_obs_kf, d_obs_kp, d_bad, nullptr};
    hipLaunchKernelGGL(k_num_tracked, dim3(max(1, (stride + LM_SMALL_T - 1) / LM_SMALL_T)), dim3(LM_SMALL_T), 0, s, m, d_kf, min_obs, d_count);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
