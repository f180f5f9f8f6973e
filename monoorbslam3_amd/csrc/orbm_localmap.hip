// The tracker's local map in device memory (include/orbm.h, "The tracker's local map on the device"):
//   orbm_local_map_device            Tracking::updateLocalKeyFrames + updateLocalMapPoints (modules/Frontend/Tracking.cpp:429-537)
//   orbm_track_counters_device       the increaseVisible / increaseFound loops of one tracked frame (:388-398, :403-412, :362-364)
//   orbm_num_tracked_points_device   KeyFrame::getNumTrackedMapPoint (modules/BasicObject/KeyFrame.cpp:146-152)
//
// k_local_map is ONE workgroup of 1024 threads, the shape of orbm_map.h: the work is a few thousand slots and a sequential walk,
// latency not throughput.  The votes are an LDS array filled by LDS atomics, a thread per frame slot walking its
// row's list; the marks are one bit per key frame in LDS; the voted key frames are appended behind a block scan over the slots in
// order; wave 0 then runs the expansion (the marks decide who is appended, so it is sequential; the lanes share a neighbour list and
// search the first child by ballot) while the other waves clear d_work; then the local key frames' rows in first-occurrence order
// (map_first_rows, orbm_map.h), which never depends on the atomics.  The two small calls are a thread per slot / per query.
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

constexpr int LM_T = 1024;                       // the workgroup of k_local_map
constexpr int LM_WAVES = LM_T / 64;
constexpr int LM_SMALL_T = 256;                  // the workgroup of the two small kernels

// CSR entry j of row p: 1 live, 0 stale, -1 an index out of range (dropped, never dereferenced)
__device__ __forceinline__ int entry_state(const MapReadView &m, int j, int p, int &k)
{
    int i;
    return map_entry(m, j, k, i) ? (int)map_live(m, k, i, p) : -1;
}

// d_result of orbm_local_map_device, as the header lists it
enum { R_KF = 0, R_ROWS = 1, R_REFUSED = 2, R_MAX_KF = 3, R_MAX_VOTES = 4, R_CLEARED = 5, R_CSR_DROPPED = 6, R_CSR_STALE = 7, R_VOTED = 8,
       R_RECENT_BAD = 9, R_LIST_DROPPED = 10, R_END = 11, R_INVALID = 12, R_DUPLICATES = 13 };
enum { END_RAN_OUT = 0, END_SIZE_LIMIT = 1, END_PARENT = 2 };

__global__ __launch_bounds__(LM_T) void k_local_map(MapReadView m, GraphReadView g, RecentList recent, int n_recent, int32_t *frame_mp, int n2, int n_neigh,
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
    if (tid == 0) s_least = MAP_NONE;
    bits_zero<LM_T>(s_mark, ORBM_GRAPH_MAX_KF);
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
        map_list(m, p, b, e);
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
        if (tid == 0) s_list[idx] = k, bit_set(s_mark, k);
        recent_bad += m.bad[k] != 0;
    }
    if (tid == 0) s_count[R_RECENT_BAD] = recent_bad;
    __syncthreads();
    // ---- the voted key frames in ascending slot order (:474-487), and maxKF: the least slot among the maxima
    int nl = n_recent, top = 0, voted = 0;
    for (int k0 = 0; k0 < m.n_kf; k0 += LM_T) {
        const int k = k0 + tid, v = k < m.n_kf ? s_votes[k] : 0;
        const bool add = v > 0 && !bit_test(s_mark, k);
        top = max(top, v), voted += v > 0;
        int tile;
        const int at = nl + block_scan<LM_WAVES>(add, s_wave, tile);
        if (add) s_list[at] = k, bit_set(s_mark, k);
        nl += tile;
    }
    top = wave_max(top);
    if (lane == 0 && top) atomicMax(&s_count[R_MAX_VOTES], top);
    block_add(s_count, {R_VOTED, R_CLEARED, R_CSR_DROPPED, R_CSR_STALE}, {voted, cleared, csr_dropped, stale});
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
            const int nn = min(max(n_neigh, 0), graph_list_length(g, kf));
            for (int t0 = 0; t0 < nn; t0 += 64) {                  // getBestCovisibleKFs(10) (:495-502)
                const int t = t0 + lane;
                const int b = t < nn ? g.ord_kf[(size_t)kf * g.cap + t] : -1;
                const bool out = t < nn && (b < 0 || b >= g.n_kf);
                dropped += __popcll(__ballot(out));
                bool cand = t < nn && !out;
                if (cand) cand = !m.bad[b] && !bit_test(s_mark, b);
                bool twice = false;                                // an earlier entry of this tile names the same key frame
                for (u64 c = __ballot(cand); c; c &= c - 1) {
                    const int l = __builtin_ctzll(c);
                    twice |= l < lane && __builtin_amdgcn_readlane(b, l) == b;
                }
                cand = cand && !twice;
                const u64 keep = __ballot(cand);
                if (cand) bit_set(s_mark, b), s_list[nl + __popcll(keep & ((1ull << lane) - 1))] = b;
                wave_order();                                      // the tile's marks, before the next tile's tests and the child's
                nl += __popcll(keep);
            }
            for (int j0 = 0; j0 < g.n_kf; j0 += 64) {              // the first child not bad and not marked, in ascending slot (:504-511)
                const int j = j0 + lane;
                const bool child = j < g.n_kf && g.parent[j] == kf && !m.bad[j] && !bit_test(s_mark, j);
                const u64 c = __ballot(child);
                if (c == 0) continue;
                const int first = j0 + __builtin_ctzll(c);
                if (lane == 0) bit_set(s_mark, first), s_list[nl] = first;
                wave_order();
                ++nl;
                break;
            }
            const int P = uniform(g.parent[kf]);                   // :513-518: not tested for bad, and the break leaves the whole walk
            if (P >= 0 && P < g.n_kf && !bit_test(s_mark, P)) {
                if (lane == 0) bit_set(s_mark, P), s_list[nl] = P;
                wave_order();
                ++nl, end = END_PARENT;
                break;
            }
        }
        if (lane == 0) s_count[R_KF] = nl, s_count[R_LIST_DROPPED] = dropped, s_count[R_END] = end;
    } else {
        for (int p = tid - 64; p < m.cap_points; p += LM_T - 64) work[p] = MAP_NONE;
    }
    __syncthreads();
    nl = s_count[R_KF];
    for (int t = tid; t < min(nl, cap_local_kf); t += LM_T) local_kf[t] = s_list[t];
    // ---- the points (:525-537)
    int invalid = 0, duplicates = 0;
    const int n_rows = map_first_rows<LM_T>(s_list, nl, m, work, rows, cap_rows, s_wave, invalid, duplicates);
    block_add(s_count, {R_INVALID, R_DUPLICATES}, {invalid, duplicates});
    const int refused = (nl > cap_local_kf ? 1 : 0) | (n_rows > cap_rows ? 2 : 0);
    for (int p = tid; p < m.cap_points; p += LM_T) local_mask[p] = !refused && ld(&work[p]) != MAP_NONE;
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
    block_add(result, {C_VISIBLE_FRAME, C_VISIBLE_QUERIES, C_FOUND, C_CLEARED}, {seen, in_view, hit, cleared});
}

// a thread per slot of the key frame *d_kf; count was cleared ahead of the launch
__global__ __launch_bounds__(LM_SMALL_T) void k_num_tracked(MapReadView m, const int32_t *__restrict__ d_kf, int min_obs, int32_t *count)
{
    const int kf = *d_kf, i = blockIdx.x * LM_SMALL_T + threadIdx.x;
    if (kf < 0 || kf >= m.n_kf) {                                  // the same word for every thread
        if (i == 0) count[1] = 1;
        return;
    }
    int tracked = 0, dropped = 0;
    if (i < map_slots(m, kf)) {
        const int p = *map_slot(m, kf, i);
        if (p >= 0 && p < m.cap_points) {                          // if (mp && mp->getNumObs() >= minObs): no test for bad
            int b, e, n_live = 0;
            map_list(m, p, b, e);
            for (int j = b; j < e; ++j) {
                int k;
                const int state = entry_state(m, j, p, k);
                n_live += state > 0, dropped += state < 0;
            }
            tracked = n_live >= min_obs;
        }
    }
    block_add(count, {0, 2}, {tracked, dropped});
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
    GraphReadView g;
    if (int rc = orbm_graph_view(&g, graph, n_kf)) return rc;
    if (!d_obs_off) return orbx_set_error(ORBX_E_ARG, "null map-point table array");   // wanted even when cap_points == 0
    MapReadView m;
    if (int rc = orbm_map_view(&m, n_kf, d_n, d_bad, d_slots, stride, d_valid, cap_points, d_obs_off, d_obs_kf, d_obs_kp, n_obs)) return rc;
    if (n2 < 0 || n_neigh < 0 || max_kf < 0 || cap_local_kf < 0 || cap_rows < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (n_recent < 0 || n_recent > MAP_MAX_RECENT) return orbx_set_error(ORBX_E_ARG, "n_recent must lie in [0, 32]");
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
    if (int rc = orbm_graph_check_limit(graph)) return rc;
    if (int rc = orbm_check_stride(stride)) return rc;
    if (int rc = frame_check_limit(n2)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
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
    if (!d_obs_off) return orbx_set_error(ORBX_E_ARG, "null map-point table array");   // wanted even when cap_points == 0
    if (cap_points < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (int rc = orbm_check_map(n_kf, d_n, d_bad, d_slots, stride, nullptr, 0, d_obs_off, d_obs_kf, d_obs_kp, n_obs)) return rc;   // no d_valid here
    if (!d_kf || !d_count) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (int rc = orbm_check_stride(stride)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    ORB_TRY(hipMemsetAsync(d_count, 0, 4 * sizeof(int32_t), s));
    const MapReadView m = {n_kf, stride, cap_points, n_obs, d_n, d_bad, d_slots, nullptr, d_obs_off, d_obs_kf, d_obs_kp};   // never tests for bad
    hipLaunchKernelGGL(k_num_tracked, dim3(max(1, (stride + LM_SMALL_T - 1) / LM_SMALL_T)), dim3(LM_SMALL_T), 0, s, m, d_kf, min_obs, d_count);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
