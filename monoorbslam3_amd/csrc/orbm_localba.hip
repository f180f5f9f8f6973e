// Local bundle adjustment on the device-resident map, the two ends of it (include/orbm.h, "Local bundle adjustment on the device-resident
// map"; the Levenberg-Marquardt loop between them is orbba_local_bundle_adjustment_device, csrc/orbba.hip):
//   orbm_local_ba_problem_device   Optimize::localBundleAdjustment's three gathering loops and its vertices and edges
//                                  (Optimize.cpp:766-806, :823-889) from the slot arrays, the observation index and the key-frame table
//   orbm_local_ba_apply_device     what it does with the optimiser's result (Optimize.cpp:914-950): the outlier observations erased with
//                                  the cascade of MapPoint::eraseObservation -> setBad (MapPoint.cpp:190-226), poses and positions written
//
// THE SLOT ARRAYS ARE THE TRUTH, the CSR only tells where the slots naming a row are (the rules and the view of orbm_map.h).
//
// The assembly.  ONE launch of ONE workgroup of 1024 threads (the shape of orbm_map.h: 20 key frames x 2000 slots x short lists
// is latency), in phases between barriers; d_work [cap_points + n_kf] is the caller's work array:
//   0  work_row[p] = none, work_kf[k] = none; the CSR's unusable entries counted
//   1  the local list: work_kf[k] = the FIRST position naming k (atomicMin: the value does not depend on the order); an entry is kept if it
//      is that first position and (position 0 or not bad); a block scan over the positions numbers the kept ones -> s_local[], work_kf[k]
//   2  a thread per slot of a local key frame: work_row[p] = the least (local index << 13 | slot) naming the valid row p (atomicMin again)
//   3  the slots again IN ORDER, a tile of 1024 at a time: a slot whose key is its row's is the row's first occurrence (BA_local_for_kf);
//      its thread counts the row's edges -- the live entries of its CSR list, a key frame's first entry only -- and marks every edge's
//      key frame that is not local as fixed; a block scan of (has an edge, edges) over the tile gives the point's number and its first
//      edge; the thread writes the point and walks its list a second time to write the edges' (key frame, feature, point)
//   4  the key frames marked fixed, numbered in ascending slot order behind the local ones by a block scan; work_kf[k] = the pose of k
//   5  the counts and the refusal; refused: return
//   6  a thread per pose (rotation, translation, fixed flag) and per edge (pose index, measurement, information)
// Counts are sums and every stored value is decided by the slot arrays alone: the bytes are the same on every run.
//
// The apply.  ONE launch of ONE workgroup of 1024 threads, a thread per local point: points are independent (a point's cascade touches only
// its own slots, d_valid[p] and d_ref_kf[p]) and the outlier edges of one point are sequential.  Then a thread per local key frame.
// The cascade is restated, not shared with k_cull: there the erased key frame is the culled one and every slot of it goes afterwards, here
// one slot goes first and the walk is per edge -- the two loops share three lines.
// No scratch memory, no handle scratch, no allocation, no host wait.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <string>

#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orbm_internal.h"
#include "orbm_map.h"

namespace {

constexpr int LB_T = 1024;              // the one workgroup
constexpr int LB_WAVES = LB_T / 64;
constexpr int LB_FIXED = MAP_NONE - 1;  // work_kf: a key frame of an edge that is not local, before it has a number (MAP_NONE: neither)
static_assert(ORBM_LOCAL_BA_MAX_LOCAL == LB_T, "a thread per entry of d_local");

// d_result of the assembly (int32 x 16) and of the apply (int32 x 8)
enum { P_POSES = 0, P_POINTS = 1, P_EDGES = 2, P_LOCAL = 3, P_FIXED = 4, P_REFUSED = 5, P_LOCAL_DROPPED = 6, P_LOCAL_BAD = 7,
       P_NO_EDGE = 8, P_SECOND = 9, P_CSR_DROPPED = 10 };
enum { A_ERASED = 0, A_POINTS_BAD = 1, A_CLEARED = 2, A_MOVED = 3, A_ROWS = 4, A_CSR_DROPPED = 5, A_MAP_DROPPED = 6, A_POSES = 7 };

// CSR entry j as an observation of row p; the slot is read with ld, as k_lba_apply's other threads clear slots in the same phase
template <bool W> __device__ __forceinline__ bool live_entry(const MapViewOf<W> &m, int j, int p, int &k, int &i)
{
    return map_live_entry<true>(m, j, p, k, i);
}

struct ProblemArgs {
    MapReadView m;
    const double *pose_R, *pose_t;       // the key-frame table's
    const void *const *kps;
    const float *points;
    const int32_t *local;
    int n_local, first_kf, cap_poses, cap_local_points, cap_edges;
    int32_t *work;                       // [cap_points] row keys, then [n_kf] key-frame marks
    double *o_pose_R, *o_pose_t;
    uint8_t *o_pose_fixed;
    double *o_points;
    int32_t *o_edge_pose, *o_edge_point;
    double *o_edge_z, *o_edge_inv_sigma2;
    int32_t *o_edge_kf, *o_edge_kp, *o_edge_off, *o_point_row, *o_pose_kf;
    int32_t *result;
};

// The edges of row p: its live CSR entries in CSR order, the first entry of a key frame only.  WRITE = false: count them, count the
// second entries, mark the key frames that are not local; true: write (key frame, feature, point) of edge number e0, e0 + 1, ...
template <bool WRITE>
__device__ __forceinline__ int problem_edges(const ProblemArgs &a, int32_t *work_kf, int p, int idx, int e0, int &second)
{
    int b, e, n = 0;
    map_list(a.m, p, b, e);
    for (int j = b; j < e; ++j) {
        int k, i;
        if (!live_entry(a.m, j, p, k, i)) continue;
        if (map_second_entry<true>(a.m, b, j, p, k)) {             // a key frame twice: the LM refuses such a problem
            second += !WRITE;
            continue;
        }
        if (WRITE) {
            const int x = e0 + n;
            if (x < a.cap_edges) a.o_edge_kf[x] = k, a.o_edge_kp[x] = i, a.o_edge_point[x] = idx;
        } else if (ld(&work_kf[k]) == MAP_NONE) {
            st(&work_kf[k], LB_FIXED);                             // whoever stores, the value is the same
        }
        ++n;
    }
    return n;
}

__global__ __launch_bounds__(LB_T) void k_lba_problem(const ProblemArgs a)
{
    __shared__ int s_local[LB_T];                                  // the kept local key frames in list order
    __shared__ int s_wave[2][LB_WAVES];
    __shared__ int s_count[16];
    const int tid = threadIdx.x;
    const MapReadView &m = a.m;
    int32_t *work_row = a.work, *work_kf = a.work + m.cap_points;
    // ---- 0
    for (int p = tid; p < m.cap_points; p += LB_T) work_row[p] = MAP_NONE;
    for (int k = tid; k < m.n_kf; k += LB_T) work_kf[k] = MAP_NONE;
    if (tid < 16) s_count[tid] = 0;
    int csr_dropped = 0, no_edge = 0, second = 0;                   // per thread, summed at the end
    for (int j = tid; j < m.n_obs; j += LB_T) csr_dropped += !map_usable(m, m.obs_kf[j], m.obs_kp[j]);
    __syncthreads();
    // ---- 1: the local key frames (Optimize.cpp:769-780)
    const int mine = tid < a.n_local ? a.local[tid] : -1;
    const bool in_range = tid < a.n_local && mine >= 0 && mine < m.n_kf;
    if (in_range) atomicMin(&work_kf[mine], tid);
    __syncthreads();
    const bool first = in_range && work_kf[mine] == tid;
    const bool is_bad = in_range && tid > 0 && m.bad[mine] != 0;  // :777; the current key frame is taken as it is
    const bool keep = first && !is_bad;
    const int local_dropped = tid < a.n_local && (!in_range || (!is_bad && !first));
    int li, unused, n_loc, n_local_dropped;
    block_scan2<LB_WAVES>(keep, local_dropped, s_wave, li, unused, n_loc, n_local_dropped);
    int skipped_bad, n_local_bad, has_first, n_has_first;
    block_scan2<LB_WAVES>(is_bad, keep && mine == a.first_kf, s_wave, skipped_bad, has_first, n_local_bad, n_has_first);
    if (first) work_kf[mine] = keep ? li : MAP_NONE;               // every read of the first positions lies before the scans' barriers
    if (keep) s_local[li] = mine;
    __syncthreads();
    // ---- 2: the rows named by a slot of a local key frame, and where first (:783-792)
    const int total = n_loc * m.stride;                            // <= 1024 * 8192
    map_mark_first<LB_T>(s_local, n_loc, m, work_row);
    __syncthreads();
    // ---- 3: points and edges in the order of first occurrence (:860-889)
    int n_points = 0, n_edges = 0;                                  // the same in every thread
    for (int t0 = 0; t0 < total; t0 += LB_T) {
        const int p = map_first_at(s_local, total, m, work_row, t0 + tid);
        const bool is_first = p >= 0;
        int cnt = 0;
        if (is_first) cnt = problem_edges<false>(a, work_kf, p, 0, 0, second);
        const bool has = is_first && cnt > 0;
        no_edge += is_first && cnt == 0;
        int my_point, my_edge, tile_points, tile_edges;
        block_scan2<LB_WAVES>(has, cnt, s_wave, my_point, my_edge, tile_points, tile_edges);
        if (has) {
            const int idx = n_points + my_point, e0 = n_edges + my_edge;
            if (idx < a.cap_local_points) {
                a.o_point_row[idx] = p, a.o_edge_off[idx] = e0;
                for (int c = 0; c < 3; ++c) a.o_points[(size_t)idx * 3 + c] = (double)a.points[(size_t)p * 3 + c];
            }
            problem_edges<true>(a, work_kf, p, idx, e0, second);
        }
        n_points += tile_points, n_edges += tile_edges;
    }
    __syncthreads();
    // ---- 4: the fixed key frames in ascending slot order (:795-806), behind the local ones
    int n_fixed = 0;
    for (int k0 = 0; k0 < m.n_kf; k0 += LB_T) {
        const int k = k0 + tid;
        const bool fixed = k < m.n_kf && work_kf[k] == LB_FIXED;
        int my, tile;
        block_scan2<LB_WAVES>(fixed, 0, s_wave, my, unused, tile, unused);
        if (fixed) {
            const int q = n_loc + n_fixed + my;
            work_kf[k] = q;
            if (q < a.cap_poses) a.o_pose_kf[q] = k;
        }
        n_fixed += tile;
    }
    if (tid < n_loc && tid < a.cap_poses) a.o_pose_kf[tid] = s_local[tid];
    // ---- 5: the counts and the refusal
    const int n_poses = n_loc + n_fixed;
    const int refused = (n_poses > a.cap_poses) | (n_points > a.cap_local_points) << 1 | (n_edges > a.cap_edges) << 2 |
                        (n_loc - (n_has_first != 0) < 1) << 3 | (n_edges < 1) << 4;
    block_add(s_count, {P_CSR_DROPPED, P_NO_EDGE, P_SECOND}, {csr_dropped, no_edge, second});
    __syncthreads();                                               // work_kf and o_pose_kf as well
    if (tid == 0) {
        s_count[P_POSES] = n_poses, s_count[P_POINTS] = n_points, s_count[P_EDGES] = n_edges, s_count[P_LOCAL] = n_loc;
        s_count[P_FIXED] = n_fixed, s_count[P_REFUSED] = refused, s_count[P_LOCAL_DROPPED] = n_local_dropped, s_count[P_LOCAL_BAD] = n_local_bad;
        if (n_points <= a.cap_local_points) a.o_edge_off[n_points] = n_edges;
    }
    __syncthreads();
    if (tid < 16) a.result[tid] = s_count[tid];
    if (refused) return;
    // ---- 6: the vertices' estimates (:826-845) and the edges' measurements (:871-878)
    for (int q = tid; q < n_poses; q += LB_T) {
        const int k = a.o_pose_kf[q];
#pragma unroll 1
        for (int c = 0; c < 9; ++c) a.o_pose_R[(size_t)q * 9 + c] = (double)(float)a.pose_R[(size_t)k * 9 + c];   // the reference's Pose is float
#pragma unroll 1
        for (int c = 0; c < 3; ++c) a.o_pose_t[(size_t)q * 3 + c] = (double)(float)a.pose_t[(size_t)k * 3 + c];
        a.o_pose_fixed[q] = q >= n_loc || k == a.first_kf;         // :830, :841
    }
    for (int x = tid; x < n_edges; x += LB_T) {
        const int k = a.o_edge_kf[x], i = a.o_edge_kp[x];
        a.o_edge_pose[x] = work_kf[k];
        map_edge_measurement(a.kps, k, i, a.o_edge_z + (size_t)x * 2, a.o_edge_inv_sigma2 + x);   // :871-877
    }
}

struct ApplyArgs {
    MapView m;
    int32_t *ref_kf;
    float *points;
    double *pose_R, *pose_t;             // the key-frame table's, in / out
    int n_local, n_points, n_edges;
    const int32_t *pose_kf, *point_row, *edge_off, *edge_kf, *edge_kp;
    const double *est_R, *est_t, *est_points;
    const uint8_t *outlier;
    int32_t *result;
};

__global__ __launch_bounds__(LB_T) void k_lba_apply(const ApplyArgs a)
{
    __shared__ int s_count[8];
    const int tid = threadIdx.x;
    const MapView &m = a.m;
    if (tid < 8) s_count[tid] = 0;
    __syncthreads();
    int count[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = tid; j < m.n_obs; j += LB_T) count[A_CSR_DROPPED] += !map_usable(m, m.obs_kf[j], m.obs_kp[j]);
    for (int idx = tid; idx < a.n_points; idx += LB_T) {
        const int p = a.point_row[idx];
        int b = a.edge_off[idx], e = a.edge_off[idx + 1];
        if (p < 0 || p >= m.cap_points || b < 0 || e < b || e > a.n_edges) {
            ++count[A_MAP_DROPPED];
            continue;
        }
        bool good = m.valid[p] != 0;
        int lb, le;
        map_list(m, p, lb, le);
        // ---- the outlier observations of this point, in edge order (Optimize.cpp:927-934)
        for (int x = b; x < e && good; ++x) {                      // :931: nothing more once the point is bad
            if (!a.outlier[x]) continue;
            const int k = a.edge_kf[x], i = a.edge_kp[x];
            if (!map_usable(m, k, i)) {
                ++count[A_MAP_DROPPED];
                continue;
            }
            if (!map_live<true>(m, k, i, p)) continue;                  // no observation there any more
            st(map_slot(m, k, i), -1);                             // KeyFrame::eraseMapPoint
            ++count[A_ERASED];
            int left = 0, first = -1, k2, i2;                      // MapPoint::eraseObservation (MapPoint.cpp:190-208)
            for (int j = lb; j < le; ++j) {
                if (!live_entry(m, j, p, k2, i2) || k2 == k) continue;
                if (left++ == 0) first = k2;
            }
            if (a.ref_kf[p] == k && left > 0) a.ref_kf[p] = first, ++count[A_MOVED];   // observations.begin()
            if (left > 2) continue;
            m.valid[p] = 0, good = false;                          // MapPoint::setBad (:202, :210-226)
            ++count[A_POINTS_BAD];
            for (int j = lb; j < le; ++j) {
                if (!live_entry(m, j, p, k2, i2) || k2 == k) continue;
                st(map_slot(m, k2, i2), -1);
                ++count[A_CLEARED];
            }
        }
        if (!good) continue;
        for (int c = 0; c < 3; ++c) a.points[(size_t)p * 3 + c] = (float)a.est_points[(size_t)idx * 3 + c];   // :944-947
        ++count[A_ROWS];
    }
    // ---- the local key frames' poses (:937-941)
    for (int q = tid; q < a.n_local; q += LB_T) {
        const int k = a.pose_kf[q];
        if (k < 0 || k >= m.n_kf) {
            ++count[A_MAP_DROPPED];
            continue;
        }
        for (int c = 0; c < 9; ++c) a.pose_R[(size_t)k * 9 + c] = (double)(float)a.est_R[(size_t)q * 9 + c];
        for (int c = 0; c < 3; ++c) a.pose_t[(size_t)k * 3 + c] = (double)(float)a.est_t[(size_t)q * 3 + c];
        ++count[A_POSES];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) block_add(s_count, c, count[c]);
    __syncthreads();
    if (tid < 8) a.result[tid] = s_count[tid];
}

} // namespace

extern "C" int orbm_local_ba_problem_device(orbm_t *h, const orbm_kf_table *kf, const int32_t *d_slots, int stride, const uint8_t *d_valid,
                                            const float *d_points, int cap_points, const int32_t *d_obs_off, const int32_t *d_obs_kf,
                                            const int32_t *d_obs_kp, int n_obs, const int32_t *d_local, int n_local, int first_kf,
                                            int cap_poses, int cap_local_points, int cap_edges, int32_t *d_work, double *d_pose_R,
                                            double *d_pose_t, uint8_t *d_pose_fixed, double *d_ba_points, int32_t *d_edge_pose,
                                            int32_t *d_edge_point, double *d_edge_z, double *d_edge_inv_sigma2, int32_t *d_edge_kf,
                                            int32_t *d_edge_kp, int32_t *d_edge_off, int32_t *d_point_row, int32_t *d_pose_kf,
                                            int32_t *d_result, void *stream)
{
    if (!kf || !d_result || !d_local) return orbx_set_error(ORBX_E_ARG, "null argument");
    ProblemArgs a = {};
    if (int rc = orbm_map_view(&a.m, kf->n_kf, kf->d_n, kf->d_bad, d_slots, stride, d_valid, cap_points, d_obs_off, d_obs_kf, d_obs_kp, n_obs)) return rc;
    if (n_local < 1 || cap_poses < 1 || cap_local_points < 1 || cap_edges < 1) return orbx_set_error(ORBX_E_ARG, "n_local and the capacities must be positive");
    if (kf->n_kf > 0 && (!kf->d_pose_R || !kf->d_pose_t || !kf->d_kps)) return orbx_set_error(ORBX_E_ARG, "null key-frame array");
    if (cap_points > 0 && !d_points) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if (!d_work || !d_pose_R || !d_pose_t || !d_pose_fixed || !d_ba_points || !d_edge_pose || !d_edge_point || !d_edge_z || !d_edge_inv_sigma2 ||
        !d_edge_kf || !d_edge_kp || !d_edge_off || !d_point_row || !d_pose_kf)
        return orbx_set_error(ORBX_E_ARG, "null output array");
    if (int rc = orbm_check_kf_rows(kf->d_kps)) return rc;
    if (first_kf < -1 || first_kf >= kf->n_kf) return orbx_set_error(ORBX_E_ARG, "first_kf is neither -1 nor a key frame of the table");
    if (n_local > ORBM_LOCAL_BA_MAX_LOCAL) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBM_LOCAL_BA_MAX_LOCAL (1024) entries in d_local");
    if (int rc = orbm_check_stride(stride)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    a.pose_R = kf->d_pose_R, a.pose_t = kf->d_pose_t, a.kps = kf->d_kps, a.points = d_points, a.local = d_local;
    a.n_local = n_local, a.first_kf = first_kf, a.cap_poses = cap_poses, a.cap_local_points = cap_local_points, a.cap_edges = cap_edges;
    a.work = d_work, a.o_pose_R = d_pose_R, a.o_pose_t = d_pose_t, a.o_pose_fixed = d_pose_fixed, a.o_points = d_ba_points;
    a.o_edge_pose = d_edge_pose, a.o_edge_point = d_edge_point, a.o_edge_z = d_edge_z, a.o_edge_inv_sigma2 = d_edge_inv_sigma2;
    a.o_edge_kf = d_edge_kf, a.o_edge_kp = d_edge_kp, a.o_edge_off = d_edge_off, a.o_point_row = d_point_row, a.o_pose_kf = d_pose_kf;
    a.result = d_result;
    hipLaunchKernelGGL(k_lba_problem, dim3(1), dim3(LB_T), 0, s, a);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_local_ba_apply_device(orbm_t *h, int n_kf, const int32_t *d_n, const uint8_t *d_bad, int32_t *d_slots, int stride,
                                          uint8_t *d_valid, int32_t *d_ref_kf, float *d_points, int cap_points, double *d_kf_pose_R,
                                          double *d_kf_pose_t, const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp,
                                          int n_obs, int n_local, int n_points, int n_edges, const int32_t *d_pose_kf,
                                          const int32_t *d_point_row, const int32_t *d_edge_off, const int32_t *d_edge_kf,
                                          const int32_t *d_edge_kp, const double *d_est_pose_R, const double *d_est_pose_t,
                                          const double *d_est_points, const uint8_t *d_outlier, int32_t *d_result, void *stream)
{
    if (!d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    ApplyArgs a = {};
    if (int rc = orbm_map_view(&a.m, n_kf, d_n, d_bad, d_slots, stride, d_valid, cap_points, d_obs_off, d_obs_kf, d_obs_kp, n_obs)) return rc;
    if (n_local < 0 || n_points < 0 || n_edges < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (cap_points > 0 && (!d_ref_kf || !d_points)) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if (n_local > 0 && (!d_kf_pose_R || !d_kf_pose_t || !d_pose_kf || !d_est_pose_R || !d_est_pose_t)) return orbx_set_error(ORBX_E_ARG, "null pose array");
    if (n_points > 0 && (!d_point_row || !d_edge_off || !d_est_points)) return orbx_set_error(ORBX_E_ARG, "null point array");
    if (n_edges > 0 && (!d_edge_kf || !d_edge_kp || !d_outlier)) return orbx_set_error(ORBX_E_ARG, "null edge array");
    if (int rc = orbm_check_stride(stride)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    a.ref_kf = d_ref_kf, a.points = d_points, a.pose_R = d_kf_pose_R, a.pose_t = d_kf_pose_t;
    a.n_local = n_local, a.n_points = n_points, a.n_edges = n_edges;
    a.pose_kf = d_pose_kf, a.point_row = d_point_row, a.edge_off = d_edge_off, a.edge_kf = d_edge_kf, a.edge_kp = d_edge_kp;
    a.est_R = d_est_pose_R, a.est_t = d_est_pose_t, a.est_points = d_est_points, a.outlier = d_outlier, a.result = d_result;
    hipLaunchKernelGGL(k_lba_apply, dim3(1), dim3(LB_T), 0, s, a);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
