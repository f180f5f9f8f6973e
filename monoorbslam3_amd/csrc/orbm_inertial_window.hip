// The window of the inertial local bundle adjustment assembled from the device-resident map (include/orbm.h, "The inertial local BA
// window on the device-resident map"): steps 1 and 3 of Optimize::localFullBundleAdjustment (Optimize.cpp:1073-1108, :1129-1244) as
//   orbm_inertial_window_problem_device          the solve states, the local points, the fixed key frames under the reference's cap,
//                                                the EdgeMono arrays in the layout of the visual-window header's calls, and the job
//                                                lists of the inertial-factor calls (orbi_factors.h)
//   orbm_inertial_window_velocity_prior_device   what KeyFrame::setVelocity leaves in the OLDEST key frame's velo_priori (step 7)
// The Levenberg-Marquardt loop between them is the caller's; the rest of the tail is orbm_local_ba_apply_device.
//
// THE SLOT ARRAYS ARE THE TRUTH, the CSR only tells where the slots naming a row are (the rules and the view of orbm_map.h).
//
// The assembly.  ONE launch of ONE workgroup of 1024 threads (the shape of orbm_map.h: 25 key frames x 2000 slots x short lists is
// latency), in phases between barriers; d_work [cap_points + 2 n_kf] is the caller's work array: row keys, states, first keys.
//   0  work_row[p] = work_kf[k] = work_first[k] = none; the CSR's unusable entries counted
//   1  the window: work_kf[k] = the FIRST position naming k (atomicMin); a position is usable if it is that first position, its key
//      frame exists and is not bad; its three d_kf_imu indices are held against their ranges.  Nothing is skipped -- the inertial
//      chain is positional -- so an unusable position refuses the call here: the counts, return
//   2  a thread per slot of a window key frame: work_row[p] = the least (position << 13 | slot) naming the valid row p (atomicMin)
//   3  the slots IN ORDER, a tile of 1024 at a time: a slot whose key is its row's is the row's first occurrence; its thread walks the
//      row's live entries and gives every key frame outside the window work_first[f] = the least key of a row it observes (atomicMin
//      again: an integer minimum does not depend on the order)
//   4  the cap: X = the max_fixed-th smallest work_first[] by a counting binary search over the keys (<= 18 rounds of a block count),
//      every key when fewer key frames than max_fixed have one; the key frames with work_first[f] <= X are the fixed states, numbered
//      in ascending slot order behind the window by a block scan -> work_kf[f]
//   5  the slots in order again: the row's edges counted -- live entries, a key frame's first entry only, on a state only --, a
//      block scan of (has an edge, edges) over the tile numbers points and edges, and the thread walks the list again to write them
//   6  the counts and the refusal; refused: return
//   7  a thread per edge (measurement, information) and per state (the job lists)
// A row's key orders the rows as their numbers do, so the reference's "push every observer of this point, then break" is the set
// {f : first[f] <= X} whatever the order the atomics ran in.  Counts are sums and every stored value is decided by the slot arrays
// alone: the bytes are the same on every run.  Integer atomics only; no scratch memory, no handle scratch, no allocation, no host wait.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/orbi.h"
#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orbm_internal.h"
#include "orbm_map.h"

namespace {

constexpr int IW_T = 1024;              // the one workgroup
constexpr int IW_WAVES = IW_T / 64;
constexpr int IW_MAX_OBS = 256;         // edges per point beyond which the linearisation drops the point whole
static_assert(ORBM_IW_MAX_SOLVE <= MAP_MAX_RECENT && ORBM_IW_MAX_SOLVE <= IW_T, "a thread per entry of d_window, a position in the key's upper bits");
static_assert(sizeof(orbi_edge) == 4 * sizeof(int32_t) && sizeof(orbi_prior_job) == 3 * sizeof(int32_t), "the job lists are int32 arrays in orbm.h");
static_assert(sizeof(orbi_prior) == 36 * sizeof(float) && offsetof(orbi_prior, velo_priori) == 0, "orbi_prior as the velocity prior writes it");

// d_result of the assembly (int32 x 16) and of the velocity prior (int32 x 8)
enum { W_STATES = 0, W_POINTS = 1, W_EDGES = 2, W_SOLVE = 3, W_FIXED = 4, W_REFUSED = 5, W_WINDOW_UNUSABLE = 6, W_IMU_RANGE = 7, W_NO_EDGE = 8,
       W_SECOND = 9, W_CSR_DROPPED = 10, W_CAPPED = 11, W_LONG = 12, W_CANDIDATES = 13 };
enum { REFUSE_STATES = 1, REFUSE_POINTS = 2, REFUSE_EDGES = 4, REFUSE_WINDOW = 8, REFUSE_NO_EDGE = 16, REFUSE_IMU = 32 };
enum { V_DONE = 0, V_RANGE = 1 };

struct WindowArgs {
    MapReadView m;
    const void *const *kps;
    const float *points;
    const int32_t *window, *kf_imu;
    int n_window, n_src, cap_bank, n_priors, max_fixed, cap_states, cap_local_points, cap_edges;
    int32_t *work;                       // [cap_points] row keys, [n_kf] the key frames' states, [n_kf] their first keys
    double *o_points;
    int32_t *o_point_row, *o_edge_off, *o_edge_state, *o_edge_point;
    double *o_edge_z, *o_edge_inv_sigma2;
    int32_t *o_edge_kf, *o_edge_kp, *o_state_kf;
    int32_t *o_init_jobs;
    uint8_t *o_fixed;
    int32_t *o_inertial_edges, *o_prior_jobs, *o_recover_jobs, *o_bias_ids, *o_prior_info_jobs;
    int32_t *result;
};

// The edges of row p: its live CSR entries in CSR order, the first entry of a key frame only, on a key frame that is a state.
// WRITE = false: count them, the second entries and the entries behind the cap; true: write edge number e0, e0 + 1, ...
template <bool WRITE>
__device__ __forceinline__ int window_edges(const WindowArgs &a, const int32_t *work_kf, int p, int idx, int e0, int &second, int &capped)
{
    int b, e, n = 0;
    map_list(a.m, p, b, e);
    for (int j = b; j < e; ++j) {
        int k, i;
        if (!map_live_entry(a.m, j, p, k, i)) continue;
        if (map_second_entry(a.m, b, j, p, k)) {                   // a key frame twice: the linearisation would drop the later edge
            second += !WRITE;
            continue;
        }
        const int s = work_kf[k];
        if (s == MAP_NONE) {                                       // a live key frame behind the cap: the reference's null vertex
            capped += !WRITE;
            continue;
        }
        if (WRITE) {
            const int x = e0 + n;
            if (x < a.cap_edges) a.o_edge_kf[x] = k, a.o_edge_kp[x] = i, a.o_edge_point[x] = idx, a.o_edge_state[x] = s;
        }
        ++n;
    }
    return n;
}

__global__ __launch_bounds__(IW_T) void k_iw_problem(const WindowArgs a)
{
    __shared__ int s_window[ORBM_IW_MAX_SOLVE];                    // the window's key frames by position
    __shared__ int s_wave[2][IW_WAVES];
    __shared__ int s_count[16];
    const int tid = threadIdx.x;
    const MapReadView &m = a.m;
    int32_t *work_row = a.work, *work_kf = a.work + m.cap_points, *work_first = work_kf + m.n_kf;
    const int n_solve = a.n_window;
    // ---- 0
    for (int p = tid; p < m.cap_points; p += IW_T) work_row[p] = MAP_NONE;
    for (int k = tid; k < 2 * m.n_kf; k += IW_T) work_kf[k] = MAP_NONE;   // the states and the first keys
    if (tid < 16) s_count[tid] = 0;
    int csr_dropped = 0, no_edge = 0, second = 0, capped = 0, too_long = 0, imu_range = 0;   // per thread, summed at the end
    for (int j = tid; j < m.n_obs; j += IW_T) csr_dropped += !map_usable(m, m.obs_kf[j], m.obs_kp[j]);
    __syncthreads();
    // ---- 1: the solve states (Optimize.cpp:1076-1079): position s is d_window[s], nothing is skipped
    const int mine = tid < n_solve ? a.window[tid] : -1;
    const bool in_range = tid < n_solve && mine >= 0 && mine < m.n_kf;
    if (in_range) atomicMin(&work_kf[mine], tid);
    __syncthreads();
    const bool usable = in_range && work_kf[mine] == tid && m.bad[mine] == 0;
    if (usable) {
        const int row = a.kf_imu[(size_t)mine * 3], rec = a.kf_imu[(size_t)mine * 3 + 1], prior = a.kf_imu[(size_t)mine * 3 + 2];
        imu_range += row < 0 || row >= a.n_src || rec < 0 || rec >= a.cap_bank || prior < 0 || prior >= a.n_priors;
    }
    if (tid < n_solve) s_window[tid] = usable ? mine : 0;          // read only when every position is usable
    int n_unusable;
    block_scan<IW_WAVES>(tid < n_solve && !usable, s_wave[0], n_unusable);
    if (n_unusable) {                                              // the same in every thread
        if (tid < 16)
            a.result[tid] = tid == W_STATES || tid == W_SOLVE ? n_solve : tid == W_REFUSED ? (int)REFUSE_WINDOW : tid == W_WINDOW_UNUSABLE ? n_unusable : 0;
        return;
    }
    // ---- 2: the rows named by a slot of a window key frame, and where first (:1083-1092)
    const int total = n_solve * m.stride;                          // <= 32 * 8192
    map_mark_first<IW_T>(s_window, n_solve, m, work_row);
    __syncthreads();
    // ---- 3: per key frame outside the window, the first local point that it observes (:1097-1105)
    for (int t0 = 0; t0 < total; t0 += IW_T) {
        const int p = map_first_at(s_window, total, m, work_row, t0 + tid);
        if (p < 0) continue;
        const int key = work_row[p];
        int b, e, k, i;
        map_list(m, p, b, e);
        for (int j = b; j < e; ++j)
            if (map_live_entry(m, j, p, k, i) && work_kf[k] == MAP_NONE) atomicMin(&work_first[k], key);
    }
    __syncthreads();
    // ---- 4: the cap (:1107) and the fixed states in ascending slot order
    int mark = 0, n_candidates;
    for (int k = tid; k < m.n_kf; k += IW_T) mark += work_first[k] != MAP_NONE;
    block_scan<IW_WAVES>(mark, s_wave[0], n_candidates);
    int X = MAP_NONE - 1;                                          // every key
    if (n_candidates >= a.max_fixed) {                             // the least X with #{f : first[f] <= X} >= max_fixed
        int lo = 0, hi = (n_solve << MAP_KEY_SHIFT) - 1;           // the count at hi is n_candidates
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            int below = 0, n_below;
            for (int k = tid; k < m.n_kf; k += IW_T) below += work_first[k] <= mid;
            block_scan<IW_WAVES>(below, s_wave[0], n_below);
            if (n_below >= a.max_fixed) hi = mid;
            else lo = mid + 1;
        }
        X = lo;
    }
    int n_fixed = 0;
    for (int k0 = 0; k0 < m.n_kf; k0 += IW_T) {
        const int k = k0 + tid;
        const bool fixed = k < m.n_kf && work_first[k] <= X;
        int tile;
        const int my = block_scan<IW_WAVES>(fixed, s_wave[0], tile);
        if (fixed) {
            const int q = n_solve + n_fixed + my, row = a.kf_imu[(size_t)k * 3];
            imu_range += row < 0 || row >= a.n_src;
            work_kf[k] = q;
            if (q < a.cap_states) a.o_state_kf[q] = k;
        }
        n_fixed += tile;
    }
    if (tid < n_solve && tid < a.cap_states) a.o_state_kf[tid] = s_window[tid];
    __syncthreads();
    // ---- 5: points and edges in the order of first occurrence (:1218-1244)
    int n_points = 0, n_edges = 0;                                  // the same in every thread
    for (int t0 = 0; t0 < total; t0 += IW_T) {
        const int p = map_first_at(s_window, total, m, work_row, t0 + tid);
        const bool is_first = p >= 0;
        int cnt = 0;
        if (is_first) cnt = window_edges<false>(a, work_kf, p, 0, 0, second, capped);
        const bool has = is_first && cnt > 0;
        no_edge += is_first && cnt == 0;
        too_long += cnt > IW_MAX_OBS;
        int my_point, my_edge, tile_points, tile_edges;
        block_scan2<IW_WAVES>(has, cnt, s_wave, my_point, my_edge, tile_points, tile_edges);
        if (has) {
            const int idx = n_points + my_point, e0 = n_edges + my_edge;
            if (idx < a.cap_local_points) {
                a.o_point_row[idx] = p, a.o_edge_off[idx] = e0;
                for (int c = 0; c < 3; ++c) a.o_points[(size_t)idx * 3 + c] = (double)a.points[(size_t)p * 3 + c];
            }
            window_edges<true>(a, work_kf, p, idx, e0, second, capped);
        }
        n_points += tile_points, n_edges += tile_edges;
    }
    // ---- 6: the counts and the refusal
    const int n_states = n_solve + n_fixed;
    block_add(s_count, {W_CSR_DROPPED, W_NO_EDGE, W_SECOND, W_CAPPED, W_LONG, W_IMU_RANGE}, {csr_dropped, no_edge, second, capped, too_long, imu_range});
    __syncthreads();                                               // the edges' key frames and o_state_kf as well
    const int refused = (n_states > a.cap_states) * REFUSE_STATES | (n_points > a.cap_local_points) * REFUSE_POINTS |
                        (n_edges > a.cap_edges) * REFUSE_EDGES | (n_edges < 1) * REFUSE_NO_EDGE | (s_count[W_IMU_RANGE] != 0) * REFUSE_IMU;
    __syncthreads();
    if (tid == 0) {
        s_count[W_STATES] = n_states, s_count[W_POINTS] = n_points, s_count[W_EDGES] = n_edges, s_count[W_SOLVE] = n_solve;
        s_count[W_FIXED] = n_fixed, s_count[W_REFUSED] = refused, s_count[W_CANDIDATES] = n_candidates;
        if (n_points <= a.cap_local_points) a.o_edge_off[n_points] = n_edges;
    }
    __syncthreads();
    if (tid < 16) a.result[tid] = s_count[tid];
    if (refused) return;
    // ---- 7: the edges' measurements (:1228-1234) and the job lists of the inertial side (:1133-1197, :1276-1299)
    for (int x = tid; x < n_edges; x += IW_T) {
        map_edge_measurement(a.kps, a.o_edge_kf[x], a.o_edge_kp[x], a.o_edge_z + (size_t)x * 2, a.o_edge_inv_sigma2 + x);   // :1228-1234
    }
    for (int q = tid; q < n_states; q += IW_T) {
        const int k = a.o_state_kf[q];
        const int row = a.kf_imu[(size_t)k * 3], rec = a.kf_imu[(size_t)k * 3 + 1], prior = a.kf_imu[(size_t)k * 3 + 2];
        const bool solve = q < n_solve;
        int32_t *init = a.o_init_jobs + (size_t)q * 3;
        init[0] = q, init[1] = row, init[2] = solve ? rec : -1;    // a fixed state has no bias vertices (:1200-1205)
        a.o_fixed[q] = solve ? 0 : ORBI_FIX_POSE | ORBI_FIX_VELO | ORBI_FIX_GYRO | ORBI_FIX_ACC;
        if (!solve) continue;
        int32_t *rj = a.o_recover_jobs + (size_t)q * 3;
        rj[0] = q, rj[1] = row, rj[2] = ORBI_RECOVER_POSE;
        a.o_bias_ids[q] = rec;
        if (q + 1 < n_solve) {                                     // :1153-1174: the OLDER key frame's pre-integrator, its C for both walks
            int32_t *ie = a.o_inertial_edges + (size_t)q * 4;
            ie[0] = q, ie[1] = q + 1, ie[2] = rec, ie[3] = ORBI_EDGE_WALKS;
        }
        if (q == 0) {                                              // :1176-1191
            a.o_prior_jobs[0] = 0, a.o_prior_jobs[1] = prior;
            a.o_prior_jobs[2] = ORBI_PRIOR_VELO | ORBI_PRIOR_GYRO | ORBI_PRIOR_ACC | ORBI_PRIOR_ACC_GYRO_INFO;
        } else {                                                   // :1293-1296: C of the key frame before, whose new bias is bias_priori
            int32_t *pj = a.o_prior_info_jobs + (size_t)(q - 1) * 3;
            pj[0] = prior, pj[1] = a.kf_imu[(size_t)a.o_state_kf[q - 1] * 3 + 1], pj[2] = row;
        }
    }
}

// KeyFrame::setVelocity's velo_priori = velo (KeyFrame.cpp:65-69) for the oldest key frame, which no prior-information job names
__global__ __launch_bounds__(64) void k_iw_velocity_prior(orbi_prior *priors, int n_priors, const float *src, int n_src, const int32_t *recover_jobs,
                                                          const int32_t *prior_jobs, int32_t *result)
{
    const int tid = threadIdx.x, row = recover_jobs[1], prior = prior_jobs[1];
    const bool ok = row >= 0 && row < n_src && prior >= 0 && prior < n_priors;
    if (ok && tid < 3) priors[prior].velo_priori[tid] = src[(size_t)row * 15 + 12 + tid];
    if (tid < 8) result[tid] = tid == V_DONE ? ok : tid == V_RANGE ? !ok : 0;
}

} // namespace

extern "C" int orbm_inertial_window_problem_device(orbm_t *h, const orbm_kf_table *kf, const int32_t *d_slots, int stride, const uint8_t *d_valid,
                                                   const float *d_points, int cap_points, const int32_t *d_obs_off, const int32_t *d_obs_kf,
                                                   const int32_t *d_obs_kp, int n_obs, const int32_t *d_window, int n_window,
                                                   const int32_t *d_kf_imu, int n_src, int cap_bank, int n_priors, int max_fixed, int cap_states,
                                                   int cap_local_points, int cap_edges, int32_t *d_work, double *d_ba_points,
                                                   int32_t *d_point_row, int32_t *d_edge_off, int32_t *d_edge_state, int32_t *d_edge_point,
                                                   double *d_edge_z, double *d_edge_inv_sigma2, int32_t *d_edge_kf, int32_t *d_edge_kp,
                                                   int32_t *d_state_kf, int32_t *d_init_jobs, uint8_t *d_fixed, int32_t *d_inertial_edges,
                                                   int32_t *d_prior_jobs, int32_t *d_recover_jobs, int32_t *d_bias_ids,
                                                   int32_t *d_prior_info_jobs, int32_t *d_result, void *stream)
{
    if (!kf || !d_result || !d_window || !d_kf_imu) return orbx_set_error(ORBX_E_ARG, "null argument");
    WindowArgs a = {};
    if (int rc = orbm_map_view(&a.m, kf->n_kf, kf->d_n, kf->d_bad, d_slots, stride, d_valid, cap_points, d_obs_off, d_obs_kf, d_obs_kp, n_obs)) return rc;
    if (n_window < 1 || max_fixed < 1 || cap_states < 1 || cap_local_points < 1 || cap_edges < 1)
        return orbx_set_error(ORBX_E_ARG, "n_window, max_fixed and the capacities must be positive");
    if (n_src < 0 || cap_bank < 0 || n_priors < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (kf->n_kf > 0 && !kf->d_kps) return orbx_set_error(ORBX_E_ARG, "null key-frame array");
    if (cap_points > 0 && !d_points) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if (!d_work || !d_ba_points || !d_point_row || !d_edge_off || !d_edge_state || !d_edge_point || !d_edge_z || !d_edge_inv_sigma2 || !d_edge_kf ||
        !d_edge_kp || !d_state_kf || !d_init_jobs || !d_fixed || !d_inertial_edges || !d_prior_jobs || !d_recover_jobs || !d_bias_ids || !d_prior_info_jobs)
        return orbx_set_error(ORBX_E_ARG, "null output array");
    if (int rc = orbm_check_kf_rows(kf->d_kps)) return rc;
    if (n_window > ORBM_IW_MAX_SOLVE) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBM_IW_MAX_SOLVE (32) entries in d_window");
    if (int rc = orbm_check_stride(stride)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    a.kps = kf->d_kps, a.points = d_points, a.window = d_window, a.kf_imu = d_kf_imu;
    a.n_window = n_window, a.n_src = n_src, a.cap_bank = cap_bank, a.n_priors = n_priors, a.max_fixed = max_fixed;
    a.cap_states = cap_states, a.cap_local_points = cap_local_points, a.cap_edges = cap_edges, a.work = d_work;
    a.o_points = d_ba_points, a.o_point_row = d_point_row, a.o_edge_off = d_edge_off, a.o_edge_state = d_edge_state, a.o_edge_point = d_edge_point;
    a.o_edge_z = d_edge_z, a.o_edge_inv_sigma2 = d_edge_inv_sigma2, a.o_edge_kf = d_edge_kf, a.o_edge_kp = d_edge_kp, a.o_state_kf = d_state_kf;
    a.o_init_jobs = d_init_jobs, a.o_fixed = d_fixed, a.o_inertial_edges = d_inertial_edges, a.o_prior_jobs = d_prior_jobs;
    a.o_recover_jobs = d_recover_jobs, a.o_bias_ids = d_bias_ids, a.o_prior_info_jobs = d_prior_info_jobs, a.result = d_result;
    hipLaunchKernelGGL(k_iw_problem, dim3(1), dim3(IW_T), 0, s, a);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_inertial_window_velocity_prior_device(orbm_t *h, struct orbi_prior *d_priors, int n_priors, const float *d_src, int n_src,
                                                          const int32_t *d_recover_jobs, const int32_t *d_prior_jobs, int32_t *d_result, void *stream)
{
    if (!d_priors || !d_src || !d_recover_jobs || !d_prior_jobs || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (n_priors < 0 || n_src < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    hipLaunchKernelGGL(k_iw_velocity_prior, dim3(1), dim3(64), 0, s, d_priors, n_priors, d_src, n_src, d_recover_jobs, d_prior_jobs, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
