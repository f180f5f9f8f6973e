// The chain of localInertialBundleAdjustment assembled from the device-resident map (include/orbm.h, "The inertial chain on the
// device-resident map"): steps 1 and 3 of Optimize::localInertialBundleAdjustment (Optimize.cpp:965-1029) as
//   orbm_inertial_chain_problem_device            the states of getRecentKeyFrames(numOpt), their fixed flags and the job lists of the
//                                                 inertial-factor calls (orbi_factors.h) and of the call below
//   orbm_inertial_chain_velocity_priors_device    what KeyFrame::setVelocity leaves in velo_priori of EVERY window key frame (:1044-1053)
// The optimisation between them is orbil_chain_optimize_device (orbil.h), one launch; the host knows every size, so the chain of the
// mapper step reads nothing back.
//
// The assembly is ONE launch of ONE workgroup of 64 threads, a thread per window position, integer work only.  The rule of the window
// assembly (orbm_inertial_window.hip) holds: the chain is positional, nothing is skipped, so an entry that is out of range, bad or named
// by an earlier entry, or a d_kf_imu index out of range, REFUSES the call -- and the refusal is honoured on the device: every job list is
// written with -1 entries and d_fixed with 15, which every call behind it drops by its own distrust.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/orbi.h"
#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orbm_internal.h"

namespace {

constexpr int IC_T = 64;
static_assert(ORBM_IC_MAX_WINDOW <= IC_T, "a thread per entry of d_window");
static_assert(sizeof(orbi_edge) == 4 * sizeof(int32_t), "the job lists are int32 arrays in orbm.h");
static_assert(sizeof(orbi_prior) == 36 * sizeof(float) && offsetof(orbi_prior, velo_priori) == 0, "orbi_prior as the velocity priors write it");

// d_result of the assembly and of the velocity priors (int32 x 8 each)
enum { C_STATES = 0, C_REFUSED = 1, C_WINDOW_UNUSABLE = 2, C_IMU_RANGE = 3 };
enum { REFUSE_WINDOW = 8, REFUSE_IMU = 32 };                       // the window assembly's bits
enum { V_DONE = 0, V_RANGE = 1 };

__global__ __launch_bounds__(IC_T) void k_ic_problem(int n_kf, const uint8_t *__restrict__ bad, const int32_t *__restrict__ window, int n,
                                                     const int32_t *__restrict__ kf_imu, int n_src, int cap_bank, int n_priors, int32_t *__restrict__ o_init_jobs,
                                                     uint8_t *__restrict__ o_fixed, int32_t *__restrict__ o_edges, int32_t *__restrict__ o_recover_jobs,
                                                     int32_t *__restrict__ o_bias_ids, int32_t *__restrict__ o_velo_jobs, int32_t *__restrict__ o_state_kf,
                                                     int32_t *__restrict__ result)
{
    __shared__ int s_window[ORBM_IC_MAX_WINDOW];
    __shared__ int s_rec[ORBM_IC_MAX_WINDOW];
    __shared__ int s_count[8];
    const int s = threadIdx.x;
    if (s < 8) s_count[s] = 0;
    const int mine = s < n ? window[s] : -1;
    if (s < n) s_window[s] = mine;
    __syncthreads();
    // Optimize.cpp:965-972: position s is d_window[s]; usable: inside the table, not bad, named by no earlier position
    bool usable = s < n && mine >= 0 && mine < n_kf && bad[mine] == 0;
    for (int q = 0; usable && q < s; ++q) usable = s_window[q] != mine;
    int row = -1, rec = -1, prior = -1;
    bool imu_range = false;
    if (usable) {
        row = kf_imu[(size_t)mine * 3], rec = kf_imu[(size_t)mine * 3 + 1], prior = kf_imu[(size_t)mine * 3 + 2];
        imu_range = row < 0 || row >= n_src || rec < 0 || rec >= cap_bank || prior < 0 || prior >= n_priors;
    }
    block_add(s_count, {C_WINDOW_UNUSABLE, C_IMU_RANGE}, {(int)(s < n && !usable), (int)imu_range});
    if (s < n) s_rec[s] = rec;
    __syncthreads();
    const int refused = (s_count[C_WINDOW_UNUSABLE] != 0) * REFUSE_WINDOW | (s_count[C_IMU_RANGE] != 0) * REFUSE_IMU;   // the same in every thread
    if (s < 8) result[s] = s == C_STATES ? n : s == C_REFUSED ? refused : s == C_WINDOW_UNUSABLE || s == C_IMU_RANGE ? s_count[s] : 0;
    if (s >= n) return;
    const int none = -1;
    int32_t *init = o_init_jobs + (size_t)s * 3, *rj = o_recover_jobs + (size_t)s * 3, *vj = o_velo_jobs + (size_t)s * 2;
    if (refused) {                                                 // every job behind drops itself; every vertex is fixed
        init[0] = init[1] = init[2] = none, rj[0] = rj[1] = rj[2] = none, vj[0] = vj[1] = none;
        o_fixed[s] = ORBI_FIX_POSE | ORBI_FIX_VELO | ORBI_FIX_GYRO | ORBI_FIX_ACC, o_bias_ids[s] = none, o_state_kf[s] = none;
        if (s + 1 < n) {
            int32_t *ie = o_edges + (size_t)s * 4;
            ie[0] = ie[1] = ie[2] = ie[3] = none;
        }
        return;
    }
    init[0] = s, init[1] = row, init[2] = rec;                     // :992-1007 the velocity and both biases of every key frame
    // setFixed(i == 0) on the three vertices of the oldest; the poses are constants of EdgeInertialOnly: no pose vertex at all
    o_fixed[s] = s == 0 ? ORBI_FIX_POSE | ORBI_FIX_VELO | ORBI_FIX_GYRO | ORBI_FIX_ACC : ORBI_FIX_POSE;
    rj[0] = s, rj[1] = row, rj[2] = 0;                             // :1044-1053 velocity and bias; the pose was never a vertex
    o_bias_ids[s] = rec;
    vj[0] = row, vj[1] = prior;
    o_state_kf[s] = mine;
    if (s + 1 < n) {                                               // :1012-1029: the OLDER key frame's pre-integrator, its C for both walks
        int32_t *ie = o_edges + (size_t)s * 4;
        ie[0] = s, ie[1] = s + 1, ie[2] = s_rec[s], ie[3] = ORBI_EDGE_WALKS;
    }
}

// KeyFrame::setVelocity's velo_priori = velo (KeyFrame.cpp:65-69), a thread per job and float
__global__ __launch_bounds__(64) void k_ic_velocity_priors(orbi_prior *priors, int n_priors, const float *__restrict__ src, int n_src,
                                                           const int32_t *__restrict__ jobs, int n, int32_t *__restrict__ result)
{
    __shared__ int s_cnt[8];
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int x = threadIdx.x; x < 3 * n; x += 64) {
        const int job = x / 3, c = x - 3 * job, row = jobs[2 * job], prior = jobs[2 * job + 1];
        const bool ok = row >= 0 && row < n_src && prior >= 0 && prior < n_priors;
        if (ok) priors[prior].velo_priori[c] = src[(size_t)row * 15 + 12 + c];
        if (c == 0) atomicAdd(&s_cnt[ok ? V_DONE : V_RANGE], 1);
    }
    __syncthreads();
    flush_counts(s_cnt, result);
}

} // namespace

extern "C" int orbm_inertial_chain_problem_device(orbm_t *h, int n_kf, const uint8_t *d_bad, const int32_t *d_window, int n_window,
                                                  const int32_t *d_kf_imu, int n_src, int cap_bank, int n_priors, int32_t *d_init_jobs,
                                                  uint8_t *d_fixed, int32_t *d_inertial_edges, int32_t *d_recover_jobs, int32_t *d_bias_ids,
                                                  int32_t *d_velo_jobs, int32_t *d_state_kf, int32_t *d_result, void *stream)
{
    if (!d_bad || !d_window || !d_kf_imu || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (!d_init_jobs || !d_fixed || !d_inertial_edges || !d_recover_jobs || !d_bias_ids || !d_velo_jobs || !d_state_kf)
        return orbx_set_error(ORBX_E_ARG, "null output array");
    if (n_window < 2) return orbx_set_error(ORBX_E_ARG, "a chain has at least 2 key frames");
    if (n_kf < 0 || n_src < 0 || cap_bank < 0 || n_priors < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (n_window > ORBM_IC_MAX_WINDOW) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBM_IC_MAX_WINDOW (20) entries in d_window");
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    hipLaunchKernelGGL(k_ic_problem, dim3(1), dim3(IC_T), 0, s, n_kf, d_bad, d_window, n_window, d_kf_imu, n_src, cap_bank, n_priors, d_init_jobs, d_fixed,
                       d_inertial_edges, d_recover_jobs, d_bias_ids, d_velo_jobs, d_state_kf, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_inertial_chain_velocity_priors_device(orbm_t *h, struct orbi_prior *d_priors, int n_priors, const float *d_src, int n_src,
                                                          const int32_t *d_velo_jobs, int n, int32_t *d_result, void *stream)
{
    if (!d_priors || !d_src || !d_velo_jobs || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (n_priors < 0 || n_src < 0 || n < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (n > ORBM_IC_MAX_WINDOW) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBM_IC_MAX_WINDOW (20) jobs");
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    hipLaunchKernelGGL(k_ic_velocity_priors, dim3(1), dim3(64), 0, s, d_priors, n_priors, d_src, n_src, d_velo_jobs, n, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
