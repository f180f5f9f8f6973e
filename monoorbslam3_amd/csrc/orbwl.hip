// The device side of localFullBundleAdjustment's Levenberg-Marquardt loop (include/orbwl.h): what runs between the stage calls.
//   k_vwl_begin    the control block, the summary and *d_lambda at the start of an optimisation
//   k_vwl_push     g2o's push: Rwb, twb, v, bg, ba and d_iter of the solve states into the saved slice
//   k_vwl_decide   g2o's policy behind a trial's error evaluation, the pop, the trace row, the counters and the verdict
//   k_vwl_end      the summary and d_result behind the classification
// Each is ONE workgroup in ONE launch, bounded by the sizes the host checked; there is no inter-workgroup synchronisation and no
// spin-wait.  No stage formula is here: the stages are the library's staged entry points, which the host driver calls in the chain's
// order; the policy's arithmetic is orb_lm_policy.h's.  The decision is taken by ONE lane, published through LDS and read by the
// workgroup behind a barrier that is in uniform control flow.
#include <hip/hip_runtime.h>

#include "orb_lm_policy.h"
#include "orbwl_kernels.h"

#pragma clang fp contract(off)

static_assert(sizeof(orbwl_loop_options) == 48, "orbwl.h fixes this layout");
static_assert(ORBWL_TRACE == LM_TRACE_ROW && ORBWL_SUMMARY == 8, "orbwl.h states a row of the trace, which lm_trace_row writes, and the summary");

namespace {

constexpr int WL_T = 256;

// entry k of a state's 21 doubles (Rwb, twb, v, bg, ba), as push and pop walk them
__device__ __forceinline__ double *wl_vertex_word(const orbi_graph &g, int s, int k)
{
    return k < 9 ? g.Rwb + 9 * (size_t)s + k : k < 12 ? g.twb + 3 * (size_t)s + k - 9 : k < 15 ? g.v + 3 * (size_t)s + k - 12 : k < 18 ? g.bg + 3 * (size_t)s + k - 15
                                                                                                                                   : g.ba + 3 * (size_t)s + k - 18;
}

__global__ __launch_bounds__(64) void k_vwl_begin(double *__restrict__ ctrl, double *__restrict__ summary, double *__restrict__ lambda, double lambda_init)
{
    const int t = threadIdx.x;
    if (t < WL_CTRL_DOUBLES) ctrl[t] = 0.0;                        // the counters are int32 zeros as well
    if (t < ORBWL_SUMMARY) summary[t] = 0.0;
    __syncthreads();
    if (t == 0) ctrl[WLC_NI] = 2.0, *lambda = lambda_init;         // setUserLambdaInit; _ni = 2 at iteration 0
}

__global__ __launch_bounds__(WL_T) void k_vwl_push(const orbi_graph g, const int32_t *__restrict__ iter, int n_solve, double *__restrict__ saved,
                                                   int32_t *__restrict__ saved_iter)
{
    for (int k = threadIdx.x; k < 21 * n_solve; k += WL_T) saved[k] = *wl_vertex_word(g, k / 21, k % 21);
    for (int k = threadIdx.x; k < n_solve; k += WL_T) saved_iter[k] = iter[k];
}

__global__ __launch_bounds__(WL_T) void k_vwl_decide(const WlDecide a)
{
    __shared__ int s_pop;
    if (threadIdx.x == 0) {
        int32_t *q = reinterpret_cast<int32_t *>(a.ctrl + WLC_INTS);
        LmPolicy p = {*a.lambda, a.ctrl[WLC_NI], a.ctrl[WLC_CURRENT], a.ctrl[WLC_RHO], q[WLI_QMAX]};
        if (a.first) lm_policy_iteration(p, a.lin_inertial[1] + a.lin_visual[1]);   // computeActiveErrors, activeRobustChi2
        const double lam = p.lam, current = p.current;
        const int it = q[WLI_IT], trial = p.qmax;
        const bool ok = a.solve_result[ORBI_R_DONE] == 1 && a.solve_result[ORBI_R_REFUSED] == 0;
        const double ti = a.try_inertial[1], tv = a.try_visual[1], scale_pose = a.out[0], scale_points = a.out_points[0];
        const LmTrial t = lm_policy_trial(p, ok, ti, tv, scale_pose, scale_points);
        const int row = q[WLI_ROWS];
        if (row < a.cap_trace) lm_trace_row(a.trace + (size_t)ORBWL_TRACE * row, it, trial, lam, current, t, ok, ti, tv, scale_pose, scale_points);
        q[WLI_ROWS] = row + 1;
        if (t.accepted) ++q[WLI_ACCEPTED]; else ++q[WLI_REJECTED];
        if (!ok) ++q[WLI_REFUSED];
        int next = WL_NEXT_TRIAL;
        if (!lm_policy_again(p, t, a.max_trials)) {
            ++q[WLI_ITS];
            q[WLI_IT] = it + 1;
            next = lm_policy_terminate(p, a.max_trials) || it + 1 >= a.iterations ? WL_NEXT_END : WL_NEXT_ITERATION;
        }
        *a.lambda = p.lam, a.ctrl[WLC_NI] = p.ni, a.ctrl[WLC_CURRENT] = p.current, a.ctrl[WLC_RHO] = p.rho, q[WLI_QMAX] = p.qmax;
        a.verdict[WLV_NEXT] = next, a.verdict[WLV_ACCEPTED] = t.accepted, a.verdict[WLV_REFUSED] = !ok, a.verdict[WLV_TRIALS] = row + 1;
        s_pop = !t.accepted;
    }
    __syncthreads();
    if (s_pop) {                                                   // pop: the vertices and their update counters
        for (int k = threadIdx.x; k < 21 * a.n_solve; k += WL_T) *wl_vertex_word(a.g, k / 21, k % 21) = a.saved[k];
        for (int k = threadIdx.x; k < a.n_solve; k += WL_T) a.iter[k] = a.saved_iter[k];
    }
}

__global__ __launch_bounds__(64) void k_vwl_end(const WlEnd a)
{
    const int t = threadIdx.x;
    const int32_t *q = reinterpret_cast<const int32_t *>(a.ctrl + WLC_INTS);
    const int rows = q[WLI_ROWS], ran = rows > 0;
    const int outliers = a.classify_result[ORBWL_R_OUTLIER];
    if (t == 0) {
        double *sm = a.summary;
        sm[0] = q[WLI_ITS], sm[1] = rows, sm[2] = q[WLI_ACCEPTED], sm[3] = q[WLI_REFUSED], sm[4] = *a.lambda, sm[5] = outliers;
        sm[6] = rows > a.cap_trace ? rows - a.cap_trace : 0, sm[7] = a.stopped;
    }
    if (t < 8) {
        int v = 0;
        if (t == ORBI_R_DONE) v = q[WLI_ACCEPTED];
        else if (t == ORBI_R_RANGE) v = a.classify_result[ORBI_R_RANGE] + (ran ? a.inertial_result[ORBI_R_RANGE] : 0);
        else if (t == ORBWL_R_REJECTED) v = q[WLI_REJECTED];
        else if (t == ORBI_R_REFUSED) v = q[WLI_REFUSED];
        else if (t == ORBVI_R_NONFINITE) v = a.classify_result[ORBVI_R_NONFINITE];
        else if (t == ORBWL_R_OUTLIER) v = outliers;
        else if (t == ORBWL_R_POINT_SINGULAR) v = ran ? a.reduce_result[ORBWL_R_POINT_SINGULAR] : 0;
        a.result[t] = v;
    }
}

} // namespace

hipError_t wl_launch_begin(double *ctrl, double *summary, double *lambda, double lambda_init, hipStream_t s)
{
    hipLaunchKernelGGL(k_vwl_begin, dim3(1), dim3(64), 0, s, ctrl, summary, lambda, lambda_init);
    return hipGetLastError();
}

hipError_t wl_launch_push(orbi_graph g, const int32_t *iter, int n_solve, double *saved, int32_t *saved_iter, hipStream_t s)
{
    hipLaunchKernelGGL(k_vwl_push, dim3(1), dim3(WL_T), 0, s, g, iter, n_solve, saved, saved_iter);
    return hipGetLastError();
}

hipError_t wl_launch_decide(const WlDecide &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_vwl_decide, dim3(1), dim3(WL_T), 0, s, a);
    return hipGetLastError();
}

hipError_t wl_launch_end(const WlEnd &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_vwl_end, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}
