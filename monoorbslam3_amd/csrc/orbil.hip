// localInertialBundleAdjustment on the device (include/orbil.h):
//   orbil_chain_solve_device      (H + lambda*I)*dx = b of a chain of inertial states, block-tridiagonal, by a walk along its band
//   orbil_chain_optimize_device   optimize(10), g2o's Levenberg-Marquardt policy, push / pop                          Optimize.cpp:1031-1036
//
// Both kernels are one workgroup.  Every stage is a device function of csrc/orbvi_stages.h: the band walk (chain_solve_assemble,
// chain_solve_largest, chain_solve_wave) is defined there once and run by both kernels, and the loop's linearisation, gather and update
// are the functions k_fac_edge, k_fac_gather and k_fac_oplus run (orbi_factors.hip), so no formula is restated here and a stage inside the
// loop gives the bytes of the staged call on the same input.  Nor is the trial policy's arithmetic: it is orb_lm_policy.h's, run by one
// lane.  What is here is the step machine around it, in the shape of k_vi_pose_loop (orbvi_loop.hip) with one round and no visual group:
// a sequence of STEPS, each LIN (the linearisation at the estimate, mode 0) or TRIAL (the errors at a trial point, mode 1); behind the
// evaluation ONE LANE (thread 0) takes the policy's decision and publishes it through LDS; behind a barrier every thread reads it and the
// workgroup pops, pushes, solves and updates as it says.  Every barrier is in control flow that is uniform across the workgroup, and the
// step count is bounded by what the host computed from the checked options: iterations * (1 + max_trials) + 1.  There is no second
// workgroup, no spin-wait and no floating-point atomic.  Global memory that the workgroup wrote (the graph, the blocks and the band in
// the caller's scratch) is read back behind a barrier only; inside the solve's one wave, behind that wave's fence.
//
// LDS.  Eight waves linearise eight edges of a pass, each in its own slice (57 KB).  The solve's tile and vectors (16 KB) LIE OVER those
// slices: a barrier separates every evaluation from every solve, so the two are never live together and the kernel stays below 64 KB.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include <string>

#include "../../include/orbil.h"
#include "../../include/orbvi_loop.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orb_lm_policy.h"
#include "orb_math.h"
#include "orbi_graph_device.h"
#include "orbvi_stages.h"

#pragma clang fp contract(off)

static_assert(sizeof(orbil_chain_options) == 40, "orbil.h fixes this layout");
static_assert(CS_MAX_STATES == ORBIL_MAX_STATES && CS_BAND == ORBIL_SOLVE_WORK(1), "orbil.h states the cap and the band of a state");

namespace {

constexpr int CS_T = 256;                                         // the staged solve's workgroup
// the solve's LDS, in doubles from one base: the tile, y (then x), the reciprocals, computeScale's terms, then the fixed flags as ints
enum { L_T = 0, L_Y = L_T + CS_TILE, L_R = L_Y + CS_N, L_V = L_R + CS_N, L_FIX = L_V + CS_N, L_WORDS = L_FIX + CS_N / 2 };

__global__ __launch_bounds__(CS_T) void k_il_chain_solve(int n, const uint8_t *__restrict__ fixed, const orbi_edge *__restrict__ edges, int n_edges, int cap,
                                                         const double *__restrict__ H_diag, const double *__restrict__ H_off, const double *__restrict__ b,
                                                         const double *__restrict__ lambda, double *band, double *__restrict__ dx, double *__restrict__ out,
                                                         int32_t *__restrict__ result)
{
    __shared__ double s_l[L_WORDS];
    __shared__ int s_cnt[8];
    int *s_fix = (int *)(s_l + L_FIX);
    chain_solve_assemble<CS_T>(threadIdx.x, n, fixed, edges, n_edges, cap, H_diag, H_off, band, s_fix, s_cnt);
    if (threadIdx.x >= 64) return;                // one wave from here on: no workgroup barrier below
    const int lane = threadIdx.x;
    const double h_max = chain_solve_largest(15 * n, band, s_fix, lane);
    const bool refused = chain_solve_wave(n, b, *lambda, dx, out, band, s_l + L_T, s_l + L_Y, s_l + L_R, s_l + L_V, s_fix, lane);
    if (lane == 0) out[1] = h_max;
    if (lane < 8) result[lane] = lane == ORBI_R_DONE ? !refused : lane == ORBI_R_REFUSED ? refused : lane == ORBI_R_RANGE ? s_cnt[ORBI_R_RANGE] : 0;
}

// ---- the loop --------------------------------------------------------------------------------------------------------------------------
constexpr int IL_T = 512, IL_WAVES = IL_T / 64;
constexpr int IL_N = ORBIL_MAX_STATES, IL_E = IL_N - 1;
constexpr int IL_STEPS_CAP = ORBVI_LOOP_MAX_ITERATIONS * (1 + ORBVI_LOOP_MAX_TRIALS) + 1;
enum { K_LIN = 0, K_TRIAL = 1, K_DONE = 3 };                      // the first two are the stages' modes
// the policy's state in LDS, written by thread 0 only
enum { Q_KIND, Q_IT, Q_QMAX, Q_ITS, Q_ROWS, Q_POP, Q_PUSH, Q_SOLVE, Q_INIT, Q_REFUSED, Q_ACCEPTED, Q_REJECTED, Q_N_REFUSED, Q_STEP, Q_MAX_STEPS, Q_WORDS };
enum { P_LAM, P_NI, P_CUR, P_RHO, PL_WORDS };
// the caller's scratch, in doubles
enum { F_WORK = 0, F_ERR = F_WORK + ORBI_EDGE_WORK * IL_E, F_CHI2 = F_ERR + 9 * IL_E, F_TOTAL = F_CHI2 + 3 * IL_E, F_HDIAG = F_TOTAL + 2,
       F_HOFF = F_HDIAG + 225 * IL_N, F_B = F_HOFF + 225 * IL_E, F_SAVED = F_B + 15 * IL_N, F_CHI2_PRIOR = F_SAVED + 21 * IL_N,
       F_BAND = F_CHI2_PRIOR + 3 * ORBVI_LOOP_MAX_PRIOR_JOBS, F_WORDS = F_BAND + CS_BAND * IL_N };
static_assert(F_WORDS <= ORBIL_LOOP_WORK, "orbil.h states the scratch");
static_assert(LM_TRACE_ROW == ORBVI_LOOP_TRACE && ORBIL_SUMMARY >= 7, "orbil.h states the summary and a row of the trace, which lm_trace_row writes");
static_assert(L_WORDS <= IL_WAVES * D_WORDS, "the solve's LDS lies over the edges' slices");
static_assert(21 * IL_N + IL_N <= IL_T, "a thread per word of the push");

struct ChainArgs {
    LinArgs fac;
    int max_steps;
    orbil_chain_options o;
    int32_t *iter;
    double *work, *trace, *summary;
    int cap_trace;
    int32_t *result;
};

// entry k of a state's 21 doubles (Rwb, twb, v, bg, ba), as push and pop walk them
__device__ __forceinline__ double *chain_vertex_word(const orbi_graph &g, int s, int k)
{
    return k < 9 ? g.Rwb + 9 * (size_t)s + k : k < 12 ? g.twb + 3 * (size_t)s + k - 9 : k < 15 ? g.v + 3 * (size_t)s + k - 12 : k < 18 ? g.bg + 3 * (size_t)s + k - 15
                                                                                                                                   : g.ba + 3 * (size_t)s + k - 18;
}

// The kernel's arguments, read afresh from the kernarg segment (the one argument sits at its start), and the thread's index behind an
// opaque copy, as in k_vi_pose_loop and for its reasons: the compiler otherwise loads every argument once ahead of the loop, moves every
// lane predicate and LDS address of every stage there too, and keeps them in more registers than there are.  Behind these a phase loads
// what it uses where it uses it, and a stage finds the registers its staged kernel has
__device__ __forceinline__ const ChainArgs &chain_args()
{
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const ChainArgs *)p;
}
__device__ __forceinline__ int chain_tid()
{
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

__global__ __launch_bounds__(IL_T) void k_il_chain_loop(const ChainArgs)     // the one argument is read through chain_args()
{
    __shared__ __attribute__((aligned(16))) double s_d[IL_WAVES][D_WORDS];   // the edges' wave slices; the solve's LDS lies over them
    __shared__ float s_f[IL_WAVES][X_WORDS];
    __shared__ int s_scnt[8];                                      // the solve's counters
    __shared__ int s_fcnt[8];                                      // the tail wave's counters
    __shared__ double s_dx[15 * IL_N];
    __shared__ double s_out[3];
    __shared__ double s_p[PL_WORDS];                               // the policy
    __shared__ int s_q[Q_WORDS];
    __shared__ int s_it[IL_N];                                     // the pushed update counters
    // Nothing lives across a stage: the step's kind, the counts and the flags are in LDS and are read where they are used
    {
        const int t = threadIdx.x;
        const ChainArgs &a = chain_args();
        if (t < Q_WORDS) s_q[t] = t == Q_MAX_STEPS ? a.max_steps : 0;   // Q_KIND = K_LIN, iteration 0
        if (t < PL_WORDS) s_p[t] = 0.0;
        if (t < 8) s_scnt[t] = 0, s_fcnt[t] = 0;
        if (t < ORBIL_SUMMARY) a.summary[t] = 0.0;
        __syncthreads();
    }
    // bounded twice: by the constant, and by Q_MAX_STEPS, which the policy counts the steps against
    for (int step = 0; step < IL_STEPS_CAP; ++step) {
        if (uniform(s_q[Q_KIND]) == K_DONE) break;                 // uniform
        {                                                          // a wave per edge in its own slice, the edges in passes over the waves
            const LinArgs &f = chain_args().fac;
            const int t = chain_tid(), lane = t & 63, wave = uniform(t >> 6), kind = uniform(s_q[Q_KIND]);
            for (int e = wave; e < f.n_edges; e += IL_WAVES) fac_edge_wave(f, kind, e, s_d[wave], s_f[wave], lane);
        }
        __syncthreads();
        {                                                          // a wave per state, and one for the totals
            const LinArgs &f = chain_args().fac;
            const int t = chain_tid(), lane = t & 63, wave = uniform(t >> 6), kind = uniform(s_q[Q_KIND]), n = f.g.n_states;
            for (int x = wave; x <= n; x += IL_WAVES) {
                if (x == n) fac_gather_tail(f, s_fcnt, lane);
                else if (kind == K_LIN) fac_gather_state(f, x, lane);
            }
        }
        __syncthreads();
        if (chain_tid() == 0) {                                    // ---- the decision: orb_lm_policy.h's arithmetic, in inertial_loop.optimize's shape
            const ChainArgs &a = chain_args();
            const int kind = s_q[Q_KIND], qmax = s_q[Q_QMAX];
            int it = s_q[Q_IT];
            bool ends = false;
            s_q[Q_POP] = s_q[Q_PUSH] = s_q[Q_SOLVE] = s_q[Q_INIT] = 0;
            if (kind == K_LIN) {                                   // computeActiveErrors, activeRobustChi2, buildSystem
                LmPolicy p = {};                                   // lambda and nu stay where they are, in LDS
                lm_policy_iteration(p, a.fac.total[1]);
                s_p[P_CUR] = p.current, s_p[P_RHO] = p.rho, s_q[Q_QMAX] = p.qmax;
                if (it == 0) s_q[Q_INIT] = 1, s_p[P_NI] = 2.0;     // computeLambdaInit: the value is taken behind the assembly
                s_q[Q_PUSH] = 1, s_q[Q_SOLVE] = 1, s_q[Q_KIND] = K_TRIAL;
            } else {
                LmPolicy p = {s_p[P_LAM], s_p[P_NI], s_p[P_CUR], s_p[P_RHO], qmax};
                const double lam = p.lam, current = p.current;
                const bool ok = !s_q[Q_REFUSED];
                const double ti = a.fac.total[1], scale_pose = s_out[0];
                const LmTrial tr = lm_policy_trial(p, ok, ti, 0.0, scale_pose, 0.0);   // no visual total, no points' side of computeScale
                const int row = s_q[Q_ROWS];
                if (row < a.cap_trace) lm_trace_row(a.trace + (size_t)ORBVI_LOOP_TRACE * row, it, qmax, lam, current, tr, ok, ti, 0.0, scale_pose, 0.0);
                s_q[Q_ROWS] = row + 1;
                if (tr.accepted) ++s_q[Q_ACCEPTED];
                else s_q[Q_POP] = 1, ++s_q[Q_REJECTED];            // pop: the vertices and their update counters
                s_p[P_LAM] = p.lam, s_p[P_NI] = p.ni, s_p[P_CUR] = p.current, s_p[P_RHO] = p.rho, s_q[Q_QMAX] = p.qmax;
                if (lm_policy_again(p, tr, a.o.max_trials)) s_q[Q_SOLVE] = 1;         // the next trial from the popped estimate: the push still holds
                else {
                    ++s_q[Q_ITS], ++it;
                    if (lm_policy_terminate(p, a.o.max_trials) || it >= a.o.iterations) ends = true;
                    else s_q[Q_IT] = it, s_q[Q_KIND] = K_LIN;
                }
            }
            if (ends) s_q[Q_KIND] = K_DONE;
            if (++s_q[Q_STEP] >= s_q[Q_MAX_STEPS]) s_q[Q_KIND] = K_DONE;   // never met: the policy ends within the host's count
        }
        __syncthreads();
        if (uniform(s_q[Q_POP])) {
            const ChainArgs &a = chain_args();
            const int t = chain_tid(), n = a.fac.g.n_states;
            if (t < 21 * n) *chain_vertex_word(a.fac.g, t / 21, t % 21) = a.work[F_SAVED + t];
            else if (t < 22 * n) a.iter[t - 21 * n] = s_it[t - 21 * n];
        }
        __syncthreads();
        if (!uniform(s_q[Q_SOLVE])) continue;                      // uniform
        const ChainArgs &a = chain_args();
        const LinArgs &f = a.fac;
        const int t = chain_tid(), lane = t & 63, n = f.g.n_states;
        double *s_l = &s_d[0][0];                                  // the solve's LDS lies over the edges' slices
        int *s_fix = (int *)(s_l + L_FIX);
        if (uniform(s_q[Q_PUSH])) {
            if (t < 21 * n) a.work[F_SAVED + t] = *chain_vertex_word(f.g, t / 21, t % 21);
            else if (t < 22 * n) s_it[t - 21 * n] = a.iter[t - 21 * n];
        }
        chain_solve_assemble<IL_T>(t, n, f.g.fixed, f.edges, f.n_edges, f.cap, f.H_diag, f.H_off, a.work + F_BAND, s_fix, s_scnt);
        if (uniform(t >> 6) == 0) {
            const double largest = chain_solve_largest(15 * n, a.work + F_BAND, s_fix, lane);
            if (lane == 0 && s_q[Q_INIT]) {                        // setUserLambdaInit, computeLambdaInit, or the 0 g2o cannot reach
                const double user = a.o.lambda_init;
                s_p[P_LAM] = user > 0 ? user : user < 0 ? 0.0 : a.o.tau * largest;
            }
            wave_order();
            const bool refused = chain_solve_wave(n, f.b, s_p[P_LAM], s_dx, s_out, a.work + F_BAND, s_l + L_T, s_l + L_Y, s_l + L_R, s_l + L_V, s_fix, lane);
            if (lane == 0) {
                s_q[Q_REFUSED] = refused;
                if (refused) ++s_q[Q_N_REFUSED];
            }
        }
        __syncthreads();
        if (t < n) fac_oplus_state(f.g, s_dx, a.iter, t);
        __syncthreads();
    }
    __syncthreads();
    const ChainArgs &a = chain_args();
    const int t = threadIdx.x;
    if (t == 0) {
        double *sm = a.summary;
        sm[0] = s_q[Q_ITS], sm[1] = s_q[Q_ROWS], sm[2] = s_q[Q_ACCEPTED], sm[3] = s_q[Q_N_REFUSED], sm[4] = s_p[P_LAM], sm[5] = s_q[Q_ROWS];
        sm[6] = s_q[Q_ROWS] > a.cap_trace ? s_q[Q_ROWS] - a.cap_trace : 0;
    }
    if (t < 8) {
        int v = 0;
        if (t == ORBI_R_DONE) v = s_q[Q_ACCEPTED];
        else if (t == ORBI_R_RANGE) v = s_fcnt[ORBI_R_RANGE] + s_scnt[ORBI_R_RANGE];
        else if (t == ORBI_R_DUPLICATE) v = s_q[Q_REJECTED];
        else if (t == ORBI_R_REFUSED) v = s_q[Q_N_REFUSED];
        else if (t == ORBI_R_PRIOR_RANGE) v = s_fcnt[ORBI_R_PRIOR_RANGE];
        else if (t == ORBVI_R_EDGE_REFUSED) v = s_fcnt[ORBI_R_REFUSED];
        a.result[t] = v;
    }
}

} // namespace

extern "C" int orbil_chain_solve_device(int n_states, const uint8_t *d_fixed, const orbi_edge *d_edges, int n_edges, int cap, const double *d_H_diag,
                                        const double *d_H_off, const double *d_b, const double *d_lambda, double *d_work, double *d_dx, double *d_out,
                                        int32_t *d_result, void *stream)
{
    if (n_states < 1 || !d_fixed || n_edges < 0 || cap < 1 || !d_H_diag || !d_b || !d_lambda || !d_work || !d_dx || !d_out || !d_result)
        return orbx_set_error(ORBX_E_ARG, "null array, scratch or result, n_states or cap < 1, or a negative edge count");
    if (n_edges > 0 && (!d_edges || !d_H_off)) return orbx_set_error(ORBX_E_ARG, "edges without their list or d_H_off");
    if (n_states < 2 || n_states > ORBIL_MAX_STATES) return orbx_set_error(ORBX_E_UNSUPPORTED, "a chain has 2 .. ORBIL_MAX_STATES (20) states");
    if (n_edges > ORBI_MAX_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBI_MAX_JOBS (4096) edges in one call");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_il_chain_solve, dim3(1), dim3(CS_T), 0, s, n_states, d_fixed, d_edges, n_edges, cap, d_H_diag, d_H_off, d_b, d_lambda, d_work, d_dx, d_out,
                       d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbil_chain_optimize_device(orbi_graph graph, int32_t *d_iter, const orbi_record *d_bank, int cap, const orbi_edge *d_edges, int n_edges,
                                           const double *d_info, const double *d_walk_info, const orbi_prior *d_priors, int n_priors,
                                           const orbi_prior_job *d_prior_jobs, int n_prior_jobs, orbil_chain_options options, double *d_work,
                                           double *d_trace, int cap_trace, double *d_summary, int32_t *d_result, void *stream)
{
    const orbil_chain_options &o = options;
    if (!graph.Rwb || !graph.twb || !graph.v || !graph.bg || !graph.ba || !graph.fixed || graph.n_states < 1 || !d_result)
        return orbx_set_error(ORBX_E_ARG, "null graph array or result, or a state count < 1");
    if (!d_iter || !d_bank || cap < 1 || n_edges < 0 || !d_work || !d_summary || cap_trace < 0 || (cap_trace > 0 && !d_trace))
        return orbx_set_error(ORBX_E_ARG, "null d_iter, bank, scratch, summary or trace, cap < 1, or a negative count");
    if (n_edges > 0 && (!d_edges || !d_info || !d_walk_info)) return orbx_set_error(ORBX_E_ARG, "edges without their list or their information");
    if (n_prior_jobs < 0 || n_priors < 0 || (n_prior_jobs > 0 && (!d_prior_jobs || !d_priors)))
        return orbx_set_error(ORBX_E_ARG, "prior jobs without their list or the priors, or a negative count");
    if (o.iterations < 1 || o.max_trials < 1) return orbx_set_error(ORBX_E_ARG, "iterations or max_trials < 1");
    if (!(o.tau == o.tau) || !(o.huber_delta == o.huber_delta) || !(o.gravity == o.gravity) || !(o.lambda_init == o.lambda_init))
        return orbx_set_error(ORBX_E_ARG, "tau, huber_delta, gravity or lambda_init is not a number");
    if (graph.n_states < 2 || graph.n_states > ORBIL_MAX_STATES) return orbx_set_error(ORBX_E_UNSUPPORTED, "a chain has 2 .. ORBIL_MAX_STATES (20) states");
    if (n_edges > graph.n_states - 1) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than n_states - 1 inertial edges");
    if (n_prior_jobs > ORBVI_LOOP_MAX_PRIOR_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVI_LOOP_MAX_PRIOR_JOBS (64) prior jobs");
    if (o.iterations > ORBVI_LOOP_MAX_ITERATIONS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVI_LOOP_MAX_ITERATIONS (100) iterations");
    if (o.max_trials > ORBVI_LOOP_MAX_TRIALS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVI_LOOP_MAX_TRIALS (10) trials in an iteration");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    ChainArgs a = {};
    LinArgs &f = a.fac;
    f.g = graph, f.bank = d_bank, f.cap = cap, f.gravity = o.gravity, f.edges = d_edges, f.n_edges = n_edges, f.info = d_info, f.walk_info = d_walk_info;
    f.priors = d_priors, f.n_priors = n_priors, f.pjobs = d_prior_jobs, f.n_pjobs = n_prior_jobs, f.delta = o.huber_delta;
    f.work = d_work + F_WORK, f.err = d_work + F_ERR, f.chi2 = d_work + F_CHI2, f.chi2_prior = d_work + F_CHI2_PRIOR, f.total = d_work + F_TOTAL;
    f.H_diag = d_work + F_HDIAG, f.H_off = d_work + F_HOFF, f.b = d_work + F_B, f.J = nullptr, f.flt = nullptr, f.result = d_result;
    a.max_steps = o.iterations * (1 + o.max_trials) + 1, a.o = o, a.iter = d_iter, a.work = d_work, a.trace = d_trace, a.summary = d_summary;
    a.cap_trace = cap_trace, a.result = d_result;
    hipLaunchKernelGGL(k_il_chain_loop, dim3(1), dim3(IL_T), 0, s, a);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
