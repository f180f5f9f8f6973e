// poseFullOptimize / poseInertialOptimize whole on the device (include/orbvi_loop.h):
//   orbvi_pose_optimize_device   the rounds, g2o's Levenberg-Marquardt policy, push / pop and the classification   Optimize.cpp:547-764
//
// ONE WORKGROUP of 512 threads runs the whole optimisation in one launch.  Every stage of an iteration is a device function of
// csrc/orbvi_stages.h, the one the staged call's kernel runs (orbi_linearize_device, orbvi_linearize_device, orbvi_solve_device,
// orbi_graph_oplus_device): no formula is restated here, so a linearisation, a solve and an update inside the loop give the bytes of the
// staged calls on the same input.  Nor is the trial policy's arithmetic: it is orb_lm_policy.h's, run by one lane.  What is here is the
// step machine around it (tests/inertial_loop.py's pose_full / pose_inertial and the shape of its optimize), the vertices' push and pop
// with their update counters, the reset of the frame's pose ahead of a round and the trace.
//
// Shape.  The loop is a sequence of STEPS, each of one kind: LIN evaluates both linearisations at the estimate (mode 0), TRIAL their
// errors at a trial point (mode 1), CLASSIFY the inliers behind a round (mode 2).  Behind the evaluation ONE LANE (thread 0) takes the
// policy's decision and publishes it through LDS; behind a barrier every thread reads it and the workgroup pops, pushes, solves and
// updates as it says.  So each stage is inlined once, every barrier is in control flow that is uniform across the workgroup, and the
// step count is bounded by what the host computed from the checked options: sum over the rounds of iterations * (1 + max_trials) + 1.
// There is no second workgroup, no spin-wait and no floating-point atomic.  Global memory that the workgroup wrote (the graph, the
// blocks in the caller's scratch) is read back behind a barrier only.
//
// Why 512 threads.  Inside a loop the compiler moves the stages' constants (the polynomials of sin, cos and atan2: some fifty register
// pairs) ahead of the loop and keeps them live across every stage.  vi_linearize_group needs 126 vector registers for itself, all but two
// of the 128 a 1024-thread workgroup has, so at 1024 threads the hoisted values are spilled to scratch (276 to 1092 bytes in the variants
// tried; a step function that is not inlined avoids the loop and pays 188 bytes of callee-saved registers instead).  Eight waves have
// 256 registers each: everything fits and scratch use is 0.  The visual stage keeps its order all the same: vi_linearize_group<2> gives
// each thread the work of the two threads t and t + 512 of the 1024 the header's order is written for, one behind the other, and files
// each one's sums under its own wave.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include <string>

#include "../../include/orbvi_loop.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orb_lm_policy.h"
#include "orb_math.h"
#include "orbi_graph_device.h"
#include "orbvi_stages.h"

#pragma clang fp contract(off)

static_assert(sizeof(orbvi_loop_options) == 96, "orbvi_loop.h fixes this layout");

namespace {

enum { K_LIN = 0, K_TRIAL = 1, K_CLASSIFY = 2, K_DONE = 3 };   // the first three are the stages' modes
// the policy's state in LDS, written by thread 0 only
enum { Q_KIND, Q_ROUND, Q_IT, Q_QMAX, Q_ITS, Q_ROWS, Q_POP, Q_PUSH, Q_SOLVE, Q_INIT, Q_RESET, Q_REFUSED, Q_TRIALS, Q_ACCEPTED, Q_N_REFUSED,
       Q_START_IT, Q_VST, Q_VISUAL, Q_STEP, Q_MAX_STEPS, Q_SAVED_IT, Q_ALL_ACCEPTED = Q_SAVED_IT + 2, Q_ALL_REJECTED, Q_ALL_REFUSED, Q_WORDS };
enum { P_LAM, P_NI, P_CUR, P_RHO, PL_WORDS };
// the fixed part of the caller's scratch, in doubles, behind the visual edges' rows
enum { F_WORK = 0, F_ERR = F_WORK + ORBI_EDGE_WORK, F_CHI2 = F_ERR + 9, F_TOTAL = F_CHI2 + 3, F_VTOTAL = F_TOTAL + 2, F_HDIAG = F_VTOTAL + 2,
       F_HOFF = F_HDIAG + 450, F_B = F_HOFF + 225, F_START = F_B + 30, F_SAVED = F_START + 12, F_CHI2_PRIOR = F_SAVED + 42,
       F_WORDS = F_CHI2_PRIOR + 3 * ORBVI_LOOP_MAX_PRIOR_JOBS };
static_assert(F_WORDS <= ORBVI_LOOP_FIXED_WORK, "orbvi_loop.h states the fixed part of the scratch");
static_assert(ORBVI_LOOP_EDGE_WORK == ORBVI_EDGE_WORK + 2, "an edge's row of orbvi_linearize_device and its error");
enum { SUM_ROUND = 6, SUM_TRIALS = 24, SUM_OVERFLOW = 25 };
static_assert(SUM_OVERFLOW < ORBVI_LOOP_SUMMARY && LM_TRACE_ROW == ORBVI_LOOP_TRACE, "orbvi_loop.h states the summary and a row of the trace, which lm_trace_row writes");
constexpr int LOOP_N = 2;                                       // key frame, frame
constexpr int LOOP_VT = 2, LOOP_T = VI_T / LOOP_VT;             // the threads of the workgroup, each two of the visual stage's 1024
constexpr int LOOP_STEPS_CAP = ORBVI_LOOP_MAX_ROUNDS * (ORBVI_LOOP_MAX_ITERATIONS * (1 + ORBVI_LOOP_MAX_TRIALS) + 1);

struct LoopArgs {
    LinArgs fac;
    ViArgs vi;
    int visual, max_steps;
    orbvi_loop_options o;
    int32_t *iter;
    double *fixed_work, *trace, *summary;
    int cap_trace;
    int32_t *result;
};

// entry k of a state's 21 doubles (Rwb, twb, v, bg, ba), as push and pop walk them
__device__ __forceinline__ double *vertex_word(const orbi_graph &g, int s, int k)
{
    return k < 9 ? g.Rwb + 9 * (size_t)s + k : k < 12 ? g.twb + 3 * (size_t)s + k - 9 : k < 15 ? g.v + 3 * (size_t)s + k - 12 : k < 18 ? g.bg + 3 * (size_t)s + k - 15
                                                                                                                                   : g.ba + 3 * (size_t)s + k - 18;
}

// The kernel's arguments, read afresh from the kernarg segment (the one argument sits at its start): about 700 bytes, which the compiler
// otherwise loads once ahead of the loop and keeps in several times the scalar registers there are.  Behind the opaque copy of the
// segment's address a phase loads what it uses where it uses it; the loads stay scalar (constant address space)
__device__ __forceinline__ const LoopArgs &fresh_args()
{
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const LoopArgs *)p;
}

// The thread's index behind an opaque copy.  Everything a stage derives from it -- a lane's predicates, its LDS addresses -- is the same in
// every step, and the compiler moves all of it ahead of the loop and keeps it there (hundreds of lane masks); a stage that starts from
// this copy computes them where the staged kernel does
__device__ __forceinline__ int fresh_tid()
{
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

__global__ __launch_bounds__(LOOP_T) void k_vi_pose_loop(const LoopArgs)     // the one argument is read through fresh_args()
{
    __shared__ __attribute__((aligned(16))) double s_d[D_WORDS];   // the inertial edge's wave slices
    __shared__ float s_f[X_WORDS];
    __shared__ double s_part[VI_WAVES][VI_SUMS];                   // the visual group
    __shared__ double s_pose[P_WORDS];
    __shared__ int s_vcnt[8];
    __shared__ int s_i[I_WORDS];
    __shared__ double s_A[SV_N * SV_LD];                           // the solve
    __shared__ double s_v[SV_N];
    __shared__ int s_fix[SV_N];
    __shared__ int s_scnt[8];
    __shared__ int s_fcnt[8];                                      // the inertial tail wave's counters
    __shared__ double s_dx[15 * LOOP_N];
    __shared__ double s_out[3];
    __shared__ double s_p[PL_WORDS];                               // the policy
    __shared__ int s_q[Q_WORDS];
    // Nothing lives across a stage: the step's kind, the counts and the flags are in LDS and are read where they are used, so that
    // a stage finds the registers its staged kernel has
    {
        const int t = threadIdx.x;
        const LoopArgs &a = fresh_args();
        const int visual = a.visual;
        if (t < Q_WORDS) s_q[t] = (t == Q_RESET || t == Q_VISUAL) ? visual : t == Q_MAX_STEPS ? a.max_steps : 0;   // Q_KIND = K_LIN, round 0, iteration 0
        if (t < PL_WORDS) s_p[t] = 0.0;
        if (t < 8) s_vcnt[t] = 0, s_scnt[t] = 0, s_fcnt[t] = 0;
        if (t < ORBVI_LOOP_SUMMARY) a.summary[t] = 0.0;
        __syncthreads();
        // the pose side of the visual group's state at entry: what every round starts from
        const int vst = visual ? uniform(a.vi.group_state[0]) : -1;
        if (vst >= 0 && vst < LOOP_N) {
            if (t < 12) a.fixed_work[F_START + t] = *vertex_word(a.fac.g, vst, t);
            else if (t == 12) s_q[Q_START_IT] = a.iter[vst];
            else if (t == 13) s_q[Q_VST] = 1 + vst;
        }
        __syncthreads();
    }
    // bounded twice: by the constant, and by Q_MAX_STEPS, which the policy counts the steps against
    for (int step = 0; step < LOOP_STEPS_CAP; ++step) {
        if (uniform(s_q[Q_KIND]) == K_DONE) break;                 // uniform
        if (uniform(s_q[Q_RESET]) && uniform(s_q[Q_VST])) {        // Optimize.cpp:717 setEstimate(initialPose), with the update counter
            const LoopArgs &a = fresh_args();
            const int t = fresh_tid();
            const int vst = uniform(s_q[Q_VST]) - 1;
            if (t < 12) *vertex_word(a.fac.g, vst, t) = a.fixed_work[F_START + t];
            else if (t == 12) a.iter[vst] = s_q[Q_START_IT];
        }
        __syncthreads();
        if (uniform(s_q[Q_KIND]) != K_CLASSIFY) {                  // the inertial edge and the priors: a wave each, as in the staged call
            const int kind = uniform(s_q[Q_KIND]);
            {
                const LinArgs &f = fresh_args().fac;
                const int t = fresh_tid(), lane = t & 63, wave = uniform(t >> 6);
                if (wave == 0 && f.n_edges > 0) fac_edge_wave(f, kind, 0, s_d, s_f, lane);
            }
            __syncthreads();
            {
                const LinArgs &f = fresh_args().fac;
                const int t = fresh_tid(), lane = t & 63, wave = uniform(t >> 6);
                if (wave < LOOP_N) {
                    if (kind == K_LIN) fac_gather_state(f, wave, lane);
                } else if (wave == LOOP_N) fac_gather_tail(f, s_fcnt, lane);
            }
            __syncthreads();
        }
        if (uniform(s_q[Q_VISUAL])) {                              // the visual group adds to the blocks the gather wrote
            vi_linearize_group<LOOP_VT>(fresh_args().vi, uniform(s_q[Q_KIND]), 0, fresh_tid(), s_part, s_pose, s_vcnt, s_i);
            __syncthreads();
        }
        if (fresh_tid() == 0) {                                    // ---- the decision: orb_lm_policy.h's arithmetic, in inertial_loop.optimize's shape
            const LoopArgs &a = fresh_args();
            const int kind = s_q[Q_KIND], visual = s_q[Q_VISUAL];
            const int round = s_q[Q_ROUND];
            int it = s_q[Q_IT], qmax = s_q[Q_QMAX];
            bool round_ends = false;
            s_q[Q_POP] = s_q[Q_PUSH] = s_q[Q_SOLVE] = s_q[Q_INIT] = s_q[Q_RESET] = 0;
            if (kind == K_LIN) {                                   // computeActiveErrors, activeRobustChi2, buildSystem
                const double ti = a.fac.total[1];
                LmPolicy p = {};                                   // lambda and nu stay where they are, in LDS
                lm_policy_iteration(p, visual ? ti + a.vi.total[1] : ti);
                s_p[P_CUR] = p.current, s_p[P_RHO] = p.rho, s_q[Q_QMAX] = p.qmax;
                if (it == 0) s_q[Q_INIT] = 1, s_p[P_NI] = 2.0;     // computeLambdaInit: the value is taken behind the assembly
                s_q[Q_PUSH] = 1, s_q[Q_SOLVE] = 1, s_q[Q_KIND] = K_TRIAL;
            } else if (kind == K_TRIAL) {
                LmPolicy p = {s_p[P_LAM], s_p[P_NI], s_p[P_CUR], s_p[P_RHO], qmax};
                const double lam = p.lam, current = p.current;
                const bool ok = !s_q[Q_REFUSED];
                const double ti = a.fac.total[1], tv = visual ? a.vi.total[1] : 0.0, scale_pose = s_out[0];
                const LmTrial t = lm_policy_trial(p, ok, ti, tv, scale_pose, 0.0);   // computeScale has no points' side here
                const int row = s_q[Q_ROWS];
                if (row < a.cap_trace) lm_trace_row(a.trace + (size_t)ORBVI_LOOP_TRACE * row, it, qmax, lam, current, t, ok, ti, tv, scale_pose, 0.0);
                s_q[Q_ROWS] = row + 1, ++s_q[Q_TRIALS];
                if (t.accepted) ++s_q[Q_ACCEPTED], ++s_q[Q_ALL_ACCEPTED];
                else s_q[Q_POP] = 1, ++s_q[Q_ALL_REJECTED];        // pop: the vertices and their update counters
                s_p[P_LAM] = p.lam, s_p[P_NI] = p.ni, s_p[P_CUR] = p.current, s_p[P_RHO] = p.rho, s_q[Q_QMAX] = p.qmax;
                if (lm_policy_again(p, t, a.o.max_trials)) s_q[Q_SOLVE] = 1;          // the next trial from the popped estimate: the push still holds
                else {
                    ++s_q[Q_ITS], ++it;
                    if (lm_policy_terminate(p, a.o.max_trials) || it >= a.o.iterations[round]) round_ends = true;
                    else s_q[Q_IT] = it, s_q[Q_KIND] = K_LIN;
                }
            }
            if (round_ends) {
                double *sm = a.summary + SUM_ROUND * round;
                sm[0] = s_q[Q_ITS], sm[1] = s_q[Q_TRIALS], sm[2] = s_q[Q_ACCEPTED], sm[3] = s_q[Q_N_REFUSED], sm[4] = s_p[P_LAM];
                if (visual) s_q[Q_KIND] = K_CLASSIFY;
            }
            if (kind == K_CLASSIFY) a.summary[SUM_ROUND * round + 5] = a.vi.n_inliers[0];
            if (kind == K_CLASSIFY || (round_ends && !visual)) {   // the next round, or the end
                if (round + 1 < a.o.rounds) {
                    s_q[Q_ROUND] = round + 1, s_q[Q_IT] = 0, s_q[Q_ITS] = 0, s_q[Q_TRIALS] = 0, s_q[Q_ACCEPTED] = 0, s_q[Q_N_REFUSED] = 0;
                    s_q[Q_RESET] = visual, s_q[Q_KIND] = K_LIN;
                } else s_q[Q_KIND] = K_DONE;
            }
            if (++s_q[Q_STEP] >= s_q[Q_MAX_STEPS]) s_q[Q_KIND] = K_DONE;   // never met: the policy ends within the host's count
        }
        __syncthreads();
        if (uniform(s_q[Q_POP])) {
            const LoopArgs &a = fresh_args();
            const int t = fresh_tid();
            if (t < 21 * LOOP_N) *vertex_word(a.fac.g, t / 21, t % 21) = a.fixed_work[F_SAVED + t];
            else if (t < 21 * LOOP_N + LOOP_N) a.iter[t - 21 * LOOP_N] = s_q[Q_SAVED_IT + t - 21 * LOOP_N];
        }
        __syncthreads();
        if (!uniform(s_q[Q_SOLVE])) continue;                      // uniform
        const LoopArgs &a = fresh_args();
        const int t = fresh_tid(), lane = t & 63;
        if (uniform(s_q[Q_PUSH])) {
            if (t < 21 * LOOP_N) a.fixed_work[F_SAVED + t] = *vertex_word(a.fac.g, t / 21, t % 21);
            else if (t < 21 * LOOP_N + LOOP_N) s_q[Q_SAVED_IT + t - 21 * LOOP_N] = a.iter[t - 21 * LOOP_N];
        }
        vi_solve_assemble<LOOP_T>(t, LOOP_N, a.fac.g.fixed, a.fac.edges, a.fac.n_edges, a.fac.cap, a.fac.H_diag, a.fac.H_off, s_A, s_fix, s_scnt);
        if (uniform(t >> 6) == 0) {
            const double largest = vi_solve_largest(15 * LOOP_N, s_A, s_fix, lane);
            if (lane == 0 && s_q[Q_INIT]) {                        // setUserLambdaInit, computeLambdaInit, or the 0 g2o cannot reach
                const double user = a.o.lambda_init[s_q[Q_ROUND]];
                s_p[P_LAM] = user > 0 ? user : user < 0 ? 0.0 : a.o.tau * largest;
            }
            wave_order();
            const bool refused = vi_solve_wave(15 * LOOP_N, a.fac.b, s_p[P_LAM], s_dx, s_out, s_A, s_v, s_fix, lane);
            if (lane == 0) {
                s_q[Q_REFUSED] = refused;
                if (refused) ++s_q[Q_N_REFUSED], ++s_q[Q_ALL_REFUSED];
            }
        }
        __syncthreads();
        if (t < LOOP_N) fac_oplus_state(a.fac.g, s_dx, a.iter, t);
        __syncthreads();
    }
    __syncthreads();
    const LoopArgs &a = fresh_args();
    const int t = threadIdx.x;
    if (t == 0) a.summary[SUM_TRIALS] = s_q[Q_ROWS], a.summary[SUM_OVERFLOW] = s_q[Q_ROWS] > a.cap_trace ? s_q[Q_ROWS] - a.cap_trace : 0;
    if (t < 8) {
        int v = 0;
        if (t == ORBI_R_DONE) v = s_q[Q_ALL_ACCEPTED];
        else if (t == ORBI_R_RANGE) v = s_fcnt[ORBI_R_RANGE] + s_vcnt[ORBI_R_RANGE] + s_scnt[ORBI_R_RANGE];
        else if (t == ORBI_R_DUPLICATE) v = s_q[Q_ALL_REJECTED];
        else if (t == ORBI_R_REFUSED) v = s_q[Q_ALL_REFUSED];
        else if (t == ORBVI_R_NONFINITE) v = s_vcnt[ORBVI_R_NONFINITE];
        else if (t == ORBI_R_PRIOR_RANGE) v = s_fcnt[ORBI_R_PRIOR_RANGE];
        else if (t == ORBVI_R_EDGE_REFUSED) v = s_fcnt[ORBI_R_REFUSED];
        a.result[t] = v;
    }
}

} // namespace

extern "C" int orbvi_pose_optimize_device(orbi_graph graph, int32_t *d_iter, const orbi_record *d_bank, int cap, const orbi_edge *d_edges, int n_edges,
                                          const double *d_info, const double *d_walk_info, const orbi_prior *d_priors, int n_priors,
                                          const orbi_prior_job *d_prior_jobs, int n_prior_jobs, orbi_calib calib, orbvi_camera camera, int cap_edges,
                                          const int32_t *d_group_state, const int32_t *d_edge_off, const double *d_points, const double *d_edge_z,
                                          const double *d_edge_inv_sigma2, uint8_t *d_active, orbvi_loop_options options, double *d_work,
                                          double *d_chi2, int32_t *d_n_inliers, double *d_trace, int cap_trace, double *d_summary, int32_t *d_result,
                                          void *stream)
{
    const orbvi_loop_options &o = options;
    if (!graph.Rwb || !graph.twb || !graph.v || !graph.bg || !graph.ba || !graph.fixed || graph.n_states < 0 || !d_result)
        return orbx_set_error(ORBX_E_ARG, "null graph array or result, or a negative state count");
    if (!d_iter || !d_bank || cap < 1 || !d_edges || n_edges < 0 || !d_info || !d_walk_info || !d_work || !d_summary || cap_trace < 0 || (cap_trace > 0 && !d_trace))
        return orbx_set_error(ORBX_E_ARG, "null d_iter, bank, edge, information, scratch, summary or trace, cap < 1, or a negative count");
    if (n_prior_jobs < 0 || n_priors < 0 || (n_prior_jobs > 0 && (!d_prior_jobs || !d_priors)))
        return orbx_set_error(ORBX_E_ARG, "prior jobs without their list or the priors, or a negative count");
    if (cap_edges < 0 || (cap_edges > 0 && (!d_group_state || !d_edge_off || !d_points || !d_edge_z || !d_edge_inv_sigma2 || !d_active || !d_chi2 || !d_n_inliers)))
        return orbx_set_error(ORBX_E_ARG, "visual edges without their group, arrays, d_active, d_chi2 or d_n_inliers, or a negative cap_edges");
    if (o.rounds < 1 || o.max_trials < 1) return orbx_set_error(ORBX_E_ARG, "rounds or max_trials < 1");
    if (!(o.tau == o.tau) || !(o.huber_delta == o.huber_delta) || !(o.chi2_threshold == o.chi2_threshold) || !(o.gravity == o.gravity))
        return orbx_set_error(ORBX_E_ARG, "tau, huber_delta, chi2_threshold or gravity is not a number");
    if (camera.camera_model != 0 && camera.camera_model != 1) return orbx_set_error(ORBX_E_ARG, "camera_model is 0 (Pinhole) or 1 (Kannala-Brandt)");
    if (o.rounds > ORBVI_LOOP_MAX_ROUNDS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVI_LOOP_MAX_ROUNDS (4) rounds");
    int max_steps = 0;
    for (int k = 0; k < o.rounds; ++k) {
        if (o.iterations[k] < 1 || !(o.lambda_init[k] == o.lambda_init[k])) return orbx_set_error(ORBX_E_ARG, "a round with iterations < 1 or a lambda_init that is not a number");
        if (o.iterations[k] > ORBVI_LOOP_MAX_ITERATIONS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVI_LOOP_MAX_ITERATIONS (100) iterations in a round");
    }
    if (o.max_trials > ORBVI_LOOP_MAX_TRIALS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVI_LOOP_MAX_TRIALS (10) trials in an iteration");
    for (int k = 0; k < o.rounds; ++k) max_steps += o.iterations[k] * (1 + o.max_trials) + 1;
    if (graph.n_states != LOOP_N) return orbx_set_error(ORBX_E_UNSUPPORTED, "the tracker's graph has exactly 2 states (key frame, frame)");
    if (n_edges > 1) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than one inertial edge");
    if (n_prior_jobs > ORBVI_LOOP_MAX_PRIOR_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVI_LOOP_MAX_PRIOR_JOBS (64) prior jobs");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    double *fw = d_work + (size_t)ORBVI_LOOP_EDGE_WORK * cap_edges;
    LoopArgs a = {};
    LinArgs &f = a.fac;
    f.g = graph, f.bank = d_bank, f.cap = cap, f.gravity = o.gravity, f.edges = d_edges, f.n_edges = n_edges, f.info = d_info, f.walk_info = d_walk_info;
    f.priors = d_priors, f.n_priors = n_priors, f.pjobs = d_prior_jobs, f.n_pjobs = n_prior_jobs, f.delta = 0.0;   // EdgeInertial carries no robust kernel here
    f.work = fw + F_WORK, f.err = fw + F_ERR, f.chi2 = fw + F_CHI2, f.chi2_prior = fw + F_CHI2_PRIOR, f.total = fw + F_TOTAL, f.H_diag = fw + F_HDIAG;
    f.H_off = fw + F_HOFF, f.b = fw + F_B, f.J = nullptr, f.flt = nullptr, f.result = d_result;
    ViArgs &v = a.vi;
    v.g = graph, v.cal = calib, v.cam = graph_camera(camera, o.huber_delta);
    v.n_groups = 1, v.cap_edges = cap_edges, v.group_state = d_group_state, v.edge_off = d_edge_off, v.points = d_points, v.z = d_edge_z, v.w = d_edge_inv_sigma2;
    v.active = d_active, v.threshold = o.chi2_threshold, v.work = d_work, v.err = d_work + (size_t)ORBVI_EDGE_WORK * cap_edges, v.chi2 = d_chi2;
    v.total = fw + F_VTOTAL, v.H = f.H_diag, v.b = f.b, v.n_inliers = d_n_inliers, v.result = d_result;
    a.visual = cap_edges > 0, a.max_steps = max_steps, a.o = o, a.iter = d_iter, a.fixed_work = fw, a.trace = d_trace, a.summary = d_summary;
    a.cap_trace = cap_trace, a.result = d_result;
    hipLaunchKernelGGL(k_vi_pose_loop, dim3(1), dim3(LOOP_T), 0, s, a);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
