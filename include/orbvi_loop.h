/*
 * orbvi_loop.h -- poseFullOptimize and poseInertialOptimize whole on the device (liborbx.so, gfx950).
 *
 * This header includes orbvi.h and is not included by it; the rules are orbvi.h's: a handle-less `*_device` entry point under the one
 * stream rule of orbx.h, which enqueues on exactly the `stream` it is given (NULL is stream 0 itself), allocates nothing, copies
 * nothing and never waits; there is no CPU path.
 *
 * ---- orbvi_pose_optimize_device: poseFullOptimize / poseInertialOptimize whole, in one launch ----
 *
 * The tracker's per-frame optimiser of the inertial phase (Optimize.cpp:547-764) as ONE KERNEL LAUNCH OF ONE WORKGROUP (512 threads) on the stream it
 * is given: the rounds, g2o's Levenberg-Marquardt policy, the vertices' push and pop and the inlier classification, with no
 * allocation, no copy, no wait and no read-back -- no scalar leaves the device.  The chain of a frame is
 *   orbi_graph_init_device -> orbi_edge_information_device -> orbvi_pose_optimize_device -> orbi_graph_recover_device
 *   (-> orbba_pose_drop_outliers_device on d_active)
 * What it shares with the staged calls: every stage.  The kernel runs the device functions of csrc/orbvi_stages.h that k_fac_edge,
 * k_fac_gather, k_fac_oplus, k_vi_linearize and k_vi_solve run, in their orders (the visual sums thread t over the edges t, t + 1024,
 * ..., the butterfly, sixteen wave results ascending; the inertial edge on one wave in its LDS slice; the Cholesky by one wave, columns
 * ascending; no floating-point atomic; no fused multiply-add), so one linearisation, solve and update inside the loop gives the bytes of
 * the staged calls on the same input.  What remains the caller's: the graph's initialisation, the edge's information (ONCE per
 * optimisation, before the call), the recovery, and what it does with d_active.
 *
 * Inputs.  An orbi_graph of EXACTLY 2 states (key frame, frame) with the caller's `fixed` flags, and d_iter[2], the update counters
 * orbi_graph_oplus_device keeps; the record bank and at most ONE orbi_edge with its d_info / d_walk_info; d_priors and d_prior_jobs (at
 * most ORBVI_LOOP_MAX_PRIOR_JOBS); the calibration and the camera; ONE visual group on the state d_group_state[0]: d_edge_off[2],
 * d_points, d_edge_z, d_edge_inv_sigma2 as orbvi_linearize_device takes them, and d_active[cap_edges], READ as the first round's levels
 * (0: level 1) and WRITTEN by every round's classification.  cap_edges == 0 is poseInertialOptimize: no visual group, its arrays may
 * be NULL, nothing is reset or classified.  d_work is the caller's scratch of cap_edges * ORBVI_LOOP_EDGE_WORK +
 * ORBVI_LOOP_FIXED_WORK doubles; nothing in it need be initialised and nothing in it is an output.  EdgeInertial carries no robust
 * kernel in these optimisers; huber_delta is the visual edges'.
 * Distrust, as in the staged calls: d_edge_off is clamped to [0, cap_edges] and made non-decreasing; a group whose state lies outside the
 * graph is dropped in every evaluation (its pose is then never reset); an inertial edge whose states or record are out of range, or
 * whose information was refused, takes no part; a prior job out of range is dropped; each is counted.
 *
 * What it does is tests/inertial_loop.py's pose_full / pose_inertial / optimize line by line.  Round k of options.rounds:
 *   - only the POSE side of the visual group's state goes back to its value at entry (Optimize.cpp:717): Rwb, twb and that state's d_iter;
 *     velocity and biases keep what the last round left;
 *   - optimize(iterations[k]): per iteration both linearisations (mode 0) and current = their robustified totals; at iteration 0 lambda =
 *     lambda_init[k] when that is > 0 (g2o's setUserLambdaInit), tau * the largest free diagonal entry of H before damping when it is 0
 *     (computeLambdaInit -- taken directly behind the assembly, so no solve is discarded), and EXACTLY 0 when it is < 0: G2O CANNOT REACH
 *     THAT VALUE; it exists so that the refusal path is reachable from the ABI, as forced_lambda_init is in tests/inertial_loop.py.  Then
 *     up to max_trials trials: push (Rwb, twb, v, bg, ba AND d_iter of both states), the damped solve, oplus, both error evaluations (mode
 *     1) at the trial point, temp = their totals, or DBL_MAX behind a refused solve; scale = computeScale + 1e-3; rho = (current - temp) /
 *     scale; accepted when rho > 0 and temp is finite: lambda *= max(1/3, min(1 - x*x*x, 2/3)) with x = 2*rho - 1 -- THE CUBE IS x*x*x,
 *     not pow: csrc/orb_lm_policy.h's lm_cube, and k_pose_optimize's (orbba.hip) in its own copy of the policy --, nu = 2; otherwise
 *     lambda *= nu, nu *= 2 and the pop, which restores d_iter as well;
 *     the iteration ends when rho >= 0 or the trials run out, the round when trials == max_trials, rho == 0 or lambda is not finite;
 *   - every edge is classified against chi2_threshold (mode 2), and d_active is the next round's level.
 * The policy's arithmetic is IEEE double in the expression order of inertial_loop.optimize, by ONE lane, published through LDS.
 *
 * Outputs.  The graph and d_iter updated in place; d_active and d_n_inliers[1] of the LAST round, in the layout
 * orbba_pose_drop_outliers_device takes; d_chi2[cap_edges] of every edge at the final estimate; d_trace[cap_trace][ORBVI_LOOP_TRACE],
 * one row per trial over all rounds: iteration, trial, lambda, current, temp, scale, rho, ok (the solve was not refused), the inertial
 * and the visual total at the trial, computeScale's pose part, its points part (0), accepted -- inertial_loop.FIELDS; trials past
 * cap_trace are counted and not written.  d_summary[ORBVI_LOOP_SUMMARY]: per round k at [6k ..) the iterations run, the trials, the
 * accepted trials, the refused solves, the last lambda and the inliers behind the round; [24] the trials of all rounds, [25] those
 * that found no row in the trace.  d_result (one workgroup writes it; no clear launch is needed): [ORBI_R_DONE] accepted trials,
 * [ORBI_R_RANGE] what the last evaluation dropped (the inertial edge, the visual group, a block of the solve), [2] rejected trials,
 * [ORBI_R_REFUSED] refused solves, [ORBVI_R_NONFINITE] as in orbvi_linearize_device at the last evaluation, [ORBI_R_PRIOR_RANGE] prior
 * jobs dropped, [ORBVI_R_EDGE_REFUSED] the inertial edge refused by its information.
 *
 * Safety of the shape.  A single workgroup of 512 threads; no inter-workgroup synchronisation, no spin-wait on memory; the one loop is
 * bounded by the sum over the rounds of iterations[k] * (1 + max_trials) + 1 steps, computed on the host from the checked options;
 * every barrier is in control flow uniform across the workgroup; each decision (accepted, terminate, refused) is taken by one lane,
 * published through LDS and read by all lanes behind a barrier before they branch; global memory the workgroup wrote is read back only
 * behind a barrier.
 * Argument checks first: ORBX_E_ARG (a null pointer, a negative count, rounds, max_trials or an iterations[k] < 1, a tau, huber_delta,
 * chi2_threshold, gravity or lambda_init[k] that is not a number, a camera_model outside {0, 1}); ORBX_E_UNSUPPORTED (a graph of other
 * than 2 states, more than one inertial edge, more than ORBVI_LOOP_MAX_PRIOR_JOBS prior jobs, rounds, iterations or max_trials above
 * ORBVI_LOOP_MAX_ROUNDS, ORBVI_LOOP_MAX_ITERATIONS, ORBVI_LOOP_MAX_TRIALS); then ORBX_E_NO_DEVICE.
 * Kernel resources (gfx950, VGPRs / scratch bytes / static LDS bytes; tests/test_vi_loop_resources.py reads them from the ISA):
 *   k_vi_pose_loop 256 / 0 / 41576 B.
 * The workgroup has 512 threads, whose eight waves have 256 VGPRs each: inside the loop the compiler keeps the stages' constants in
 * registers across every stage, which 128 do not hold beside the visual stage's 126 (csrc/orbvi_loop.hip).  The visual sums keep the
 * order of 1024 threads: a thread does the work of the threads t and t + 512 of those, one behind the other, each under its own wave.
 * Latency-bound like the staged calls; tools/vi_pose_loop_latency.py records what a whole optimisation takes.
 * The mapper's localInertialBundleAdjustment (up to 20 key frames, every pose fixed, no visual edge) is closed in the same shape by
 * orbil_chain_optimize_device (orbil.h, which includes orbvi.h as this header does): the inertial stages of csrc/orbvi_stages.h, the
 * policy of csrc/orb_lm_policy.h, and a solve along the band of the chain in place of the dense one.
 */
#ifndef ORBVI_LOOP_H
#define ORBVI_LOOP_H

#include "orbvi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBVI_LOOP_MAX_ROUNDS 4
#define ORBVI_LOOP_MAX_ITERATIONS 100  /* per round */
#define ORBVI_LOOP_MAX_TRIALS 10       /* per iteration: g2o's default _maxTrialsAfterFailure */
#define ORBVI_LOOP_MAX_PRIOR_JOBS 64
#define ORBVI_LOOP_EDGE_WORK 18        /* doubles of d_work per visual edge */
#define ORBVI_LOOP_FIXED_WORK 2048     /* doubles of d_work behind the edges' */
#define ORBVI_LOOP_TRACE 13            /* doubles of a row of d_trace */
#define ORBVI_LOOP_SUMMARY 32          /* doubles of d_summary */
#define ORBVI_R_EDGE_REFUSED 7         /* d_result of orbvi_pose_optimize_device: the inertial edge refused by its information */

typedef struct orbvi_loop_options {    /* by value */
    int32_t rounds;                    /* 1 .. 4: poseFullOptimize has 4, poseInertialOptimize 1 */
    int32_t iterations[4];             /* per round, >= 1: 10 in the reference */
    int32_t max_trials;                /* 1 .. 10 */
    int32_t pad[2];
    double lambda_init[4];             /* per round: > 0 setUserLambdaInit, 0 computeLambdaInit, < 0 exactly 0 (g2o cannot reach it) */
    double tau;                        /* 1e-5 in g2o */
    double huber_delta;                /* of the visual edges: (double)sqrtf(5.991) */
    double chi2_threshold;             /* 5.991 */
    float gravity, pad2;
} orbvi_loop_options;

/* The whole optimisation of a tracked frame's inertial graph.  d_iter [2]; d_edges [n_edges], n_edges 0 or 1, with d_info [n_edges][81] and
 * d_walk_info [n_edges][18] of orbi_edge_information_device; d_group_state [1], d_edge_off [2], d_points [cap_edges][3], d_edge_z
 * [cap_edges][2], d_edge_inv_sigma2, d_active (read and written), d_chi2 [cap_edges], d_n_inliers [1]: NULL allowed with cap_edges == 0;
 * d_work [cap_edges * ORBVI_LOOP_EDGE_WORK + ORBVI_LOOP_FIXED_WORK]; d_trace [cap_trace][ORBVI_LOOP_TRACE] (NULL with cap_trace == 0);
 * d_summary [ORBVI_LOOP_SUMMARY].  One launch. */
int orbvi_pose_optimize_device(orbi_graph graph, int32_t *d_iter, const orbi_record *d_bank, int cap, const orbi_edge *d_edges, int n_edges,
                               const double *d_info, const double *d_walk_info, const orbi_prior *d_priors, int n_priors,
                               const orbi_prior_job *d_prior_jobs, int n_prior_jobs, orbi_calib calib, orbvi_camera camera, int cap_edges,
                               const int32_t *d_group_state, const int32_t *d_edge_off, const double *d_points, const double *d_edge_z,
                               const double *d_edge_inv_sigma2, uint8_t *d_active, orbvi_loop_options options, double *d_work, double *d_chi2,
                               int32_t *d_n_inliers, double *d_trace, int cap_trace, double *d_summary, int32_t *d_result, void *stream);

#ifdef __cplusplus
}
#endif
#endif
