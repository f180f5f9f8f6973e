/*
 * orbil.h -- localInertialBundleAdjustment on the device: the damped step of a chain of inertial states and the whole optimisation in
 * one launch (liborbx.so, gfx950).
 *
 * Optimize::localInertialBundleAdjustment (reference modules/Backend/Optimize.cpp:953-1062) is what the mapper runs when the tracker is
 * RECENTLY_LOST (LocalMapping.cpp:47-48), directly in front of localFullBundleAdjustment: the last min(n, 10 or 20) key frames with every
 * pose fixed, the velocity and both biases of the oldest fixed too (:992-1007), one EdgeInertialOnly with its two EdgeBiasWalk between
 * neighbours (:1012-1029), no prior, no robust kernel, optimize(10) with g2o's default computeLambdaInit (:1034-1036), and the recovery
 * (:1044-1053).  Every formula of it is orbi_factors.h's; the trial policy is csrc/orb_lm_policy.h's.  This header adds the two pieces
 * that were missing: a solve for this graph, and the loop.
 *
 * This header includes orbvi.h and nothing includes it; the rules are orbvi.h's: handle-less `*_device` entry points under the one
 * stream rule of orbx.h ("Streams and threads"), which enqueue on exactly the `stream` they are given (NULL is stream 0 itself),
 * allocate nothing, copy nothing and never wait; there is no CPU path.  d_result is 8 x int32, WRITTEN by every call.
 *
 * ---- orbil_chain_solve_device: the damped step of a chain ----
 *
 * Solves (H + lambda*I)*dx = b over the free dof of a CHAIN of 2 <= n_states <= ORBIL_MAX_STATES states (20: the reference's maxOpt with
 * beLarge; up to 19 free states x 9 dof, block-tridiagonal).  The arguments and outputs are orbvi_solve_device's -- d_fixed, d_edges,
 * n_edges, cap, d_H_diag, d_H_off, d_b, *d_lambda in device memory; d_dx [n_states][15]; d_out [3] = (computeScale without its + 1e-3,
 * the largest H_jj over the free dof before damping, the smallest or refusing pivot); the d_result counters --, with one more: d_work,
 * the caller's scratch of ORBIL_SOLVE_WORK(n_states) doubles, nothing in it an input or an output.
 *   Distrust    an edge is dropped and counted in ORBI_R_RANGE when orbi.h's rule refuses it (i, j or rec outside its range, i == j)
 *               or when |i - j| != 1: its block falls outside the band.
 *   Arithmetic  orbvi_solve_device's, on a band.  A dof that d_fixed fixes is an identity row and column with a zero right-hand side.
 *               Columns ascend; each inner sum runs ascending over the columns of the band, from zero; one sqrt and one reciprocal per
 *               column; the forward substitution ascends, the backward one descends; computeScale is summed ascending over all 15n rows
 *               from zero.  IEEE double, nothing fused, no floating-point atomic: the same input gives the same bytes.
 *   Refusal     a pivot d with !(d > 0) or not finite: ORBI_R_REFUSED is counted instead of ORBI_R_DONE, d_dx is all zero, d_out[0] = 0
 *               and d_out[2] is that pivot.
 *   Bytes       block column s of the factor touches only the rows of blocks s and s + 1.  The terms the dense order of
 *               orbvi_solve_device adds outside the band are products with an exact zero, so on a chain of finite values the band order
 *               gives the dense order's bytes: for n_states <= ORBVI_MAX_STATES d_dx and d_out are those of orbvi_solve_device on the
 *               same input (tests/test_inertial_chain_gpu.py holds it to that).
 *   Where the factor lives.  NOT whole in LDS: 15n rows x 30 doubles are 72 KB at n = 20, beyond the 64 KB of static LDS every kernel of
 *               this library stays within.  THE BAND is in d_work: row i of the 15n has 30 doubles, the columns of the block before its own
 *               and of its own.  One workgroup assembles A there; one wave then walks the n block columns.  In step s the 30 rows of
 *               blocks s and s + 1 are the wave's tile in LDS, a lane per row (which it keeps in registers), factorised as orbvi_solve_device does a matrix; the forward
 *               substitution of block s runs in the same step; the finished rows of block s go back to the band.  The backward
 *               substitution reads the blocks L[s+1,s] and L[s,s] back from the band behind the wave's fence.  The tile is two blocks
 *               of 15 rows by 31 doubles, addressed by the parity of the block, so nothing is moved between the steps.
 *
 * ---- orbil_chain_optimize_device: localInertialBundleAdjustment's optimisation whole, in one launch ----
 *
 * ONE KERNEL LAUNCH OF ONE WORKGROUP (512 threads) on the stream it is given: optimize(iterations), g2o's Levenberg-Marquardt policy,
 * the vertices' push and pop, with no allocation, no copy, no wait and no read-back.  The chain of a mapper step is
 *   orbm_inertial_chain_problem_device (orbm.h) -> orbi_graph_init_device -> orbi_edge_information_device
 *     -> orbil_chain_optimize_device -> orbi_graph_recover_device -> orbi_set_bias_device -> orbm_inertial_chain_velocity_priors_device
 * and the host knows every size of it, so the chain has no read-back at all.  The rules and the text of orbvi_loop.h apply: the kernel
 * runs the device functions of csrc/orbvi_stages.h that k_fac_edge, k_fac_gather and k_fac_oplus run, and the band walk of the call
 * above, so a linearisation, a solve and an update inside the loop give the bytes of the staged calls on the same input; the policy's
 * arithmetic is csrc/orb_lm_policy.h's, in IEEE double, by ONE lane, published through LDS.
 *
 * Inputs.  An orbi_graph of 2 .. ORBIL_MAX_STATES states with the caller's `fixed` flags (the assembly's d_fixed) and d_iter [n_states],
 * the update counters orbi_graph_oplus_device keeps; the record bank; d_edges [n_edges], n_edges <= n_states - 1, with their d_info /
 * d_walk_info of orbi_edge_information_device; d_priors and d_prior_jobs, at most ORBVI_LOOP_MAX_PRIOR_JOBS (the reference passes none
 * here; the gather applies them at no cost); d_work, the caller's scratch of ORBIL_LOOP_WORK doubles, nothing in it an input or an
 * output; d_trace [cap_trace][ORBVI_LOOP_TRACE]; the options by value.
 * Distrust, as in the staged calls: an edge whose states or record are out of range, or whose information was refused, takes no part
 * in the linearisation; an edge the band cannot hold takes no part in the solve; a prior job out of range is dropped; each is counted.
 *
 * What it does is tests/inertial_loop.py's optimize line by line on the back-end ModelPose(visual=False).  Per iteration: every edge by
 * a wave in its own LDS slice, the edges in passes over the eight waves; then the gather, a wave per state, and the totals (mode 0);
 * current = the robustified total.  At iteration 0 lambda = lambda_init when that is > 0 (setUserLambdaInit), tau * the largest free
 * diagonal entry of H before damping when it is 0 (computeLambdaInit, taken directly behind the assembly: no solve is discarded), and
 * EXACTLY 0 when it is < 0: G2O CANNOT REACH THAT VALUE; it exists so that the refusal path is reachable from the ABI, as in
 * orbvi_loop_options.  Then up to max_trials trials: push (Rwb, twb, v, bg, ba AND d_iter of every state, ahead of the first trial of
 * the iteration), the chain solve with the loop's lambda, oplus, the error evaluation (mode 1) at the trial point, temp = its total or
 * DBL_MAX behind a refused solve, lm_policy_trial, the pop on a rejected trial, which restores d_iter as well, and one row of the trace.
 * lm_policy_again and lm_policy_terminate end the iteration and the optimisation exactly as in orbvi_pose_optimize_device.
 *
 * Outputs.  The graph and d_iter in place.  d_trace: one row per trial, inertial_loop.FIELDS (the visual total and the points' side of
 * computeScale are 0); trials past cap_trace are counted and not written.  d_summary [ORBIL_SUMMARY]: [0] the iterations run, [1] the
 * trials, [2] the accepted trials, [3] the refused solves, [4] the last lambda, [5] the trials in all, [6] those that found no row in the
 * trace, [7] 0.  d_result (one workgroup writes it): [ORBI_R_DONE] accepted trials, [ORBI_R_RANGE] what the last evaluation dropped (edges
 * of the linearisation and blocks of the solve), [2] rejected trials, [ORBI_R_REFUSED] refused solves, [4] 0, [ORBI_R_PRIOR_RANGE] prior
 * jobs dropped, [6] 0, [ORBVI_R_EDGE_REFUSED] edges refused by their information.
 *
 * Safety of the shape.  A single workgroup of 512 threads; no inter-workgroup synchronisation, no spin-wait on memory; the one loop is
 * bounded by iterations * (1 + max_trials) + 1 steps, computed on the host from the checked options; every barrier is in control flow
 * uniform across the workgroup; each decision (accepted, terminate, refused) is taken by one lane, published through LDS and read by all
 * lanes behind a barrier before they branch; global memory the workgroup wrote is read back only behind a barrier (inside the solve's one
 * wave: behind that wave's fence).  The solve's LDS (the tile and its vectors) lies over the edges' slices: the two are never live together.
 * Argument checks first: ORBX_E_ARG (a null pointer, a negative count, n_states or cap < 1, iterations or max_trials < 1, a tau,
 * huber_delta, gravity or lambda_init that is not a number); ORBX_E_UNSUPPORTED (n_states outside 2 .. ORBIL_MAX_STATES, more than
 * n_states - 1 edges, more than ORBVI_LOOP_MAX_PRIOR_JOBS prior jobs, iterations or max_trials above ORBVI_LOOP_MAX_ITERATIONS,
 * ORBVI_LOOP_MAX_TRIALS); then ORBX_E_NO_DEVICE.
 * Kernel resources (gfx950, VGPRs / scratch bytes / static LDS bytes; tests/test_inertial_chain_resources.py reads them from the ISA):
 *   k_il_chain_solve 127 / 0 / 15872 B, k_il_chain_loop 256 / 0 / 59928 B.
 * Latency-bound like the staged calls; tools/chain_loop_latency.py records what a whole optimisation takes.
 */
#ifndef ORBIL_H
#define ORBIL_H

#include "orbvi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBIL_MAX_STATES 20                   /* the reference's maxOpt with beLarge (ORBX_E_UNSUPPORTED above, and below 2) */
#define ORBIL_SOLVE_WORK(n) (450 * (n))       /* doubles of d_work of orbil_chain_solve_device: the band, 15 rows x 30 per state */
#define ORBIL_LOOP_WORK 32768                 /* doubles of d_work of orbil_chain_optimize_device */
#define ORBIL_SUMMARY 8                       /* doubles of d_summary */

typedef struct orbil_chain_options {          /* by value */
    int32_t iterations;                       /* 1 .. ORBVI_LOOP_MAX_ITERATIONS: 10 in the reference */
    int32_t max_trials;                       /* 1 .. ORBVI_LOOP_MAX_TRIALS */
    double lambda_init;                       /* > 0 setUserLambdaInit, 0 computeLambdaInit, < 0 exactly 0 (g2o cannot reach it) */
    double tau;                               /* 1e-5 in g2o */
    double huber_delta;                       /* of EdgeInertialOnly: 0 (no robust kernel) in the reference */
    float gravity, pad;
} orbil_chain_options;

/* The damped step of a chain.  d_fixed [n_states]; d_edges / d_H_off [n_edges][225] may be NULL with n_edges == 0; cap: the size of the
 * record bank the edges' `rec` is held against; d_lambda [1]; d_work [ORBIL_SOLVE_WORK(n_states)]; d_dx [n_states][15]; d_out [3].
 * One launch. */
int orbil_chain_solve_device(int n_states, const uint8_t *d_fixed, const orbi_edge *d_edges, int n_edges, int cap, const double *d_H_diag,
                             const double *d_H_off, const double *d_b, const double *d_lambda, double *d_work, double *d_dx, double *d_out,
                             int32_t *d_result, void *stream);

/* The whole optimisation of a chain of inertial states.  d_iter [n_states]; d_edges [n_edges], n_edges <= n_states - 1, with d_info
 * [n_edges][81] and d_walk_info [n_edges][18]; d_priors / d_prior_jobs may be NULL with n_prior_jobs == 0; d_work [ORBIL_LOOP_WORK];
 * d_trace [cap_trace][ORBVI_LOOP_TRACE] (NULL with cap_trace == 0); d_summary [ORBIL_SUMMARY].  One launch. */
int orbil_chain_optimize_device(orbi_graph graph, int32_t *d_iter, const orbi_record *d_bank, int cap, const orbi_edge *d_edges, int n_edges,
                                const double *d_info, const double *d_walk_info, const orbi_prior *d_priors, int n_priors,
                                const orbi_prior_job *d_prior_jobs, int n_prior_jobs, orbil_chain_options options, double *d_work,
                                double *d_trace, int cap_trace, double *d_summary, int32_t *d_result, void *stream);

#ifdef __cplusplus
}
#endif
#endif
