/*
 * orbwl.h -- localFullBundleAdjustment's Levenberg-Marquardt loop in the library (liborbx.so, gfx950): the window loop.
 *
 * After the IMU is initialised every key frame runs Optimize::localFullBundleAdjustment (reference modules/Backend/Optimize.cpp:
 * 1064-1310, called from LocalMapping.cpp:46-49).  The library's staged calls serve every stage of one iteration of it -- the inertial
 * linearisation and the update of orbi.h, and the visual window's four calls: EdgeMono's linearisation, the Schur complement, the
 * ordered Cholesky solve and the back-substitution ("The window loop closed by the host", names their header, which like
 * orbm.h this one names by what its calls do) -- and left the loop to the caller.  orbwl_window_optimize_device closes it:
 * optimizer.optimize(iterations) with g2o's policy, the vertices' push and pop, and the classification of Optimize.cpp:1255-1261.
 * The mapper's chain on a device-resident map is then
 *   orbm_inertial_window_problem_device -> orbi_graph_init_device -> orbi_edge_information_device -> orbwl_window_optimize_device ->
 *   orbi_graph_recover_device -> orbm_local_ba_apply_device (with this call's d_outlier) -> orbi_prior_information_device
 *
 * This header includes orbvi.h and nothing includes it.  A handle-less `*_device` entry point under the one stream rule of orbx.h: it
 * enqueues on exactly the `stream` it is given (NULL is stream 0 itself) and allocates nothing in the steady state.
 * THIS CALL WAITS ON THE CALLER'S STREAM, ONCE PER TRIAL AND ONCE AT THE END.  orbba_local_bundle_adjustment_device does the same; it
 * is the second exception to "never waits".  Why the host closes the loop: the window's stages are grids (a workgroup per state, per
 * pair of states, over thousands of edges and points), one workgroup walking them would serialise a machine's worth of work, joining
 * workgroups inside one launch needs a barrier that spins on memory, which this library does not write, and the mapper's abort flag
 * lives in host memory.  What the host reads per trial is ONE 16-byte verdict in page-locked memory and nothing else: the policy, the
 * push and pop, the trace and the counters run on the device.  The page-locked block comes from a workspace leased for the call
 * (csrc/orb_host.h), pooled per device, so two host threads may be inside the call at once.  Any HIP error ends the call at once:
 * nothing more is enqueued behind a failed wait.
 *
 * The stages.  The driver calls the library's own staged entry points in the order tests/inertial_loop.py's DeviceWindow runs them; no
 * stage kernel is restated, so one linearisation, reduce, solve, back-substitution and update inside the loop give the bytes of the
 * staged calls on the same input.  Per iteration: both linearisations (mode 0), current = their robustified totals.  Per trial: the
 * Schur step at *d_lambda, the solve, the back-substitution from the live point buffer into the other, the push (ahead of an
 * iteration's first trial: a popped estimate is the pushed one), orbi_graph_oplus_device ON THE STATES [0, n_solve) ONLY -- a state
 * >= n_solve never changes a byte --, both error evaluations (mode 1) at the trial point, k_vwl_decide, the wait.  An accepted trial
 * makes the other point buffer the live one; at the end the live buffer is copied to d_points when it is not d_points.
 *
 * The policy is tests/inertial_loop.py's optimize / local_full line by line (csrc/orb_lm_policy.h), by ONE lane in IEEE double, in its
 * expression order: temp = the two totals' sum, or DBL_MAX behind a refused solve (ORBI_R_REFUSED in the solve's own result slot);
 * scale = (pose + points) + 1e-3; rho = (current - temp) / scale; accepted when rho > 0 and temp is finite: lambda *= max(1/3, min(1 -
 * x*x*x, 2/3)) with x = 2*rho - 1 -- THE CUBE IS x*x*x, not pow --, nu = 2; otherwise lambda *= nu, nu *= 2 and the pop, which restores
 * Rwb, twb, v, bg, ba AND d_iter of the solve states; the iteration ends when rho >= 0 or the trials run out, the optimisation when
 * qmax == max_trials, rho == 0 or lambda is not finite.  lambda_init > 0 is setUserLambdaInit (the reference uses 1e0, or 1e-2 with
 * beLarge); < 0 is EXACTLY 0: G2O CANNOT REACH THAT VALUE, it exists, as in orbvi_loop.h, so that the refused-solve path can be
 * reached; == 0 is ORBX_E_UNSUPPORTED: this optimiser always sets a user value and computeLambdaInit would cost a discarded reduce.
 *
 * The stop flag.  `stop` is a HOST pointer (NULL: no flag), the mapper's abort_BA.  The host reads *stop before every iteration and
 * before every further trial of an iteration; a value other than 0 ends the loop there, between two steps, so no trial is left
 * half-applied.  This is this library's rule: no parity with where g2o tests its force-stop flag is claimed.
 *
 * At return, whatever ended the loop: the final estimate is in the graph, d_iter and d_points, and EVERY EDGE IS CLASSIFIED (mode 2 of
 * the visual linearisation at the final estimate: d_chi2 and d_outlier), as the listing runs its steps 5 to 7 behind an aborted
 * optimisation too.
 *
 * Outputs.  d_trace[cap_trace][ORBWL_TRACE], one row per trial: iteration, trial, lambda, current, temp, scale, rho, ok (the solve was
 * not refused), the inertial and the visual total at the trial, computeScale's pose part, its points part, accepted --
 * inertial_loop.FIELDS, the layout of ORBVI_LOOP_TRACE; trials past cap_trace are counted and not written.
 * d_summary[ORBWL_SUMMARY]: [0] the iterations run (one the flag cut short is not counted), [1] the trials, [2] the accepted trials,
 * [3] the refused solves, [4] the last lambda, [5] the outliers, [6] the trials that found no row in the trace, [7] 1 when the stop
 * flag ended the loop.  d_result[8]: [ORBI_R_DONE] accepted trials, [ORBWL_R_REJECTED] rejected trials, [ORBI_R_REFUSED] refused
 * solves, [ORBWL_R_OUTLIER] the outliers, and of the last evaluation [ORBI_R_RANGE] (the classification's dropped edges and the last
 * inertial error evaluation's), [ORBVI_R_NONFINITE] (the classification's) and [ORBWL_R_POINT_SINGULAR] (the last Schur step's).
 *
 * d_work is the caller's ONE scratch block of orbwl_window_work_doubles(...) doubles, 16-byte aligned; nothing in it need be
 * initialised and nothing in it is an output.  The library carves it into these slices, in this order, each rounded up to an even
 * number of doubles so that every slice is 16-byte aligned (S = n_states, N = 15 n_solve, L = n_points, E = cap_edges, J = n_edges,
 * P = n_prior_jobs):
 *   H_diag 225 S, H_off 225 J, b 15 S; the inertial work 488 J (ORBI_EDGE_WORK), errors 9 J, chi2 3 J, prior chi2 3 P, totals 4 (mode
 *   0 and mode 1); the EdgeMono work 24 E, errors 2 E, totals 4, Hll 9 L, bl 3 L, Hlp 18 E, point_off (L + 1) int32; S N N, rhs N,
 *   Hll_inv 9 L, tl 3 L, dx N, xl 3 L; the second point buffer 3 L; d_out 3, d_out_points 1, d_lambda 1; the saved vertices 21 n_solve
 *   with their d_iter n_solve int32; the control block 16; one 8-int result slot per stage call, 9 slots (so that the solve's refusal
 *   survives the calls behind it).
 *
 * Argument checks first: ORBX_E_ARG (a null pointer other than d_priors / d_prior_jobs without prior jobs, d_active, d_trace with
 * cap_trace == 0 and stop; a negative count; cap < 1; n_points < 1; n_solve outside [1, n_states]; iterations or max_trials < 1; an
 * option that is not a number; a camera_model outside {0, 1}; a d_work that is not 16-byte aligned), then ORBX_E_UNSUPPORTED (the
 * limits of the staged calls: more than 32 solve states, 2^20 edges, 2^18 points, ORBI_MAX_JOBS states, inertial edges or prior
 * jobs; iterations above ORBWL_MAX_ITERATIONS, max_trials above ORBWL_MAX_TRIALS; lambda_init == 0), then ORBX_E_NO_DEVICE.  There is
 * no CPU path.
 *
 * Kernel resources (gfx950, VGPRs / scratch bytes / static LDS bytes; tests/test_vw_loop_resources.py reads them from the ISA):
 *   k_vwl_begin 4 / 0 / 0 B, k_vwl_push 18 / 0 / 0 B, k_vwl_decide 28 / 0 / 4 B, k_vwl_end 10 / 0 / 0 B.
 * Latency-bound like the staged calls; tools/vw_window_loop_latency.py records what a whole optimisation takes.
 * localInertialBundleAdjustment, which the mapper runs directly in front of this function when the tracker is RECENTLY_LOST, has no
 * points and no grid-sized stage: orbil_chain_optimize_device (orbil.h) runs it whole in one launch of one workgroup, without a wait.
 */
#ifndef ORBWL_H
#define ORBWL_H

#include "orbvi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBWL_MAX_ITERATIONS 100   /* of one optimisation */
#define ORBWL_MAX_TRIALS 10        /* per iteration: g2o's default _maxTrialsAfterFailure */
#define ORBWL_TRACE 13             /* doubles of a row of d_trace */
#define ORBWL_SUMMARY 8            /* doubles of d_summary */
#define ORBWL_R_REJECTED 2         /* d_result: rejected trials */
#define ORBWL_R_OUTLIER 5          /* d_result: edges with chi2 > chi2_threshold at the final estimate */
#define ORBWL_R_POINT_SINGULAR 6   /* d_result: points the last Schur step skipped */

typedef struct orbwl_loop_options {    /* by value */
    int32_t iterations;                /* 1 .. 100: 10 in the reference, 25 with beLarge */
    int32_t max_trials;                /* 1 .. 10 */
    double lambda_init;                /* > 0 setUserLambdaInit (1e0, or 1e-2 with beLarge), < 0 exactly 0 (g2o cannot reach it), 0 unsupported */
    double huber_delta_visual;         /* (double)sqrtf(5.991) */
    double huber_delta_inertial;       /* 0 in this optimiser: EdgeInertial carries no robust kernel */
    double chi2_threshold;             /* 5.991 */
    float gravity, pad;
} orbwl_loop_options;

/* The size of d_work in doubles: host arithmetic only, no device needed.  Negative on a negative count, n_states, n_solve or n_points
 * < 1, or n_solve > n_states. */
int64_t orbwl_window_work_doubles(int n_states, int n_solve, int n_points, int cap_edges, int n_edges, int n_prior_jobs);

/* optimizer.optimize(options.iterations) and the classification of a window, in the layouts orbm_inertial_window_problem_device leaves.
 * d_iter [n_states]; d_edges [n_edges] with d_info [n_edges][81] and d_walk_info [n_edges][18] of orbi_edge_information_device (the
 * caller's call, once, before this one); d_points [n_points][3] (in and out); d_edge_state, d_edge_point [cap_edges], d_edge_z
 * [cap_edges][2], d_edge_inv_sigma2 [cap_edges]; d_active [cap_edges] (NULL: every edge active); d_work [orbwl_window_work_doubles];
 * d_chi2 [cap_edges], d_outlier [cap_edges]; d_trace [cap_trace][ORBWL_TRACE] (NULL with cap_trace == 0); d_summary [ORBWL_SUMMARY];
 * d_result [8]; stop: a HOST pointer or NULL.  WAITS on `stream` once per trial and once at the end. */
int orbwl_window_optimize_device(orbi_graph graph, int32_t *d_iter, const orbi_record *d_bank, int cap, const orbi_edge *d_edges, int n_edges,
                                 const double *d_info, const double *d_walk_info, const orbi_prior *d_priors, int n_priors,
                                 const orbi_prior_job *d_prior_jobs, int n_prior_jobs, orbi_calib calib, orbvi_camera camera, int n_solve,
                                 int n_points, int cap_edges, double *d_points, const int32_t *d_edge_state, const int32_t *d_edge_point,
                                 const double *d_edge_z, const double *d_edge_inv_sigma2, const uint8_t *d_active, orbwl_loop_options options,
                                 double *d_work, double *d_chi2, uint8_t *d_outlier, double *d_trace, int cap_trace, double *d_summary,
                                 int32_t *d_result, const volatile int32_t *stop, void *stream);

#ifdef __cplusplus
}
#endif
#endif
