/*
 * orbfi.h -- fullInertialOptimize's shared-bias graph linearised on the device (liborbx.so, gfx950).
 *
 * LocalMapping::initializeIMU (reference modules/Frontend/LocalMapping.cpp:427-463) runs inertialOptimize (orbii.h), applyScaleRotation
 * (orbm_apply_scale_rotation_device, orbm.h) and then Optimize::fullInertialOptimize(point_map, 100, beFirst, false, prioriG, prioriA)
 * (modules/Backend/Optimize.cpp:239-442).  The reference calls it with beFirst = true only (LocalMapping.cpp:57-59), the beInit branch:
 * a VertexPose and a velocity per key frame, key frame id 0 fixed, ONE gyro and ONE accelerometer Vertex3D for the whole map, an
 * EdgeInertial with Huber 4.1134 between consecutive key frames whose bias vertices are that one pair, two EdgePriori3D on the pair,
 * every map point a marginalised vertex with one EdgeMono per observation.  EdgeMono, the Schur complement, the 480-unknown ordered
 * Cholesky and the back-substitution are the visual-window header's; this header adds the inertial edge whose bias vertices live in a third state, the
 * gather that goes with it, the step-4 recovery that hands the one bias to every key frame, and the job lists of this graph shape.
 *
 * This header includes orbi.h and nothing includes it; like orbm.h it names the visual window's calls by what they do, not by their symbols
 * ("fullInertialOptimize as a chain on one stream", has the symbols).  Same rules as orbi.h: handle-less `*_device` entry points under the one
 * stream rule of orbx.h ("Streams and threads") -- a call enqueues on exactly the `stream` it is given (a hipStream_t; NULL is stream 0
 * itself), takes device pointers only, allocates nothing and never waits.  Arguments are checked first (ORBX_E_ARG: a null pointer, a
 * negative count, cap, n_src, n_dst or n_kf < 1, bias_state outside [0, n_states), a mode outside 0..1, a huber_delta or prior weight
 * that is not a number), then the limits (ORBX_E_UNSUPPORTED: more than ORBFI_MAX_KEYFRAMES key frames, more than ORBI_MAX_JOBS edges or
 * jobs), then the call fails with ORBX_E_NO_DEVICE without a HIP device.  There is no CPU path.  d_result is 8 x int32, WRITTEN by
 * every call.  Every index read from device memory is distrusted: dropped and counted, never dereferenced out of range.  No floating-point
 * atomics: the same input gives the same bytes.
 *
 * The graph is an orbi_graph (orbi.h) of n_kf + 1 states.
 *   [0, n_kf)   the key frames in getAllKeyFrames order (oldest first), d_fixed = ORBI_FIX_GYRO | ORBI_FIX_ACC: "no such vertex"; their
 *               bg, ba stay zero.  When the caller says key frame id 0 is still the first one (Optimize.cpp:268, fix_first), state 0 also
 *               has ORBI_FIX_POSE | ORBI_FIX_VELO.
 *   b = n_kf    the bias carrier, ORBI_FIX_POSE | ORBI_FIX_VELO: its bg, ba are the one bias pair; its pose and velocity are the last key
 *               frame's, fixed and never read by an edge.
 * This layout is exactly what orbi_graph_oplus_device, the visual window's linearise (n_solve = n_states = n_kf + 1: the carrier has no visual
 * edge), the visual window's reduce, the visual window's solve and the visual window's back-substitution take.  LIMIT: ORBFI_MAX_KEYFRAMES = ORBVW_MAX_SOLVE_STATES - 1 =
 * 31 key frames, the 480 unknowns of that solve; the reference reaches this step at 17 or a few more.  No second Cholesky is written.
 *
 * ---- orbfi_linearize_device ----
 *
 * computeError, linearizeOplus and constructQuadraticForm of the graph's inertial part.  Edge e = d_edges[e] = (i, j, rec; flags are
 * ignored) is EdgeInertial (G2oTypes.cpp:377-445) exactly as orbi_linearize_device evaluates it -- the float part, everything behind the
 * cast to double, the information d_info[81e ..) of orbi_edge_information_device, chi2, Huber: orbi.h, "Arithmetic", from the same internal
 * headers -- with two differences: the bias vertices, cast to float ahead of the deltas, are those of state `bias_state`, not of state i;
 * and the fixed mask of the Jacobian's columns 9..14 is the carrier's (columns 0..8: state i's, 15..23: state j's).
 *   priors   the two EdgePriori3D of Optimize.cpp:352-367 on the carrier: measurement = record prior_rec's updated_bias widened (the LAST
 *            key frame's, :354), Omega = p*I with p = prior_g / prior_a, floats widened to double.  e = measurement - estimate, J = -I,
 *            chi2 = (e0*(p*e0) + e1*(p*e1)) + e2*(p*e2); H[r][r] += p and b[r] += p*e_r for the dof the carrier's mask leaves free.
 *            d_chi2_prior[2] = (gyro, acc).  prior_rec outside [0, cap): both priors are dropped, their chi2 is zero, and d_result
 *            [ORBI_R_PRIOR_RANGE] = 2; otherwise d_result[ORBI_R_PRIOR_DONE] = 2.
 *   mode 0   WRITES (it does not add: it takes the place orbi_linearize_device has in the chain of the visual-window header)
 *            d_err[9e ..), d_chi2[e]; d_chi2_prior[2]; d_total[2] = (plain, robustified): the edges ascending from zero, then the gyro and
 *            the acc prior; d_float[15e ..) (may be NULL): the float dR, dV, dP of the edge;
 *            d_H_diag[n_states][225], d_b[n_states][15]: with M = J^T (w Omega) J (30 x 30, sums over the 9 rows ascending from zero) and
 *            m = -J^T (w Omega e) of an edge, a key frame s receives M[0:9, 0:9] and m[0:9] of the edges with i == s and M[15:24, 15:24],
 *            m[15:24] of those with j == s into [0:9, 0:9] and [0:9); the carrier receives M[9:15, 9:15], m[9:15] of ALL edges into
 *            [9:15, 9:15] and [9:15).  Each entry is summed from zero over the state's edges in ascending edge order, the two priors are
 *            added last (gyro, acc), and everything else of a block is zero.  A wave per state.
 *            d_off_edges[3 n_edges] (orbi_edge) with d_H_off[3 n_edges][225]: entries 3e, 3e + 1, 3e + 2 are (i, j, rec, 0) with M[0:9, 15:24]
 *            at [0:9, 0:9]; (i, b, rec, 0) with M[0:9, 9:15] at [0:9, 9:15]; (j, b, rec, 0) with M[15:24, 9:15] at [0:9, 9:15]; zeros fill
 *            the rest of each block.  The visual window's reduce takes the two arrays unchanged as its d_edges and d_H_off with n_edges = 3
 *            n_edges; entries naming the same pair add up there, so an interior key frame's two (s, b) entries do.
 *   mode 1   d_err, d_chi2, d_chi2_prior, d_total, d_float only; d_H_diag, d_b, d_off_edges, d_H_off may be NULL and are not touched.
 *   dropped  an edge with i, j or rec outside its range, i == j, or a state equal to bias_state (ORBI_R_RANGE), and an edge whose
 *            information orbi_edge_information_device refused (ORBI_R_REFUSED), writes zeros everywhere: d_err, d_chi2, d_float, its
 *            three d_H_off blocks and its three d_off_edges entries (all four ints 0: i == j, which the reduce skips and counts), and adds
 *            nothing.  The others are counted in ORBI_R_DONE.
 * d_work: ORBFI_EDGE_WORK doubles per edge, the caller's, both modes.  Two launches.
 *
 * ---- orbfi_recover_device ----
 *
 * Step 4 (Optimize.cpp:401-434) for n jobs d_jobs[3k ..) = (state, destination, flags): orbi_graph_recover_device AS WITH
 * ORBI_RECOVER_POSE WHATEVER THE FLAGS SAY -- (Rwb, twb, v) rounded to float into d_dst[15*destination ..), T_cw into d_pose_R[9k ..) /
 * d_pose_t[3k ..) (they go together, may be NULL), what orbm_local_ba_apply_device takes -- except that d_bias[6k ..) of EVERY job is
 * (bg, ba) of state bias_state rounded to float (newBias of :405-406, setImuBias for all).  The same drop and duplicate rules: out of
 * range ORBI_R_RANGE, a destination an earlier job names ORBI_R_DUPLICATE, the d_bias row of either zero.  The job's code is the one of
 * orbi_graph_recover_device, written once (csrc/orbi_factors_device.h).  One launch.
 *
 * ---- orbfi_jobs_device ----
 *
 * The job lists of this graph shape from an orbm_inertial_window_problem_device call (orbm.h) whose window was ALL key frames, oldest
 * first (every point is then local, no key frame is left over to be fixed, n_states = n_solve = n_kf there), without a read-back of lists.
 * Read: d_init_jobs [n_kf][3], d_inertial_edges [n_kf - 1], d_recover_jobs [n_kf][3].  Written:
 *   d_fixed [n_kf + 1]         as "The graph" above, from the host ints n_kf and fix_first
 *   d_init_out [n_kf + 1][3]   (k, key frame k's state row, -1: zero bias, "no such vertex") for the key frames; (n_kf, the LAST key frame's
 *                              state row, the last key frame's record) for the carrier: the record's updated_bias initialises the bias
 *                              vertices (:283-290)
 *   d_edges_out [n_kf - 1]     the edges with flags 0
 *   d_recover_out [n_kf][3]    the recover jobs, unchanged: a COPY, not a check -- these indices are distrusted where they are used,
 *                              by orbfi_recover_device (out of range: dropped and counted there), and are not counted here
 *   d_prior_rec [1]            the last key frame's record, for a caller that wants it (-1 when out of range)
 * Distrust: a state row outside [0, n_src) is written as -1 and a carrier record outside [0, cap) as -2, which orbi_graph_init_device
 * drops; an edge with i or j outside [0, n_kf), i == j or rec outside [0, cap) is written as (-1, -1, -1, 0), which every call drops; each
 * is counted in ORBI_R_RANGE, every other init job in ORBI_R_DONE.  One launch of one wave.
 *
 * ---- The chain ----
 *
 *   orbm_inertial_window_problem_device with d_window = all key frames -> ONE read-back of d_result's first 32 bytes
 *   orbfi_jobs_device -> orbi_graph_init_device (d_init_out, n_kf + 1 jobs) -> orbi_edge_information_device (d_edges_out)
 *   the caller's Levenberg-Marquardt loop: 100 iterations from a user lambda init of 1e-5 (:250).  One iteration:
 *     orbfi_linearize_device -> the visual window's linearise -> the visual window's reduce (d_off_edges, d_H_off, 3 n_edges) -> the visual window's solve ->
 *     the visual window's back-substitution -> orbi_graph_oplus_device -> both linearisations in mode 1 at the trial
 *     THE LOOP IS NOT HERE: its decisions are the caller's (tests/full_inertial_loop.py closes it as test code)
 *   orbfi_recover_device (d_recover_out)
 *   orbm_local_ba_apply_device, UNCHANGED, with an all-zero d_outlier: this optimiser classifies nothing
 *   orbi_set_bias_device (d_bias_ids, the recover's d_bias) -> orbi_prior_information_device (d_prior_info_jobs)
 *   orbm_inertial_window_velocity_prior_device -> orbm_build_observations_device -> orbm_refresh_points_device
 * The !beInit branch (biases per key frame, EdgeBiasWalk, no priors; Optimize.cpp:268-279, :331-349) is EXISTING CALLS ONLY: orbi_linearize_device
 * with ORBI_EDGE_WALKS, no prior jobs and Huber 4.1134, with the same visual side.
 * Not here: gravityOptimize / EdgeGravity, any loop, more than 31 key frames.
 *
 * Kernel resources (gfx950, VGPRs / scratch bytes / static LDS bytes; tests/test_full_inertial_resources.py reads them from the ISA):
 *   k_fi_edge 81 / 0 / 28640 B, k_fi_gather 26 / 0 / 32 B, k_fi_recover 54 / 0 / 32 B, k_fi_jobs 20 / 0 / 32 B.
 * At most 30 edges: every call is latency-bound, nothing has been tuned for throughput and no throughput claim is made.  An edge is one
 * wave, four per workgroup (k_fac_edge's shape and LDS slices); a wave per state then gathers in edge order from the caller's workspace.
 */
#ifndef ORBFI_H
#define ORBFI_H

#include "orbi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBFI_MAX_KEYFRAMES 31                           /* ORBVW_MAX_SOLVE_STATES - 1: the carrier is the 32nd solve state (ORBX_E_UNSUPPORTED above) */
#define ORBFI_EDGE_WORK 482                              /* doubles of workspace per edge (orbfi_linearize_device) */
#define ORBFI_HUBER_DELTA 4.1134                         /* Optimize.cpp:322-324 */

int orbfi_jobs_device(const int32_t *d_init_jobs, const orbi_edge *d_inertial_edges, const int32_t *d_recover_jobs, int n_kf, int fix_first, int n_src,
                      int cap, uint8_t *d_fixed, int32_t *d_init_out, orbi_edge *d_edges_out, int32_t *d_recover_out, int32_t *d_prior_rec,
                      int32_t *d_result, void *stream);

int orbfi_linearize_device(orbi_graph graph, const orbi_record *d_bank, int cap, float gravity, const orbi_edge *d_edges, int n_edges,
                           const double *d_info, int bias_state, int prior_rec, float prior_g, float prior_a, double huber_delta, int mode,
                           double *d_work, double *d_err, double *d_chi2, double *d_chi2_prior, double *d_total, double *d_H_diag, double *d_b,
                           orbi_edge *d_off_edges, double *d_H_off, float *d_float, int32_t *d_result, void *stream);

int orbfi_recover_device(orbi_graph graph, orbi_calib calib, int bias_state, const int32_t *d_jobs, int n, float *d_dst, int n_dst, float *d_bias,
                         double *d_pose_R, double *d_pose_t, int32_t *d_result, void *stream);

#ifdef __cplusplus
}
#endif
#endif
