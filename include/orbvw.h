/*
 * orbvw.h -- the visual window of the inertial local bundle adjustment on the device (liborbx.so, gfx950): EdgeMono with the map
 * points as marginalised vertices, the Schur complement over the points, the damped solve of the reduced system and the
 * back-substitution into the points.
 *
 * After the IMU is initialised every key frame runs Optimize::localFullBundleAdjustment (reference modules/Backend/Optimize.cpp:
 * 1064-1310, called from LocalMapping.cpp:46-49): 10 or 25 recent key frames with VertexPose + velocity + two biases (15 dof each),
 * up to 150 fixed key frames, every map point they see as a marginalised Vertex3D, and one EdgeMono (G2oTypes.cpp:59-69) per
 * observation.  orbi.h linearises the inertial part of that graph and applies an update; orbvi.h linearises EdgeMonoOnlyPose and
 * solves a system of at most four states.  This header adds what a window needs, so that one Levenberg-Marquardt iteration is a
 * chain on one stream
 *   orbi_linearize_device -> orbvw_linearize_device -> orbvw_reduce_device -> orbvw_solve_device -> orbvw_backsub_device ->
 *   orbi_graph_oplus_device -> orbi_linearize_device (mode 1) + orbvw_linearize_device (mode 1, on d_points_out)
 * and the caller reads back four scalars for its accept / reject decision: the two robustified totals at the trial point, d_out[0]
 * of the solve and d_out_points[0] of the back-substitution (their sum is g2o's computeScale without its + 1e-3).  THE LOOP ITSELF
 * IS NOT HERE: its decisions are the caller's.  A caller that closes it (tests/inertial_loop.py does, as test code): an
 * accepted trial makes d_points_out the next d_points (two buffers that swap), a rejected one restores Rwb, twb, v, bg, ba AND d_iter
 * (orbvi.h says why) and leaves d_points as it is; a refused solve (ORBI_R_REFUSED) is a rejected trial; without a user lambda init,
 * d_out[1] comes from one orbvw_reduce_device whose system is discarded.  Assembling this problem from the device-resident map
 * (getRecentKeyFrames) and the job list of the setPrioriInformation chaining behind the optimisation are
 * orbm_inertial_window_problem_device (orbm.h, "The inertial local BA window on the device-resident map"), which leaves its arrays in
 * the layout of the calls below.  Not here: inertialOptimize / fullInertialOptimize.
 * A caller that does not want to close the loop itself: orbwl.h (orbwl_window_optimize_device) closes it over these calls, and waits.
 *
 * This header includes orbvi.h and nothing includes it.  Same rules as there: handle-less `*_device` entry points under the one
 * stream rule of orbx.h ("Streams and threads") -- a call enqueues on exactly the `stream` it is given (a hipStream_t; NULL is stream
 * 0 itself), allocates nothing, copies nothing and never waits.  Arguments are checked first (ORBX_E_ARG: a null pointer, a
 * negative count, n_points < 1, n_solve outside [1, n_states], cap < 1, a mode outside 0..2, a huber_delta or chi2_threshold that is
 * not a number, a camera_model outside {0, 1}, d_points_out == d_points), then ORBX_E_UNSUPPORTED (more than ORBVW_MAX_SOLVE_STATES
 * solve states, ORBVW_MAX_EDGES edges, ORBVW_MAX_POINTS points, ORBI_MAX_JOBS states or inertial edges), then the call fails with
 * ORBX_E_NO_DEVICE without a HIP device.  There is no CPU path.  d_result is 8 x int32, WRITTEN by every call.
 *
 * The states.  The optimisable key frames are the states [0, n_solve) of an orbi_graph; fixed key frames follow as the states
 * [n_solve, n_states), of which only Rwb and twb are read.  An edge on a state >= n_solve hangs on a fixed pose whatever d_fixed
 * says; so does an edge on a state < n_solve with ORBI_FIX_POSE.
 *
 * Arithmetic (all four calls).  IEEE double: +, -, *, / and the correctly rounded sqrt (the Kannala-Brandt model adds atan and
 * atan2), no fused multiply-add, no floating-point atomics, each expression read left to right, a 3-term product-sum as (p0 + p1)
 * + p2, longer sums ascending from zero.  The same input gives the same bytes.  tests/vw_model.py restates every line in numpy.
 *
 * ---- orbvw_linearize_device: EdgeMono ----
 *
 * Edge e observes point d_edge_point[e] of d_points[n_points][3] from state d_edge_state[e], with the measurement d_edge_z[e][2] (kp.pt)
 * and the weight d_edge_inv_sigma2[e] (1 / kp.size^2): the arrays orbba_problem and orbm_local_ba_problem_device leave, edges sorted
 * by point.  d_active[cap_edges] (uint8, NULL = every edge active) is read only.  cap_edges is the number of edges.
 *
 * Distrust.  d_edge_point[e] is read as clamped to [0, n_points - 1] and then as the largest clamped value up to and including e, so
 * the edges of a point are one range.  The call WRITES these ranges to d_point_off[n_points + 1] in every mode: point l owns the edges
 * [d_point_off[l], d_point_off[l + 1]), d_point_off[0] = 0, d_point_off[n_points] = cap_edges.  An edge is DROPPED -- zeros in its d_err,
 * d_chi2, d_Hlp and d_outlier, nothing added anywhere -- and counted
 *   - in ORBI_R_REFUSED, once per POINT, when its point has more than ORBVW_MAX_OBS edges (the point is dropped whole);
 *   - else in ORBI_R_RANGE when its state lies outside [0, n_states);
 *   - else in ORBI_R_DUPLICATE when an EARLIER edge of the same point names the same state.
 * The others are counted in ORBI_R_DONE.  A kept edge whose error or chi2 is not finite and that is active (mode 2: every kept edge)
 * is counted in ORBVI_R_NONFINITE; it adds nothing to any sum and its error and chi2 are written as computed.
 *
 * The edge.  The pose derivation from (R_wb, t_wb), Pc, the error, chi2, project / getProjJacobian (csrc/orbba_camera.h), the float
 * t_bc and the 2 x 6 pose Jacobian J_p are EXACTLY those of orbvi.h ("Arithmetic": the pose, the edge, Jacobian), evaluated per edge.
 * Both kernels take them from one internal header, csrc/orbi_graph_device.h.  The point Jacobian is
 *   J_l = (-Jp)*R_cw,  (J_l)_rc = ((-Jp_r0)*R_0c + (-Jp_r1)*R_1c) + (-Jp_r2)*R_2c.
 * Huber is the one of orbi.h (huber_delta > 0; chi2 > delta*delta: rho = (2*sqrt(chi2))*delta - delta*delta, w = delta/sqrt(chi2); else rho =
 * chi2, w = 1).  W = w*inv_sigma2, We = (W*ex, W*ey).  With A, B each J_p or J_l: (A^T W B)_ab = A_0a*(W*B_0b) + A_1a*(W*B_1b) and
 * (A^T W e)_a = A_0a*We_0 + A_1a*We_1.
 * Modes.
 *   0   d_err[e][2] and d_chi2[e] of every edge.  The active, finite, kept edges ("used") then add:
 *       - per state s < n_solve without ORBI_FIX_POSE: J_p^T W J_p is ADDED to d_H_diag[225*s ..][0:6, 0:6] (upper triangle computed, the
 *         lower receives the same sums) and J_p^T W e is SUBTRACTED from d_b[15*s .. 15*s + 6): the call sits behind
 *         orbi_linearize_device, which writes these blocks.  One workgroup of 1024 threads per state walks ALL edges: thread t takes
 *         the edges t, t + 1024, ... in ascending order and adds those of its state to its 21 + 6 partial sums, which start at zero;
 *         each partial is reduced over the wave by the butterfly v = v + v[lane ^ o], o = 32, 16, 8, 4, 2, 1, and the sixteen wave
 *         results are added in ascending wave order, from zero (k_vi_linearize's order, over all edges).
 *       - d_Hll[l][9] (J_l^T W J_l, both triangles from the upper's sums) and d_bl[l][3] = 0 - J_l^T W e are WRITTEN for every point,
 *         each summed from zero over the point's used edges in ascending edge order.
 *       - d_Hlp[e][18] = the 3 x 6 J_l^T W J_p of the edge, row-major; zero for a fixed pose and for an edge that is not used.
 *       d_total[2] = (plain, robustified) chi2 of the used edges, summed over all edges in the workgroup order above.
 *   1   d_err, d_chi2, d_total only: what a trial needs.  d_work, d_H_diag, d_b, d_Hll, d_bl, d_Hlp may be NULL and are not touched.
 *   2   step 5 of the reference (Optimize.cpp:1255-1261): d_err and d_chi2 of every edge, d_outlier[e] = chi2 > chi2_threshold,
 *       literally that comparison, for every kept edge, counted in ORBVW_R_OUTLIER.  d_active is not read; everything of mode 0 and
 *       d_total may be NULL.
 * d_work: ORBVW_EDGE_WORK doubles per edge, the caller's (mode 0; NULL otherwise).
 *
 * ---- orbvw_reduce_device: the Schur complement ----
 *
 * d_S[N][N] (N = 15*n_solve, both triangles) and d_rhs[N] in two steps.
 *   base     the matrix and right-hand side of orbvi_solve_device: d_H_diag[s] at (s, s); for every inertial edge e of d_edges in
 *            ascending order d_H_off[e] ADDED at (i, j) and its transpose at (j, i), an off-diagonal block starting from zero (i, j or
 *            rec outside its range against n_solve and cap, or i == j: skipped, ORBI_R_RANGE); a dof that d_fixed fixes is an identity
 *            row and column with a zero right-hand side; *d_lambda, ONE double in device memory, is added to every free diagonal entry.
 *   points   per point l: M = d_Hll[l] with lambda added to its diagonal, symmetric (the upper triangle is read); the inverse by
 *            cofactors as k_lm_points has it: c00 = M11*M22 - M12*M12, c01 = M02*M12 - M01*M22, c02 = M01*M12 - M02*M11, det = (M00*c00 +
 *            M01*c01) + M02*c02, id = 1/det, inv = [c00*id, c01*id, c02*id; ., (M00*M22 - M02*M02)*id, (M01*M02 - M00*M12)*id; ., .,
 *            (M00*M11 - M01*M01)*id], mirrored, to d_Hll_inv[l][9]; d_tl[l] = inv*d_bl[l] (product-sums).  A determinant that is not finite
 *            or not > 0: the point is SKIPPED everywhere, counted in ORBVW_R_POINT_SINGULAR, and its d_Hll_inv and d_tl are zero.
 *   Schur    for every pair of states i <= j < n_solve with both poses free, one workgroup of 256 threads: thread t takes the points
 *            t, t + 256, ... in ascending order; for a point that is not skipped, has at most ORBVW_MAX_OBS edges and has an edge a on
 *            state i and an edge b on state j (the first such edge of its range each), with A = d_Hlp[a], B = d_Hlp[b]:
 *              C = inv*B (3 x 6 product-sums), T_rc = (A_0r*C_0c + A_1r*C_1c) + A_2r*C_2c, and for i == j u_r = (A_0r*tl_0 + A_1r*tl_1) + A_2r*tl_2
 *            are added to the thread's 36 + 6 partial sums; the butterfly and the four wave results ascending, from zero, as above.
 *            The sums are SUBTRACTED from d_S[15i + r][15j + c] and, the same value, from d_S[15j + c][15i + r] -- for i == j only the
 *            entries r <= c are computed -- and the u sums from d_rhs[15i + r].  d_S is symmetric whenever the base is.
 * d_point_off is read with every entry clamped to [0, cap_edges] and a range as [lo, max(lo, hi)), so nothing is read past
 * cap_edges.  These two calls only read edges per point, so the running maximum of orbvi.h's d_edge_off rule is not taken: ranges
 * that overlap give numbers that mean nothing, never an access outside the arrays.
 * d_out[1] = the largest undamped diagonal entry over the free dof of the base and over d_Hll of every point, 0 when none is larger:
 * what computeLambdaInit reads.  d_out[0] and d_out[2] are not touched.  d_result: ORBI_R_DONE = 1, ORBI_R_RANGE, ORBVW_R_POINT_SINGULAR.
 *
 * ---- orbvw_solve_device: the ordered Cholesky for N <= 480 ----
 *
 * Solves d_S*dx = d_rhs with the Cholesky, the forward and the backward substitution of orbvi.h, in exactly its orders: columns
 * ascend; for column j the pivot d = a_jj - s, s = the sum of l_jk*l_jk over k < j ascending from zero, l_jj = sqrt(d), r_j = 1/l_jj,
 * l_ij = (a_ij - s)*r_j with s = the sum of l_ik*l_jk over k < j ascending from zero; y_i = (rhs_i - s)*r_i, s over k < i ascending;
 * x_i = (y_i - s)*r_i, s = the sum of l_ki*x_k over k > i DESCENDING.  Only the LOWER triangle of d_S is read.  For n_solve <=
 * ORBVI_MAX_STATES this gives the bytes of orbvi_solve_device on the same system.  The matrix does not fit in LDS: it stays in d_S,
 * which L OVERWRITES (l_ij to both d_S[i][j] and d_S[j][i], so that a column of L is read along a row).  One workgroup of 512 threads, a
 * thread per row, one launch, left-looking in block columns of 15: a thread adds the products over the columns before the block for
 * all 15 columns at once and then continues each column's sum over the block's earlier columns, so the sum of every element still
 * ascends over k from zero.  The right-hand side rides along as row N of the matrix: its l_Nk is y_k by the same expression in the
 * same order, which is the forward substitution.
 *   outputs  d_dx[n_solve][15] = x.  d_out[0] = the sum over all dof j ascending from zero of dx_j*(lambda*dx_j + b_j), b the d_b
 *            orbvw_linearize_device left (NOT d_rhs): the pose side of g2o's computeScale.  d_out[2] = the smallest pivot.  d_out[1]
 *            is not touched.
 *   refusal  a pivot <= 0 or not finite: ORBI_R_REFUSED is counted instead of ORBI_R_DONE, d_dx is all zero, d_out[0] = 0 and
 *            d_out[2] is that pivot.
 *
 * ---- orbvw_backsub_device ----
 *
 * Per point l that reduce did not skip (a d_Hll_inv[l] that is not all zero): r = d_bl[l] - s, s_a = the sum over the point's edges e
 * ascending from zero of q_a(e) = the sum over c = 0..5 ascending from zero of Hlp(e)_ac*dx[15*state(e) + c] (edges on states outside
 * [0, n_solve) and points with more than ORBVW_MAX_OBS edges add nothing); x_l = inv*r (product-sums) to d_xl[l][3]; d_points_out[l] =
 * d_points[l] + x_l.  A skipped point has x_l = 0 and is copied unchanged.  d_points_out must not be d_points: a trial leaves the estimate
 * intact.  d_out_points[0] = the sum of c_l = (x_0*(lambda*x_0 + bl_0) + x_1*(lambda*x_1 + bl_1)) + x_2*(lambda*x_2 + bl_2) over the points:
 * one workgroup of 1024 threads, thread t takes the points t, t + 1024, ... ascending, the butterfly, the sixteen waves ascending.
 * d_result: ORBI_R_DONE = points updated, ORBVW_R_POINT_SINGULAR = points copied.
 *
 * Kernel resources (gfx950, VGPRs / scratch bytes / static LDS bytes; tests/test_vw_resources.py reads them from the ISA):
 *   k_vw_off_init 4 / 0 / 0 B, k_vw_off_first 4 / 0 / 0 B, k_vw_off_scan 28 / 0 / 4096 B, k_vw_edge 106 / 0 / 32 B, k_vw_point 62 / 0 / 0 B,
 *   k_vw_state 112 / 0 / 3456 B, k_vw_point_inv 43 / 0 / 0 B, k_vw_base 38 / 0 / 64 B, k_vw_schur 214 / 0 / 1344 B,
 *   k_vw_solve 114 / 0 / 63368 B, k_vw_backsub 82 / 0 / 0 B, k_vw_scale 32 / 0 / 160 B.
 * Every call is latency-bound (a window has a few thousand edges and at most 480 unknowns): nothing here has been tuned for
 * throughput and no throughput claim is made.
 */
#ifndef ORBVW_H
#define ORBVW_H

#include "orbvi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBVW_MAX_SOLVE_STATES 32  /* 480 unknowns (ORBX_E_UNSUPPORTED above) */
#define ORBVW_MAX_EDGES (1 << 20)  /* EdgeMono per call */
#define ORBVW_MAX_POINTS (1 << 18) /* map points per call */
#define ORBVW_MAX_OBS 256          /* edges per point; a point with more is dropped whole */
#define ORBVW_EDGE_WORK 24         /* doubles of workspace per edge (orbvw_linearize_device, mode 0) */
#define ORBVW_R_OUTLIER 5          /* d_result of orbvw_linearize_device, mode 2: edges with chi2 > chi2_threshold */
#define ORBVW_R_POINT_SINGULAR 6   /* d_result of orbvw_reduce_device / orbvw_backsub_device: points skipped / copied unchanged */

/* computeError, linearizeOplus and constructQuadraticForm of cap_edges EdgeMono (mode 0), their errors only (mode 1), or their outlier
 * classification (mode 2).  huber_delta: (double)sqrtf(5.991); chi2_threshold: 5.991 (mode 2 only).  d_point_off [n_points + 1]
 * (WRITTEN, every mode); d_err [cap_edges][2], d_chi2 [cap_edges]; d_total [2] (modes 0, 1); d_work [cap_edges][ORBVW_EDGE_WORK], d_H_diag
 * [n_states][225] and d_b [n_states][15] (ADDED to), d_Hll [n_points][9], d_bl [n_points][3], d_Hlp [cap_edges][18] (mode 0); d_outlier
 * [cap_edges] (mode 2).  Six launches in mode 0, five in mode 1, four in mode 2. */
int orbvw_linearize_device(orbi_graph graph, orbi_calib calib, orbvi_camera camera, int n_solve, int n_points, int cap_edges, const double *d_points,
                           const int32_t *d_edge_state, const int32_t *d_edge_point, const double *d_edge_z, const double *d_edge_inv_sigma2,
                           const uint8_t *d_active, double huber_delta, double chi2_threshold, int mode, int32_t *d_point_off, double *d_work,
                           double *d_err, double *d_chi2, double *d_total, double *d_H_diag, double *d_b, double *d_Hll, double *d_bl, double *d_Hlp,
                           uint8_t *d_outlier, int32_t *d_result, void *stream);

/* The reduced system.  d_fixed [n_solve]; d_edges / d_H_off [n_edges][225] may be NULL with n_edges == 0; cap: the size of the record bank
 * the edges' `rec` is held against; d_H_diag [n_solve][225], d_b [n_solve][15]; d_lambda [1]; d_point_off [n_points + 1], d_edge_state
 * [cap_edges], d_Hll, d_bl, d_Hlp as orbvw_linearize_device left them.  Written: d_S [N][N], d_rhs [N], d_Hll_inv [n_points][9], d_tl
 * [n_points][3], d_out[1].  Three launches. */
int orbvw_reduce_device(int n_solve, const uint8_t *d_fixed, const orbi_edge *d_edges, int n_edges, int cap, const double *d_H_diag,
                        const double *d_H_off, const double *d_b, const double *d_lambda, int n_points, int cap_edges, const int32_t *d_point_off,
                        const int32_t *d_edge_state, const double *d_Hll, const double *d_bl, const double *d_Hlp, double *d_S, double *d_rhs,
                        double *d_Hll_inv, double *d_tl, double *d_out, int32_t *d_result, void *stream);

/* The ordered Cholesky solve of d_S*dx = d_rhs; d_S [N][N] is OVERWRITTEN with L.  d_b [n_solve][15] and d_lambda [1] enter d_out[0]
 * only.  d_dx [n_solve][15]; d_out [3]: [0] and [2] written.  One launch. */
int orbvw_solve_device(int n_solve, double *d_S, const double *d_rhs, const double *d_b, const double *d_lambda, double *d_dx, double *d_out,
                       int32_t *d_result, void *stream);

/* The points' step.  d_dx [n_solve][15]; d_xl [n_points][3], d_points_out [n_points][3] (not d_points), d_out_points [1].  Two launches. */
int orbvw_backsub_device(int n_solve, int n_points, int cap_edges, const int32_t *d_point_off, const int32_t *d_edge_state, const double *d_Hlp,
                         const double *d_Hll_inv, const double *d_bl, const double *d_dx, const double *d_lambda, const double *d_points,
                         double *d_xl, double *d_points_out, double *d_out_points, int32_t *d_result, void *stream);

#ifdef __cplusplus
}
#endif
#endif
