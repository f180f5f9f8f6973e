/*
 * orbvi.h -- the visual edges of the inertial optimisers and their damped step on the device (liborbx.so, gfx950).
 *
 * After the IMU is initialised every tracked frame runs poseFullOptimize (reference modules/Backend/Optimize.cpp:610-764); the key
 * frame-less case is poseInertialOptimize (:547-608).  Their graphs hold the inertial states, edges and priors of orbi.h ("Inertial
 * factors linearised on the device") and one EdgeMonoOnlyPose (G2oTypes.cpp:49-57, G2oTypes.h:47-54) per matched map point on the
 * frame's VertexPose: a few hundred to 2000 edges, the only large part.  orbi.h linearises the inertial part and applies an update;
 * this header adds the two layers between them, so that one Levenberg-Marquardt iteration is a chain on one stream
 *   orbi_graph_init_device -> orbi_edge_information_device -> orbi_linearize_device -> orbvi_linearize_device ->
 *   orbvi_solve_device -> orbi_graph_oplus_device -> orbi_linearize_device (mode 1) + orbvi_linearize_device (mode 1)
 * and the caller reads back two scalars (the chi2 at the trial point, d_out[0] of the solve) for its accept / reject decision.  In
 * these STAGED calls THE LOOP ITSELF IS NOT HERE: its decisions are the caller's.  The tracker's two loops, closed, are
 * orbvi_pose_optimize_device (orbvi_loop.h; the end of this comment): one launch on the same stage code.  A caller that closes the staged chain
 * itself (tests/inertial_loop.py does, as test code) needs two things no staged call does for it.  The lambda init: d_out[1], what
 * computeLambdaInit multiplies by tau, is written by orbvi_solve_device only, so iteration 0 of every optimize() costs one solve whose step is discarded (any *d_lambda; a refused
 * solve writes d_out[1] all the same).  The pop: g2o pushes CameraImuPose WITH its update counter, so a rejected trial restores d_iter
 * along with Rwb, twb, v, bg and ba -- a counter left as the trial set it renormalises the rotation at other updates than the
 * reference.  Not here either: EdgeMono (G2oTypes.cpp:59-69), where the
 * map points are vertices too -- a local window needs the Schur complement over its points, which is a later layer, and this is
 * also why the solve stops at ORBVI_MAX_STATES states.
 *
 * This header includes orbi.h and is not included by it.  Same rules as there: handle-less `*_device` entry points under the one
 * stream rule of orbx.h ("Streams and threads") -- a call enqueues on exactly the `stream` it is given (a hipStream_t; NULL is stream
 * 0 itself), allocates nothing, copies nothing and never waits.  Arguments are checked first (ORBX_E_ARG: a null pointer, a
 * negative count, a mode outside 0..2, a huber_delta or chi2_threshold that is not a number, a camera_model outside {0, 1};
 * ORBX_E_UNSUPPORTED: more than ORBI_MAX_JOBS groups, edges or states, more than ORBVI_MAX_STATES states for the solve); then the call
 * fails with ORBX_E_NO_DEVICE without a HIP device.  There is no CPU path.  d_result is 8 x int32, WRITTEN by every call.
 *
 * ---- orbvi_linearize_device: EdgeMonoOnlyPose on the states of an orbi_graph ----
 *
 * Edges come in n_groups groups; group g hangs on the pose of state d_group_state[g] and owns the edges [d_edge_off[g],
 * d_edge_off[g + 1]) of d_points[cap_edges][3] (mp->getPos()), d_edge_z[cap_edges][2] (kp.pt) and d_edge_inv_sigma2[cap_edges] (1 /
 * kp.size^2) -- for one group exactly what orbba_pose_edges_device (orbba.h) leaves in device memory.  d_active[cap_edges] (uint8, NULL =
 * every edge active): 0 is an edge at level 1 (Optimize.cpp:730).
 *
 * Distrust.  d_edge_off is a device array: every entry is read as clamped to [0, cap_edges] and then as the largest clamped entry
 * up to and including itself, so the ranges are inside the arrays, non-decreasing and disjoint; nothing is read or written past
 * cap_edges.  A group whose state lies outside [0, n_states) is dropped (ORBI_R_RANGE); a group whose state an EARLIER group of the
 * list names, dropped or not, is dropped (ORBI_R_DUPLICATE), so a pose block is written by one workgroup.  A dropped group writes
 * zeros to the d_err and d_chi2 of its edges, to its d_total and to its d_n_inliers; its d_active is not written.  The others are
 * counted in ORBI_R_DONE.  An edge whose error or chi2 is not finite (a point on the camera plane Z = 0) and that is active (mode
 * 2: every edge) is counted in ORBVI_R_NONFINITE; it adds nothing to H, b and the totals -- the reference would poison the system --
 * and its error and chi2 are written as computed.
 *
 * Arithmetic.  IEEE double throughout: +, -, *, / and the correctly rounded sqrt only for the Pinhole model (the Kannala-Brandt
 * model adds atan and atan2), no fused multiply-add, each expression read left to right, a 3-term product-sum as (p0 + p1) + p2,
 * Hat's zeros multiplied; the calibration's floats are widened.  tests/vi_model.py restates every line below in numpy.
 *   the pose    from the graph's (R_wb, t_wb) of the group's state on every call (CameraImuPose::update, G2oTypes.cpp:23-24):
 *                 R_cw = R_cb*R_wb^T, (R_cw)_ij = (rcb_i0*rwb_j0 + rcb_i1*rwb_j1) + rcb_i2*rwb_j2      t_cw = t_cb - R_cw*t_wb
 *               ONE CANONICALISATION: the reference's CameraImuPose(Tcw, Twb) keeps the frame's float T_cw until the first update
 *               and derives it from then on; here it is always derived (DESIGN.md records what that changes).
 *   the edge    Pc = R_cw*Pw + t_cw, (Pc)_i = ((r_i0*x + r_i1*y) + r_i2*z) + t_i;  e = z - project(Pc);  chi2 = inv_sigma2*(ex*ex +
 *               ey*ey).  project and getProjJacobian are csrc/orbba_camera.h, shared with orbba.hip: Pinhole u = fx*(X/Z) + cx,
 *               Jp = [fx/Z, 0, -fx*X/(Z*Z); 0, fy/Z, -fy*Y/(Z*Z)]; the Kannala-Brandt model as Fisheye.cpp:35-49, :83-108.
 *   Jacobian    R_bc = R_cb^T; t_bc = the FLOAT Pose::inverse of T_cb as ImuCalib holds it (Imu.h:52-54, Pose.cpp:12-14):
 *               (t_bc)_i = ((-rcb_0i)*t_0 + (-rcb_1i)*t_1) + (-rcb_2i)*t_2 in float, then widened.
 *                 Pb = R_bc*Pc + t_bc (the product-sum, then + t)          M = R_cb*Hat(Pb)
 *                 J[:, 0:3] = (-Jp)*M          J[:, 3:6] = (-Jp)*(-R_cb)          (each a product-sum over the negated factors)
 *   the form    Huber is the one of orbi.h (huber_delta > 0; chi2 > delta*delta: rho = (2*sqrt(chi2))*delta - delta*delta, w =
 *               delta/sqrt(chi2); else rho = chi2, w = 1).  W = w*inv_sigma2, WJ = W*J, We = (W*ex, W*ey).  The edge adds
 *               J_0a*WJ_0b + J_1a*WJ_1b to H_ab (a <= b; the lower triangle receives the same sums) and J_0a*We_0 + J_1a*We_1 to g_a.
 *   the sums    one workgroup of 1024 threads per group.  Thread t takes the group's edges t, t + 1024, ... in ascending order and
 *               adds each to its own 21 + 6 + 2 partial sums (H's upper triangle row by row, g, plain and robustified chi2),
 *               which start at zero and live in registers.  Each partial is then reduced over the wave by the butterfly v = v +
 *               v[lane ^ o] for o = 32, 16, 8, 4, 2, 1, and the sixteen wave results are added in ascending wave order, from zero.
 *               No floating-point atomics: the same input gives the same bytes.  A 1024-thread workgroup has 128 VGPRs per lane,
 *               which the 27 sums and the Kannala-Brandt Jacobian do not share: a thread makes three passes over its own edges
 *               (errors and weights; the Jacobian; the sums) through d_work, ORBVI_EDGE_WORK doubles per edge, the caller's (mode 0).
 * Modes.
 *   0   d_err[e][2] and d_chi2[e] of EVERY edge of the group, active or not.  The sums over the ACTIVE edges are ADDED to what
 *       d_H_diag[225*s ..][0:6, 0:6] (both triangles) holds and g is SUBTRACTED from d_b[15*s .. 15*s + 6), s the group's state:
 *       THE CALL ADDS, because it sits behind orbi_linearize_device on the stream, which writes these blocks; a caller with visual
 *       edges only clears them first.  Nothing else of d_H_diag and d_b is touched.  d_total[2g ..) = (plain, robustified) chi2
 *       of the group's active edges.  A group whose state has ORBI_FIX_POSE adds nothing to H and b (orbi.h's rule); its errors,
 *       chi2 and totals are written all the same.
 *   1   d_err, d_chi2 and d_total only: what a trial needs.  d_H_diag and d_b may be NULL and are not touched.
 *   2   the classification of Optimize.cpp:722-735: d_err and d_chi2 of every edge, then d_active[e] = !(chi2 > chi2_threshold),
 *       literally that comparison, so a chi2 that is not a number stays an inlier as in the reference; d_n_inliers[g] = their
 *       count.  d_active is then exactly the d_inlier orbba_pose_drop_outliers_device takes.  d_active is not read; d_total,
 *       d_H_diag and d_b may be NULL and are not touched.
 *
 * ---- orbvi_solve_device: the damped step ----
 *
 * Solves (H + lambda*I)*dx = b over the free dof of n_states <= ORBVI_MAX_STATES states.  H is the 15n x 15n matrix with d_H_diag[s]
 * at (s, s) and, for every edge e of d_edges in ascending order, d_H_off[e] ADDED at (i, j) and its transpose at (j, i) -- the
 * arrays orbi_linearize_device and the call above leave.  Only i, j and rec of an edge are read, under orbi.h's rule: i, j or rec
 * outside its range, or i == j: the block is skipped (ORBI_R_RANGE).  A dof that d_fixed fixes is an identity row and column with a
 * zero right-hand side, so its dx is exactly 0 and orbi_graph_oplus_device takes d_dx as it is.  *d_lambda, ONE double in device
 * memory so that a caller can chain trials, is added to every free diagonal entry: g2o's setLambda on a BlockSolverX with nothing
 * marginalised.
 *   Cholesky    L*L^T, dense, in double, in LDS, by one wave.  Columns ascend.  For column j: d = a_jj - s with s = the sum of
 *               l_jk*l_jk over k < j ascending from zero; d is the PIVOT; l_jj = sqrt(d), r_j = 1/l_jj (the column's one square root
 *               and one division); l_ij = (a_ij - s)*r_j with s = the sum of l_ik*l_jk over k < j ascending from zero.
 *   forward     y_i = (b_i - s)*r_i, s = the sum of l_ik*y_k over k < i ascending from zero.
 *   backward    x_i = (y_i - s)*r_i, s = the sum of l_ki*x_k over k > i DESCENDING from the last dof, from zero (the order in which
 *               the x_k become known).
 *   outputs     d_dx[n][15] = x.  d_out[0] = the sum over all dof j ascending from zero of dx_j*(lambda*dx_j + b_j): g2o's
 *               computeScale without its + 1e-3.  d_out[1] = the largest H_jj over the free dof before damping, 0 when none is
 *               larger: what computeLambdaInit multiplies by tau (orbba_lm_options.tau).  d_out[2] = the smallest pivot.
 *   refusal     a pivot <= 0 or not finite: ORBI_R_REFUSED is counted instead of ORBI_R_DONE, d_dx is all zero, d_out[0] = 0 and
 *               d_out[2] is that pivot.  g2o treats a failed solve as a rejected trial.
 *
 * Kernel resources (gfx950, VGPRs / scratch bytes / static LDS bytes; tests/test_vi_resources.py reads them from the ISA):
 *   k_vi_linearize 126 / 0 / 3952 B, k_vi_solve 81 / 0 / 30032 B, k_counters_clear 2 / 0 / 0 B.
 * Both calls are latency-bound (one group of a few hundred to 2000 edges; at most 60 unknowns): nothing here has been tuned for
 * throughput and no throughput claim is made.
 *
 * ---- the tracker's two loops, closed: include/orbvi_loop.h ----
 *
 * orbvi_pose_optimize_device runs the whole of poseFullOptimize / poseInertialOptimize as ONE kernel launch of one workgroup: the rounds,
 * g2o's Levenberg-Marquardt policy, push / pop and the classification, on the stage code of the two calls above and of
 * orbi_linearize_device / orbi_graph_oplus_device (csrc/orbvi_stages.h, which the staged kernels run as well), so that a linearisation,
 * a solve and an update inside the loop give the bytes of the staged calls.  Its contract, options and kernel resources are in
 * orbvi_loop.h, which includes this header; the chain is
 *   orbi_graph_init_device -> orbi_edge_information_device -> orbvi_pose_optimize_device -> orbi_graph_recover_device
 *   (-> orbba_pose_drop_outliers_device)
 * localFullBundleAdjustment's loop is closed by the host in orbwl.h (it waits once per trial); initializeIMU's loops are not in the product.
 * localInertialBundleAdjustment's loop is orbil_chain_optimize_device (orbil.h): one launch of one workgroup on the inertial stages of
 * csrc/orbvi_stages.h, with the solve of this header replaced by a walk along the band of its chain (up to 20 states).
 */
#ifndef ORBVI_H
#define ORBVI_H

#include "orbi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBVI_MAX_STATES 4         /* orbvi_solve_device: 60 unknowns (ORBX_E_UNSUPPORTED above) */
#define ORBVI_EDGE_WORK 16         /* doubles of workspace per edge (orbvi_linearize_device, mode 0) */
#define ORBVI_R_NONFINITE 4        /* d_result of orbvi_linearize_device: edges whose error or chi2 is not finite */

typedef struct orbvi_camera {      /* by value: the camera fields of orbba_pose_problem */
    double fx, fy, cx, cy;
    int32_t camera_model, pad;     /* 0 Pinhole, 1 Kannala-Brandt */
    double fisheye_k[4];
} orbvi_camera;

/* computeError, linearizeOplus and constructQuadraticForm of the EdgeMonoOnlyPose of n_groups groups (mode 0), their errors only
 * (mode 1), or their inlier classification (mode 2).  huber_delta: (double)sqrtf(5.991) in the reference, on through all four rounds
 * (the `iter == 2` test at Optimize.cpp:736 never fires); chi2_threshold: 5.991 (mode 2 only).  d_total [n_groups][2] (modes 0, 1);
 * d_H_diag [n_states][225], d_b [n_states][15] (mode 0, ADDED to); d_work [cap_edges][ORBVI_EDGE_WORK] (mode 0, scratch; NULL otherwise);
 * d_active, d_n_inliers [n_groups] (mode 2, written).  One launch, two when n_groups != 1. */
int orbvi_linearize_device(orbi_graph graph, orbi_calib calib, orbvi_camera camera, int n_groups, int cap_edges, const int32_t *d_group_state,
                           const int32_t *d_edge_off, const double *d_points, const double *d_edge_z, const double *d_edge_inv_sigma2,
                           uint8_t *d_active, double huber_delta, double chi2_threshold, int mode, double *d_work, double *d_err,
                           double *d_chi2, double *d_total, double *d_H_diag, double *d_b, int32_t *d_n_inliers, int32_t *d_result, void *stream);

/* The damped step.  d_fixed [n_states] (the graph's); d_edges / d_H_off [n_edges][225] may be NULL with n_edges == 0; cap: the size of
 * the record bank the edges' `rec` is held against; d_lambda [1]; d_dx [n_states][15]; d_out [3].  n_states >= 1.  One launch. */
int orbvi_solve_device(int n_states, const uint8_t *d_fixed, const orbi_edge *d_edges, int n_edges, int cap, const double *d_H_diag,
                       const double *d_H_off, const double *d_b, const double *d_lambda, double *d_dx, double *d_out, int32_t *d_result,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif
