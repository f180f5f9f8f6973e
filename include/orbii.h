/*
 * orbii.h -- the steps of the IMU initialisation on the device (liborbx.so, gfx950).
 *
 * LocalMapping::initializeIMU (reference modules/Frontend/LocalMapping.cpp:374-482) is what takes a visual map into the inertial
 * steady state of orbi.h: a prior for the gravity direction and the velocities (:391-407), Optimize::inertialOptimize (modules/Backend/
 * Optimize.cpp:93-205: one velocity per key frame, ONE gyro and ONE accelerometer bias, the gravity direction and, the first time, the
 * scale of the map), its recovery into the key frames (:186-204) and Map::applyScaleRotation (orbm.h, "The map rescaled and rotated on
 * the device").  This header has the prior, the graph, the stages of ONE Levenberg-Marquardt iteration of inertialOptimize and the
 * recovery, for a caller whose pose table, state rows, record bank and prior slots live in device memory.  The solve of the damped system
 * is the ordered Cholesky for N <= 480 that the library already has (INTEGRATION.md names the call and spells the chain out); THE LOOP
 * ITSELF IS NOT HERE: the accept / reject decision of a trial is the caller's, who reads two scalars back per trial.
 * fullInertialOptimize and gravityOptimize are not here either.  (localInertialBundleAdjustment, the mapper's other optimiser on inertial
 * edges alone, is whole in the library, loop included: orbil.h.)
 *
 * Rules: those of orbi.h.  Handle-less `*_device` entry points, one stream (NULL is stream 0 itself), nothing allocated, no host wait.
 * Arguments are checked first (ORBX_E_ARG: a null pointer, a negative or zero capacity, fewer than two key frames, a kind or mode that
 * does not exist; then ORBX_E_UNSUPPORTED: more than ORBII_MAX_KF key frames), then the call fails with ORBX_E_NO_DEVICE without a HIP
 * device.  There is no CPU path.  d_result is 8 x int32, WRITTEN by every call, indexed by orbi.h's ORBI_R_*.  Ids held in device memory
 * are distrusted: dropped and counted, never dereferenced out of range.
 *
 * Jobs.  The key frames of the map, OLDEST FIRST (Map::getAllKeyFrames), as n_kf jobs d_jobs[4k .. 4k+4) = (row of the pose table, row of
 * the 15-float state array (Rwb[9], twb[3], v[3]), record of the orbi_record bank, orbi_prior slot).  The same list serves the prior, the
 * graph and the recovery; key frame k of the graph IS job k.  The record of a key frame is the PreIntegrator from it to the NEXT one
 * (KeyFrame::pre_integrator of the earlier key frame is the one every edge takes, Optimize.cpp:158, :167), so the last job's record is
 * read by nobody and may be -1.
 *
 * The graph (orbii_graph, by value; every array the caller's, in device memory)
 *   v [n_kf][3]    the Vertex3D velocities, double
 *   shared [16]    bg[3], ba[3] (the two bias Vertex3D), Rwg[9] row-major (VertexGravity), scale[1] (VertexScale; stays as set for kind G)
 *   iter [1]       int32: GravityDirection's update counter (G2oTypes.h:80-87)
 *   Rwb [n_kf][9], twb [n_kf][3], Oc [n_kf][3], Pcb [n_kf][3]   the constants of the edges, from the key frames' FLOAT T_cw and T_wb widened
 *                  (CameraImuPose(kf->getPose(), kf->getImuPose())); Oc = -R_cw^T t_cw and Pcb = R_cw^T t_cb in double (G2oTypes.cpp:81-82)
 * A TRIAL'S PUSH AND POP ARE COPIES OF v, shared AND iter: nothing else of the graph changes during an optimisation.
 *
 * The system is dense.  dof order [bg 0..2, ba 3..5, gravity 6..7, scale 8, v_k at 9 + 3k]; N = ORBII_N(n_kf) = 15 * ceil((9 + 3 n_kf) / 15),
 * so ORBII_MAX_KF = 157 gives N = 480.  Every dof at or beyond 9 + 3 n_kf, and dof 8 for kind G (which has no scale vertex), is an identity
 * row and column of d_H with a zero in d_b and takes no damping: its step is exactly zero.  d_H [N][N] row-major holds both triangles,
 * d_b [N]; the damped copy (d_S, d_rhs) with d_b read as [N / 15][15] and *d_lambda in device memory is what the ordered Cholesky takes,
 * and its d_dx [N] is what orbii_oplus_device takes.
 *
 * Arithmetic.  The float parts are the float code of csrc/orbi_so3.h in orbi.h's orders, bit for bit tests/imu_model.py; behind the cast
 * everything is IEEE double, +, -, *, / without fused multiply-add, the device's sqrt, sin, cos, atan2, asin and exp, each expression read
 * left to right, a 3x3 product or matrix-vector product summed as (p0 + p1) + p2, longer sums ascending from zero.  tests/imu_init_model.py
 * restates this header in numpy; the float outputs equal it bit for bit where only +, -, *, / and the shared float SO(3) code are
 * involved, the doubles are held to 1e-9 of it.
 *   the prior (LocalMapping.cpp:391-407), float.  Over the jobs that are not dropped, in order (a dropped job is taken out of the chain):
 *       O_k = (-(R_cw^T))*t_cw of pose row k rounded to float (KeyFrame.cpp:30);  dVu_k = (dV + JVg*dbg) + JVa*dba of the record (orbi.h);
 *       for every key frame k with a successor k':  dir = dir - Rwb_k*dVu_k (from zero, ascending: the sum is sequential),
 *       velo_k = (O_k' - O_k) / delta_t_k componentwise; v_k = velo_k, and the LAST key frame takes its predecessor's velo (:398-399).
 *       Every v is written to the state row [12..15) and to velo_priori of the prior slot (KeyFrame::setVelocity).
 *       n = sqrtf((dir0*dir0 + dir1*dir1) + dir2*dir2), dir = dir / n componentwise (left as it is when n == 0, Eigen's normalize);
 *       v = gI x dir with gI = (0, 0, -1), its zero terms dropped: v = (dir1, -dir0, 0);  nv = sqrtf((v0*v0 + v1*v1) + v2*v2);
 *       theta = (float)asin((double)nv) -- the reference's unqualified asin;  w = (theta*v) / nv;  Rwg = ExpSO3f(w), orbi.h's (NOT
 *       normalised: LieAlgeBra.cpp:47-58), stored as 9 doubles holding the floats.
 *       nv == 0 (gravity already along -z, or no usable pair): the reference divides by zero; here Rwg = I and ORBI_R_REFUSED counts
 *       it -- a stated canonicalisation.  The velocities are written all the same.
 *   an edge (G2oTypes.cpp:94-163 EdgeInertialGS, kind 0; :186-246 EdgeInertialG, kind 1) links key frames e and e + 1 with record
 *       d_edges[e].rec.  (dR, dV, dP) = getDeltaRotation / Velocity / Position of (bg, ba) CAST TO FLOAT, orbi.h's float code, widened;
 *       dbg = the float bg - bias.bg widened; G, dt = the floats widened; s = scale; g = Rwg*(0, 0, -G) with the zero terms dropped:
 *       g_i = Rwg_i2*(-G);  Rb1w = Rwb_e^T;  eR = (dR^T*Rb1w)*Rwb_e+1;  er = LogSO3(eR);
 *       kind 0:  ev = Rb1w*(s*(v2 - v1) - g*dt) - dV
 *                ep = Rb1w*(((((s*Oc2 + Pcb2) - s*Oc1) - Pcb1) - (s*v1)*dt) - ((0.5*g)*dt)*dt) - dP
 *       kind 1:  ev = Rb1w*((v2 - v1) - g*dt) - dV          ep = Rb1w*(((twb2 - twb1) - v1*dt) - ((0.5*g)*dt)*dt) - dP
 *       The Jacobian, 9 x 15 in the LOCAL order [v1 0..2, bg 3..5, ba 6..8, v2 9..11, gravity 12..13, scale 14], rows (er, ev, ep); blocks
 *       not named are zero.  JG (3 x 2) = Rwg*gm with gm(0,1) = -G, gm(1,0) = G, zero terms dropped: JG_i0 = Rwg_i1*G, JG_i1 = Rwg_i0*(-G).
 *         v1       kind 0: ev (-s)*Rb1w, ep ((-s)*dt)*Rb1w                 kind 1: ev -Rb1w, ep (-dt)*Rb1w
 *         bg       er (((-invJr)*eR^T)*Jr)*JRg with invJr = InverseRightJacobianSO3(er), Jr = RightJacobianSO3(JRg*dbg); ev -JVg; ep -JPg
 *         ba       ev -JVa; ep -JPa for kind 0.  KIND 1 HAS -JPg THERE: EdgeInertialG::linearizeOplus writes -JPg where -JPa belongs
 *                  (G2oTypes.cpp:236), and this header restates it as written
 *         v2       kind 0: ev s*Rb1w                                       kind 1: ev Rb1w
 *         gravity  ev ((-Rb1w)*JG)*dt; ep (c*Rb1w)*JG with c = ((-0.5)*dt)*dt
 *         scale    kind 0 only: ev (s*Rb1w)*(v2 - v1); ep (s*Rb1w)*((Oc2 - Oc1) - v1*dt)
 *       Omega = d_info[81e ..), what orbi_edge_information_device leaves for an orbi_edge list of which only `rec` is read: it IS this
 *       edge's information (G2oTypes.cpp:84-91 equals :361-372), eigenvalue clamp omitted as there.  There is no robust kernel.
 *       We = Omega*e, chi2 = e^T*We, WJ = Omega*J, M = J^T*WJ (15 x 15), r = -(J^T*We), every sum over k = 0..8 ascending from zero.
 *   the priors (Optimize.cpp:121-129): two EdgePriori3D, e = initial_bias - estimate with the float initial bias widened, Omega =
 *       (double)priori_g * I and (double)priori_a * I: chi2 = ((e0*(w*e0) + e1*(w*e1)) + e2*(w*e2)), H_dd += w, b_d += w*e_d.
 *   the form.  Every entry of d_H and d_b is the sum, from zero, of its edges' contributions in ASCENDING EDGE ORDER, the prior last.  No
 *       floating-point atomics: the same input gives the same bytes.  d_total[0] = the edges' chi2 ascending from zero, then the gyro
 *       prior's, then the accelerometer prior's.
 *   oplus (G2oTypes.h:80-87, :185-205, Vertex3D): bg, ba, v_k += their dx;  Rwg = Rwg*ExpSO3(dx6, dx7, 0) -- ExpSO3 normalises its result
 *       (orbi.h's double Newton sequence) --, iter += 1, and at iter == 3 Rwg = NormalizeRotation(Rwg), iter = 0;  kind 0: scale =
 *       scale*exp(dx8).
 *
 * Kernel resources (gfx950, VGPRs / scratch bytes / static LDS bytes; tests/test_imu_init_resources.py reads them from the ISA):
 *   k_ii_prior 68 / 0 / 5748 B, k_ii_init 46 / 0 / 256 B, k_ii_edge 65 / 0 / 20608 B, k_ii_assemble 34 / 0 / 0 B, k_ii_damp 9 / 0 / 0 B,
 *   k_ii_oplus 60 / 0 / 0 B, k_ii_recover 16 / 0 / 256 B.
 * Every call is latency-bound (at most 157 key frames and 480 unknowns): nothing here has been tuned for throughput and no throughput
 * claim is made.  An edge is one wave, four per workgroup (k_fac_edge's shape): the 9 x 15 Jacobian, Omega*J and their product live in
 * the wave's own slice of LDS and the edge leaves a 15 x 15 block and a 15-vector in the caller's workspace; a thread per entry of d_H then
 * adds up the entry's edges in edge order.
 */
#ifndef ORBII_H
#define ORBII_H

#include <stdint.h>

#include "orbi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBII_MAX_KF 157           /* key frames of one initialisation: N = 480 (ORBX_E_UNSUPPORTED above) */
#define ORBII_N(n_kf) (15 * ((9 + 3 * (n_kf) + 14) / 15))
#define ORBII_EDGE_WORK 240        /* doubles of workspace per edge: M (225), r (15) */
#define ORBII_KIND_GS 0            /* EdgeInertialGS: be_first, the scale is a vertex */
#define ORBII_KIND_G 1             /* EdgeInertialG */
#define ORBII_SHARED_BG 0          /* offsets into orbii_graph.shared */
#define ORBII_SHARED_BA 3
#define ORBII_SHARED_RWG 6
#define ORBII_SHARED_SCALE 15
#define ORBII_SUMMARY 10           /* floats of orbii_recover_device's d_summary: Rwg[9], scale */

typedef struct orbii_bias {        /* ImuCalib::initial_bias */
    float bg[3], ba[3];
} orbii_bias;

typedef struct orbii_graph {       /* by value: all device memory */
    double *v;                     /* [n_kf][3] */
    double *shared;                /* [16] bg, ba, Rwg, scale */
    int32_t *iter;                 /* [1] */
    double *Rwb, *twb, *Oc, *Pcb;  /* [n_kf][9], [n_kf][3] x 3: constants */
    int32_t n_kf, pad;
} orbii_graph;

/* The prior (LocalMapping.cpp:391-407) for n jobs.  d_pose_R [n_pose][9] / d_pose_t [n_pose][3]: the key-frame table's T_cw, doubles
 * holding floats, rounded to float first.  Writes d_state[15*row + 12 ..) and d_priors[slot].velo_priori of every job kept and d_Rwg [9].
 * Dropped and counted: ORBI_R_RANGE -- a pose row, state row or prior slot outside its range, a record outside [0, cap) (the LAST job's
 * may also be -1); ORBI_R_DUPLICATE -- a state row or a prior slot that an earlier job of the list names, dropped or not.  ORBI_R_DONE:
 * the jobs kept.  ORBI_R_REFUSED: 1 when nv == 0.  One launch of one wave. */
int orbii_prior_device(const double *d_pose_R, const double *d_pose_t, int n_pose, float *d_state, int n_src, const orbi_record *d_bank,
                       int cap, orbi_prior *d_priors, int n_priors, const int32_t *d_jobs, int n, double *d_Rwg, int32_t *d_result,
                       void *stream);

/* The vertices and the edges' constants (Optimize.cpp:110-153) from the graph.n_kf jobs: v_k = d_state[15*row + 12 ..) widened, (Rwb, twb)_k
 * = d_state[15*row ..) widened, Oc_k and Pcb_k from pose row k and calib.tcb; bg, ba = initial_bias widened; Rwg = d_Rwg[9], the identity
 * when d_Rwg == NULL (the branch imu_state != NOT_INITIALIZE); scale; iter = 0.  Only the pose row and the state row of a job are read.
 * A job with one of them outside its range is dropped (ORBI_R_RANGE): its key frame is v = twb = Oc = Pcb = 0, Rwb = I. */
int orbii_graph_init_device(orbii_graph graph, orbi_calib calib, const double *d_pose_R, const double *d_pose_t, int n_pose,
                            const float *d_state, int n_src, const int32_t *d_jobs, orbii_bias initial_bias, const double *d_Rwg,
                            double scale, int32_t *d_result, void *stream);

/* computeError, linearizeOplus and constructQuadraticForm of the graph.n_kf - 1 edges and the two priors.  d_edges [n_kf - 1]: only `rec` is
 * read; d_info [n_kf - 1][81].  kind: ORBII_KIND_GS / _G.  mode 0: d_err [n_kf - 1][9], d_chi2 [n_kf - 1], d_chi2_prior [2], d_total [1],
 * the undamped d_H [N][N] and d_b [N]; mode 1: errors, chi2 and total only -- d_H and d_b are neither read nor written and may be NULL.
 * d_work: (n_kf - 1) x ORBII_EDGE_WORK doubles of scratch, the caller's, both modes.  d_float [n_kf - 1][15] (the float dR, dV, dP) may be
 * NULL.  An edge whose rec is outside [0, cap) (ORBI_R_RANGE) or whose d_info block starts with a zero, what a refused information
 * leaves (ORBI_R_REFUSED), takes no part: its outputs are zero.  ORBI_R_DONE: the edges that took part.  Two launches. */
int orbii_linearize_device(orbii_graph graph, const orbi_record *d_bank, int cap, float gravity, const orbi_edge *d_edges,
                           const double *d_info, orbii_bias initial_bias, float priori_g, float priori_a, int kind, int mode, double *d_work,
                           double *d_err, double *d_chi2, double *d_chi2_prior, double *d_total, double *d_H, double *d_b, float *d_float,
                           int32_t *d_result, void *stream);

/* The damped system of a trial: d_S [N][N] = d_H with *d_lambda added to every FREE diagonal entry (dof < 9 + 3 n_kf, without dof 8 for
 * kind 1), d_rhs [N] = d_b.  d_out[1] = the largest undamped free diagonal entry, 0 when none is larger: what computeLambdaInit
 * multiplies by tau when priori_g == 0; d_out[0] and d_out[2] are not touched (the solve writes them).  d_H and d_b are only read, so a
 * rejected trial damps again without linearising again.  ORBI_R_DONE = 1.  One launch. */
int orbii_damp_device(int n_kf, int kind, const double *d_H, const double *d_b, const double *d_lambda, double *d_S, double *d_rhs,
                      double *d_out, int32_t *d_result, void *stream);

/* oplusImpl of the four kinds of vertex with the solve's d_dx [N] as it is.  ORBI_R_DONE = the vertices moved (n_kf + 3, + 1 for kind 0).
 * One launch. */
int orbii_oplus_device(orbii_graph graph, int kind, const double *d_dx, int32_t *d_result, void *stream);

/* Step 4 (Optimize.cpp:186-204) for the graph.n_kf jobs: v_k rounded to float into d_state[15*row + 12 ..) and d_priors[slot].velo_priori;
 * d_bias [n_kf][6] = (bg, ba) rounded to float IN EVERY ROW, the array orbi_set_bias_device takes; d_summary [ORBII_SUMMARY] = Rwg rounded
 * to float, then (float)scale -- what orbm_apply_scale_rotation_device reads.  The rest of step 4 is existing calls.
 * Only the state row and the prior slot of a job are read; outside its range: ORBI_R_RANGE; named by an earlier job, dropped or not:
 * ORBI_R_DUPLICATE; neither row nor slot of such a job is written.  One launch. */
int orbii_recover_device(orbii_graph graph, const int32_t *d_jobs, float *d_state, int n_src, orbi_prior *d_priors, int n_priors,
                         float *d_bias, float *d_summary, int32_t *d_result, void *stream);

#ifdef __cplusplus
}
#endif
#endif
