/*
 * orbi.h -- IMU preintegration, the frame-pose prediction and the linearised inertial factors on the device (liborbx.so, gfx950).
 *
 * What the tracker does with the inertial samples of a frame once the mapper has initialised the IMU (reference
 * modules/Sensor/Imu.cpp:76-204, modules/BasicObject/Frame.cpp:57-88, KeyFrame.cpp:100-115, Tracking.cpp:90-91, :185-243):
 * integrate them into the PreIntegrator of the last frame and of the last key frame, predict the new frame's pose from one of
 * them, and hand that pose to the projection search.  Everything here lives in caller-owned DEVICE memory, so the chain
 *   orbi_integrate_device -> orbi_predict_device -> orbm_project_frame_device (orbm.h) -> the searches -> poseOptimize ->
 *   orbi_imu_pose_device
 * runs on one stream without a host hop.  Of the inertial optimisers of Optimize.cpp the per-iteration linearisation of their
 * inertial edges, bias walks and priors is here, with KeyFrame::setPrioriInformation ("Inertial factors linearised on the device"
 * below); their Levenberg-Marquardt loops are not.
 *
 * Every entry point is a handle-less `*_device` entry point under the one stream rule of orbx.h ("Streams and threads"): it
 * enqueues on exactly the `stream` it is given (a hipStream_t; NULL is stream 0 itself), allocates nothing and never waits on
 * the host.  Arguments are checked first (ORBX_E_ARG: a null pointer, a negative count, cap or cap_meas < 1; ORBX_E_UNSUPPORTED:
 * more than ORBI_MAX_JOBS jobs); then the call fails with ORBX_E_NO_DEVICE without a HIP device.  There is no CPU path.
 * Returns 0 or a negative ORBX_E_* code (orbx.h); text in orbx_last_error().
 *
 * State
 *   orbi_calib   by value: ImuCalib's T_cb (Rcb row-major, tcb), the diagonals of cov_noise and cov_walk (gyro x 3, acc x 3) and
 *                GRAVITY_VALUE (Imu.h:15).
 *   the bank     `cap` orbi_record in device memory, one per frame / key frame slot; a record is ORBI_RECORD_BYTES (1232, a
 *                multiple of 16) bytes.  A bias is (bg[3], ba[3]).  The reference's `information` and its per-object copies of the
 *                two covariances are not kept (the first belongs to setPrioriInformation, the others are the calibration's).
 *   the pool     cap x cap_meas x 7 floats: row `id` holds the (w[3], a[3], dt) triples that IntegrateNewMeasurement pushes to
 *                `measurements` (Imu.cpp:102), n_meas of them.
 *
 * Jobs.  A call works through a list of n <= ORBI_MAX_JOBS jobs held in device memory, one WAVE per job.  Ids are distrusted:
 *   - a job whose id (or second id: the `src` of a reset, the `next` of a merge; or sample range, for an integration) lies outside
 *     its range is dropped and counted in d_result[ORBI_R_RANGE];
 *   - a job j is dropped and counted in d_result[ORBI_R_DUPLICATE] when an EARLIER job j' < j of the list -- dropped or not --
 *     conflicts with it: id_j == id_j', or id_j == second_j', or second_j == id_j' (second ids >= 0 only).  Each wave finds this by
 *     scanning the jobs ahead of its own, so a record is written by at most one wave that nobody else reads, and no execution
 *     order reaches the output;
 *   - a job that would leave more than cap_meas measurements in its pool row is refused BEFORE it writes anything: record and pool
 *     row stay as passed, d_result[ORBI_R_REFUSED] counts it and d_result[ORBI_R_NEED] is the largest measurement count a refused
 *     job needed (the full count).  A record's n_meas outside [0, cap_meas] is read as clamped to that range.
 * d_result is 8 x int32, WRITTEN by every call (not accumulated); n = 0 is allowed and leaves eight zeros.
 *
 * Arithmetic.  Everything is float32 as in the reference, built from IEEE +, -, *, / and the correctly rounded sqrtf only, no
 * fused multiply-add; sinf / cosf are orb_sincosf (csrc/orb_math.h), which tests/test_oracle_kat.py pins to glibc on [0, 2*pi]:
 * |w * dt| beyond that range is outside the pinned range.  Eigen's summation orders cannot be pinned, so THIS HEADER FIXES EVERY
 * EVALUATION ORDER; tests/imu_model.py restates it in numpy and the device equals that model bit for bit.  Canonicalisations:
 *   - each of the reference's expressions is read left to right; a scalar in front of a product scales its first factor;
 *   - a 3x3 product is (A*B)_ij = (a_i0*b_0j + a_i1*b_1j) + a_i2*b_2j, a matrix-vector product likewise; Hatf's zeros ARE
 *     multiplied (the matrix is dense there); norm(x) = sqrtf((x0*x0 + x1*x1) + x2*x2);
 *   - IntegrateNewMeasurement(gyro, acc, dt), Imu.cpp:101-148, with w = gyro - bias.bg, a = acc - bias.ba, dt2 = dt*dt,
 *     Ra = dR*a, Ah = Hatf(a), RA = dR*Ah, RAJ = RA*JRg, all of the OLD dR, dV, JRg, JVg, JVa:
 *       dP  = (dP + dV*dt) + (0.5f*Ra)*dt2            dV  = dV + Ra*dt
 *       JPg = (JPg + JVg*dt) - (0.5f*RAJ)*dt2         JVg = JVg - RAJ*dt
 *       JPa = (JPa + JVa*dt) - (0.5f*dR)*dt2          JVa = JVa - dR*dt
 *       A10 = (-RA)*dt   A20 = (-(0.5f*RA))*dt2   A21 = dt*I   B11 = dR*dt   B21 = (0.5f*dR)*dt2
 *       dw = w*dt, d2 = (dw0*dw0 + dw1*dw1) + dw2*dw2, d = sqrtf(d2), W = Hatf(dw); the branch is (double)d < 1e-6:
 *         ExpSO3f            small: dE = (I + W) + (0.5f*W)*W        else: dE = (I + (sinf(d)/d)*W) + (((1 - cosf(d))/d2)*W)*W
 *         RightJacobianSO3f  small: Jr = I                            else: Jr = (I - ((1 - cosf(d))/d2)*W) + (((d - sinf(d))/(d2*d))*W)*W
 *         where ((s*W)*W)_ij = ((s*w_i0)*w_0j + (s*w_i1)*w_1j) + (s*w_i2)*w_2j
 *       dR  = NormalizeRotationf(dR*dE)                A00 = dE^T   B00 = Jr*dt
 *       C[0:9,0:9] = A*C*A^T + B*N*B^T from the 3x3 blocks, structural zeros and identities not multiplied and not added:
 *         T = A*C:    T_0b = A00*C_0b     T_1b = A10*C_0b + C_1b            T_2b = (A20*C_0b + dt*C_1b) + C_2b
 *         S = T*A^T:  S_a0 = T_a0*A00^T   S_a1 = T_a0*A10^T + T_a1          S_a2 = (T_a0*A20^T + T_a1*dt) + T_a2
 *         Q = B*N*B^T: (Q_ab)_ij = ((x_i0*n_0)*y_j0 + (x_i1*n_1)*y_j1) + (x_i2*n_2)*y_j2 with (x, y, n) =
 *                     Q_00: (B00, B00, gyro noise)   Q_11: (B11, B11, acc noise)   Q_12: (B11, B21, acc)   Q_21: (B21, B11, acc)
 *                     Q_22: (B21, B21, acc); the other four blocks of Q do not exist
 *         C_ab = S_ab + Q_ab where Q_ab exists, else S_ab
 *       C[9+i][9+i] += cov_walk[i], i < 6              JRg = dE^T*JRg - Jr*dt            delta_t += dt
 *   - NormalizeRotationf (LieAlgeBra.cpp:129-132) is the polar factor U*V^T of its argument.  The sequence here: two Newton steps
 *     X <- 0.5f*(X + cof(X)/det(X)) (X^-T = cof(X)/det(X)), with cof_ij = x_pq*x_rs - x_ps*x_rq for p = (i+1)%3, r = (i+2)%3,
 *     q = (j+1)%3, s = (j+2)%3, and det = (x_00*cof_00 + x_01*cof_01) + x_02*cof_02.  The argument is a product of two rotations
 *     that are orthogonal to a few ulps, and the iteration is quadratic: in a numpy float32 run |R^T R - I| stays <= 1.2e-7 after
 *     1000 samples.
 *   - the updated deltas of the prediction (Imu.cpp:194-204): dbg, dba = delta_bias;
 *       dRu = NormalizeRotationf(dR*ExpSO3f(JRg*dbg))   dVu = (dV + JVg*dbg) + JVa*dba   dPu = (dP + JPg*dbg) + JPa*dba
 *   - the prediction (Tracking.cpp:211-243), g = (0, 0, -gravity), dt = delta_t:
 *       Rwb2 = NormalizeRotationf(Rwb*dRu)   twb2 = ((twb + v*dt) + ((0.5f*g)*dt)*dt) + Rwb*dPu   v2 = (v + g*dt) + Rwb*dVu
 *   - Pose::inverse (Pose.cpp:12-14) is (R^T, (-(R^T))*t) and Pose::operator* (Pose.cpp:8-10) is (R1*R2, R1*t2 + t1):
 *       T_cw = T_cb * T_wb.inverse() (Frame.cpp:65-71)        T_wb = T_cw.inverse() * T_cb (Frame.cpp:57-63)
 *
 * Kernel resources (gfx950, VGPRs / scratch bytes / static LDS bytes; tests/test_imu_resources.py reads them from the ISA):
 *   k_imu<reset> 14 / 0 / 32 B, k_imu<integrate> 103 / 0 / 12368 B, k_imu<set_bias> 97 / 0 / 12368 B, k_imu<merge> 101 / 0 / 12368 B,
 *   k_imu_predict 26 / 0 / 688 B, k_imu_pose 8 / 0 / 124 B, k_counters_clear 2 / 0 / 0 B.
 * One wave per job, four waves per workgroup: the record, the 9x9 product's intermediate and the 3x3 temporaries live in the
 * wave's own part of LDS, the lanes are spread over matrix entries, and the phases of a sample are separated by wave-level
 * fences only -- no workgroup barrier inside the sample loop.
 *
 * ---- Inertial factors linearised on the device (declarations: orbi_factors.h, included at the end of this file) ----
 *
 * What poseInertialOptimize, poseFullOptimize, localInertialBundleAdjustment and localFullBundleAdjustment (Optimize.cpp:547-608,
 * :610-760, :960-1060, :1090-1250) do per iteration with their inertial edges, for a caller who keeps g2o's solver (orbba_linearize is
 * the same layer for the visual edges): computeError, linearizeOplus, the information matrices and constructQuadraticForm.  The loops
 * themselves, the visual edges in the IMU-pose parametrisation and the edges of the IMU initialisation are not here.  (Since then localInertialBundleAdjustment's
 * loop is orbil.h's, whole in one launch on the stage code of these calls, and the tracker's two are in the library as well.)  Same rules as
 * above: handle-less, one stream, no allocation, no host wait, arguments first (ORBX_E_ARG), then ORBX_E_NO_DEVICE, no CPU path,
 * d_result 8 x int32 written by every call.
 *
 * The graph (orbi_graph, by value; all arrays the caller's, in device memory)
 *   vertices   n_states states, each the estimates of one VertexPose and three Vertex3D in DOUBLE as g2o holds them: Rwb[n][9] (row-
 *              major), twb[n][3], v[n][3], bg[n][3], ba[n][3]; fixed[n] (uint8): ORBI_FIX_POSE / _VELO / _GYRO / _ACC = setFixed of that
 *              vertex, also "this state has no such vertex".
 *   dof        15 per state, [dphi, dt, dv, dbg, dba].  The pose part is CameraImuPose::update (G2oTypes.cpp:10-25): t_wb += R_wb*dt, then
 *              R_wb <- R_wb*ExpSO3(dphi), and NormalizeRotation after every third update (d_iter, the caller's counter per state).
 *   edges      orbi_edge {i, j, rec, flags}: EdgeInertial (G2oTypes.cpp:377-445) between states i (first) and j (second) with record
 *              `rec` of the bank; with both poses fixed it is EdgeInertialOnly (:309-356, the same residual and the same velocity and
 *              bias Jacobians).  The bias vertices it reads are state i's.  ORBI_EDGE_WALKS: the edge also carries the gyro and the acc
 *              EdgeBiasWalk between the bias vertices of i and j (Optimize.cpp:1019-1029, :1163-1170), e = b_j - b_i, J = (-I, +I).
 *   priors     orbi_prior per slot, floats as KeyFrame holds them; orbi_prior_job {state, prior, mask}: the EdgePriori3D of the
 *              state's velocity (ORBI_PRIOR_VELO), gyro bias (_GYRO) and acc bias (_ACC), e = priori - estimate, J = -I.  THE ACC
 *              PRIOR IS WEIGHTED WITH acc_info, as poseInertialOptimize does (Optimize.cpp:594); with ORBI_PRIOR_ACC_GYRO_INFO it is
 *              weighted with gyro_info, which is what localFullBundleAdjustment passes (Optimize.cpp:1189).  Two jobs naming one
 *              (state, bit) are both applied, as g2o would.
 *   distrust   an edge with i, j or rec outside its range, or i == j, and a prior job with its state or slot outside its range, is
 *              dropped and counted; its outputs are zero.
 *
 * Arithmetic.  The parts the reference computes in float are float, in this header's orders, bit for bit tests/imu_model.py: with
 * bgf, baf = the bias vertices of state i cast to float, dbg = bgf - bias.bg, dba = baf - bias.ba (Imu.cpp:182-192):
 *       dR = NormalizeRotationf(dR*ExpSO3f(JRg*dbg))   dV = (dV + JVg*dbg) + JVa*dba   dP = (dP + JPg*dbg) + JPa*dba
 * Everything behind the cast to double is IEEE double: +, -, *, / without fused multiply-add, the device's sqrt, sin, cos and atan2,
 * each expression read left to right, a 3x3 product summed as (p0 + p1) + p2, longer sums ascending from zero; LogSO3,
 * RightJacobianSO3 and InverseRightJacobianSO3 with their 1e-6 branches and the tr == 3 exit (LieAlgeBra.cpp:60-112); dt and g =
 * (0, 0, -gravity) are the floats widened; tests/factors_model.py restates it and the device is held to 1e-9 of it.
 *   information   d_info = (X + X^T)/2, X the general inverse of C[0:9,0:9] widened to double (Gauss-Jordan on [C | I], partial
 *              pivoting: the first row of the largest |entry|; the pivot row is divided by the pivot), NOT symmetrised first
 *              (G2oTypes.cpp:366-367).  The eigenvalue clamp behind it (:368-372) is omitted: the smallest eigenvalue is 7e6 .. 3e9
 *              on records of 2 .. 400 samples, against the threshold 1e-12 (tests/test_factors_cpu.py asserts the clamp is a no-op on
 *              every test record).  d_walk_info: the inverses of C[9:12,9:12] and C[12:15,12:15] by cofactors (adj/det).
 *   priors     orbi_prior_information_device, in double from the float C, stored as float: velo_info = V*diag(lambda)*V^T of the
 *              symmetrised C[3:6,3:6] by ORBI_JACOBI_SWEEPS cyclic Jacobi sweeps over the pairs (0,1), (0,2), (1,2) (theta = (a_qq -
 *              a_pp)/(2 a_pq), t = sgn(theta)/(|theta| + sqrt(theta^2 + 1)), c = 1/sqrt(t^2 + 1), s = t*c), eigenvalues < 1e-12 set to 0;
 *              gyro_info / acc_info by cofactors.
 *   the form   chi2 = e^T*Omega*e.  Huber (huber_delta > 0, inertial edges only; g2o's RobustKernelHuber as in orbba.h): chi2 >
 *              delta^2: rho = 2*sqrt(chi2)*delta - delta^2, w = delta/sqrt(chi2); else rho = chi2, w = 1.  H += J^T*(w*Omega)*J,
 *              b -= J^T*(w*Omega)*e with the columns of fixed dof removed from J, so that rows and columns of fixed dof are zero; chi2
 *              does not look at the fixed masks.  d_H_off[e] is the block (rows: state i, columns: state j) of edge e alone.  A
 *              diagonal block and b add up their contributions in ascending edge order (the edge's inertial part, then its walks),
 *              the prior jobs last in ascending order; d_total = (plain, robustified) adds up edges ascending, each as inertial, gyro
 *              walk, acc walk, then prior jobs ascending as velocity, gyro, acc.  No floating-point atomics: the same input gives the
 *              same bytes.
 *
 * Kernel resources (gfx950, VGPRs / scratch bytes / static LDS bytes; tests/test_factors_resources.py reads them from the ISA):
 *   k_fac_prior_info 103 / 0 / 32 B, k_fac_init 40 / 0 / 32 B, k_fac_edge_info 40 / 0 / 5792 B, k_fac_edge 81 / 0 / 28640 B,
 *   k_fac_gather 50 / 0 / 32 B, k_fac_oplus 70 / 0 / 32 B, k_fac_recover 38 / 0 / 32 B, k_counters_clear 2 / 0 / 0 B.
 * The graphs are tiny (2 states for the tracker, a few tens for a local window) and every call is latency-bound: nothing here has
 * been tuned for throughput and no throughput claim is made.  An inertial edge is one wave, four per workgroup (k_imu's shape), its
 * 9x30 Jacobian, the 9x9 information and their product in the wave's own LDS slice; a wave per state then gathers its edges in edge
 * order from the caller's workspace.  The float helpers come from csrc/orbi_so3.h, shared with orbi_imu.hip.
 */
#ifndef ORBI_H
#define ORBI_H

#include <stdint.h>

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBI_MAX_JOBS 4096     /* jobs per call (ORBX_E_UNSUPPORTED above) */
#define ORBI_RECORD_BYTES 1232

/* indices into d_result (8 x int32) */
#define ORBI_R_DONE 0          /* jobs carried out (a merge of a record with itself included) */
#define ORBI_R_RANGE 1         /* dropped: an id, second id or sample range outside its range */
#define ORBI_R_DUPLICATE 2     /* dropped: conflicts with an earlier job of the list */
#define ORBI_R_REFUSED 3       /* refused: the pool row would overflow; nothing of the job was written */
#define ORBI_R_NEED 4          /* the largest measurement count a refused job needed */
#define ORBI_R_REINTEGRATED 5  /* set_bias: jobs that re-integrated; merge: jobs that took the Reset branch */
#define ORBI_R_NOOP 6          /* merge: jobs with id == next */

typedef struct orbi_calib {
    float Rcb[9], tcb[3];      /* ImuCalib::T_cb, R row-major */
    float cov_noise[6];        /* diagonal: noiseGyro^2 x 3, noiseAcc^2 x 3 */
    float cov_walk[6];         /* diagonal: walkGyro^2 x 3, walkAcc^2 x 3 */
    float gravity;             /* GRAVITY_VALUE */
} orbi_calib;

typedef struct orbi_record {
    float bias[6], updated_bias[6], delta_bias[6]; /* (bg, ba) each */
    float delta_t;
    float dR[9], dV[3], dP[3];                     /* matrices row-major */
    float JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
    float C[225];                                  /* row-major 15 x 15 */
    int32_t n_meas;                                /* measurements in the record's pool row */
    int32_t pad[3];
} orbi_record;

typedef struct orbi_sample {   /* ImuData (Imu.h:18-24) */
    float w[3], a[3];
    double t;
} orbi_sample;

typedef struct orbi_job {      /* one computePreIntegration(imus, endTime) */
    int32_t id;                /* the record */
    int32_t first, count;      /* the samples d_samples[first .. first + count); two jobs may name the same range */
    int32_t pad;
    double timestamp;          /* of the frame / key frame the record belongs to */
    double end_time;
} orbi_job;

/* Reset(bias) and the three constructors (Imu.cpp:76-99) for the records d_ids[0..n): bias = the bias, updated_bias = bias,
 * delta_bias = 0, delta_t = 0, dR = I, everything else 0, n_meas = 0 (the pool row itself is not written).  The bias of job j:
 * d_src[j] >= 0 -- record d_src[j]'s updated_bias (the copy constructor of :90-93; d_src[j] == d_ids[j] is ReIntegrate's Reset);
 * d_src[j] == -1, or d_src == NULL -- d_bias[6j .. 6j+6), or zero when d_bias == NULL (the default constructor).  d_src[j] < -1 or
 * >= cap: dropped (ORBI_R_RANGE). */
int orbi_reset_device(orbi_record *d_bank, int cap, const int32_t *d_ids, const int32_t *d_src, const float *d_bias, int n,
                      int32_t *d_result, void *stream);

/* Frame::computePreIntegration / KeyFrame::computePreIntegration (Frame.cpp:73-88, KeyFrame.cpp:100-115) for n jobs.  The dt rule is
 * the reference's: startTime = timestamp + (double)delta_t of the record as passed; with count == 1 the one dt is end_time -
 * startTime; otherwise the first sample's is t[first + 1] - startTime, the last one's end_time - t[last], a middle one's t[i + 1] -
 * t[i]; all in double, each rounded to float once.  Then IntegrateNewMeasurement per sample, which also appends (w, a, dt) to the
 * record's pool row.  count == 0 integrates nothing.  A sample range outside [0, n_samples] is dropped (ORBI_R_RANGE). */
int orbi_integrate_device(orbi_calib calib, orbi_record *d_bank, float *d_pool, int cap, int cap_meas, const orbi_job *d_jobs, int n,
                          const orbi_sample *d_samples, int n_samples, int32_t *d_result, void *stream);

/* setNewBias (Imu.cpp:174-180) for the records d_ids[0..n) with the bias d_bias[6j .. 6j+6) each (the local inertial BA leaves a
 * different one per key frame, Optimize.cpp:1050-1052): updated_bias = the bias, delta_bias = updated_bias - bias, and ReIntegrate
 * (Imu.cpp:150-155) from the pool row when (double)norm(delta_bias.bg) > 0.01 -- compared in double, as the reference's literal makes
 * it.  The pool row and n_meas are unchanged by a re-integration. */
int orbi_set_bias_device(orbi_calib calib, orbi_record *d_bank, float *d_pool, int cap, int cap_meas, const int32_t *d_ids,
                         const float *d_bias, int n, int32_t *d_result, void *stream);

/* MergeNext (Imu.cpp:157-172) for Map::eraseKeyFrame behind orbm_cull_keyframes_device: record d_ids[j] takes in the measurements of
 * record d_next[j].  d_ids[j] == d_next[j] is the reference's no-op (ORBI_R_NOOP).  The sum of both n_meas is tested against
 * cap_meas before anything is reset or written.  (double)norm(delta_bias.bg) > 1e-5: Reset(updated_bias), then both lists in order;
 * otherwise the next record's list only.  The merged list is left in d_ids[j]'s pool row; record d_next[j] is only read. */
int orbi_merge_next_device(orbi_calib calib, orbi_record *d_bank, float *d_pool, int cap, int cap_meas, const int32_t *d_ids,
                           const int32_t *d_next, int n, int32_t *d_result, void *stream);

/* The one formula behind predictCurFramePose, predictCurFramePoseByKF and updateFrameIMU (Tracking.cpp:185-199, 211-243) with
 * setImuPoseAndVelocity behind it (Frame.cpp:65-71).  d_src: (Rwb[9], twb[3], v[3]) of the last frame / last key frame, 15 floats
 * in device memory; `id`: the record to predict with, in [0, cap) (a host value: ORBX_E_ARG outside).  d_dst receives the new
 * frame's 15 floats (it may be d_src).  d_pose_R[9] / d_pose_t[3] receive T_cw as doubles holding the float values -- exactly what
 * orbm_project_*_device and orbba_pose_optimize_batch_device take; both may be NULL (updateFrameIMU needs d_dst only).  One launch. */
int orbi_predict_device(orbi_calib calib, const orbi_record *d_bank, int cap, int id, const float *d_src, float *d_dst,
                        double *d_pose_R, double *d_pose_t, void *stream);

/* The other direction, Frame::setPose's T_wb = T_cw.inverse() * T_cb (Frame.cpp:57-63), from the doubles poseOptimize leaves,
 * rounded to float first: d_dst[0..12) receives (Rwb, twb); the velocity d_dst[12..15) is not touched.  This puts a visually
 * optimised frame's IMU pose where the next prediction reads it.  One launch. */
int orbi_imu_pose_device(orbi_calib calib, const double *d_pose_R, const double *d_pose_t, float *d_dst, void *stream);

#ifdef __cplusplus
}
#endif

/* ---- Inertial factors linearised on the device: the declarations (the text is above) ---- */
#include "orbi_factors.h"

#endif
