// IMU preintegration and the frame-pose prediction on the device (include/orbi.h):
//   orbi_reset_device        PreIntegrator's constructors and Reset                    Imu.cpp:76-99
//   orbi_integrate_device    Frame / KeyFrame::computePreIntegration                   Frame.cpp:73-88, Imu.cpp:101-148
//   orbi_set_bias_device     setNewBias with ReIntegrate                               Imu.cpp:150-155, 174-180
//   orbi_merge_next_device   MergeNext                                                 Imu.cpp:157-172
//   orbi_predict_device      predictCurFramePose[ByKF], updateFrameIMU                 Tracking.cpp:185-243, Frame.cpp:65-71
//   orbi_imu_pose_device     Frame::setPose's T_wb                                     Frame.cpp:57-63
//
// Every evaluation order is the header's (float; +, -, *, / through the ORB_F* wrappers, no fused multiply-add: the build passes
// -ffp-contract=off and the pragma below repeats it here; sqrtf is the correctly rounded one, sinf / cosf are orb_sincosf).
// WSYNC and the float helpers (the 3x3 products, ExpSO3f, RightJacobianSO3f, the Newton step) are orbi_so3.h's, shared with orbi_factors.hip.
//
// Shape: the sample loop is sequential and a sample is small and dense, so a job is ONE WAVE, four jobs per workgroup (k_refresh's
// shape).  The record, the 9x9 product's intermediate T and the 3x3 temporaries live in the wave's own slice of LDS.  A sample is
// five phases; in each, the lanes are spread over matrix entries -- seven groups of nine lanes, one 3x3 each, and all 64 lanes over
// the 81 entries of T and of C -- and every phase is  read + compute -> WSYNC -> write -> WSYNC, so an in-place update never meets a
// lane that still reads the old value.  WSYNC is a wavefront-scope fence and a wave barrier: the LDS pipe serves a wave's
// instructions in order, the fence keeps the compiler from moving them.  No workgroup barrier inside the sample loop: the two
// __syncthreads of k_imu fence the calibration's copy in LDS and the workgroup's counters, before and after all of it.
// Samples are staged 32 at a time (plus the one whose time stamp the last dt needs) so that the loop never waits for global memory.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "../../include/orbi.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orb_math.h"
#include "orbi_so3.h"

#pragma clang fp contract(off)

static_assert(sizeof(orbi_record) == ORBI_RECORD_BYTES && ORBI_RECORD_BYTES % 16 == 0, "orbi.h fixes the record's layout");
static_assert(sizeof(orbi_sample) == 32 && sizeof(orbi_job) == 32 && sizeof(orbi_calib) == 100, "orbi.h fixes these layouts");

namespace {

// ---- a wave's slice of LDS: the record's floats as orbi_record lays them out, then the temporaries -------------------------------
enum {
    F_BIAS = 0, F_UPD = 6, F_DELTA = 12, F_DT = 18, F_DR = 19, F_DV = 28, F_DP = 31, F_JRG = 34, F_JVG = 43, F_JVA = 52, F_JPG = 61,
    F_JPA = 70, F_C = 79, F_NMEAS = 304,                  // == offsetof(orbi_record, ...) / 4
    L_T = 304, L_W = 385, L_AH = 394, L_RA = 403, L_RAJ = 412, L_DE = 421, L_JR = 430, L_M = 439, L_M2 = 448, L_A10 = 457, L_A20 = 466,
    L_B00 = 475, L_B11 = 484, L_B21 = 493, L_STAGE = 504, // the staged samples: 33 x 8 words, 16-byte aligned
    L_WORDS = L_STAGE + 33 * 8
};
static_assert(offsetof(orbi_record, C) == 4 * F_C && offsetof(orbi_record, n_meas) == 4 * F_NMEAS && offsetof(orbi_record, JPa) == 4 * F_JPA,
              "the LDS image is the record");
enum { CAL_NG = 0, CAL_NA = 3, CAL_WALK = 6, CAL_WORDS = 12 };
constexpr int IMU_WAVES = 4, IMU_T = 64 * IMU_WAVES, STAGE = 32;

// IntegrateNewMeasurement(gyro, acc, dt) on the wave's record S (Imu.cpp:101-148, include/orbi.h).  Lane-uniform arguments.
__device__ __forceinline__ void integrate_sample(float *S, const float *cal, int lane, float gx, float gy, float gz, float cx, float cy,
                                                 float cz, float dt)
{
    const int g = lane / 9, e = lane - 9 * g, i = e / 3, j = e - 3 * i;
    const float *dR = S + F_DR;
    const float wx = sub(gx, S[F_BIAS]), wy = sub(gy, S[F_BIAS + 1]), wz = sub(gz, S[F_BIAS + 2]);
    const float a[3] = {sub(cx, S[F_BIAS + 3]), sub(cy, S[F_BIAS + 4]), sub(cz, S[F_BIAS + 5])};
    const float dt2 = mul(dt, dt);
    const float dwx = mul(wx, dt), dwy = mul(wy, dt), dwz = mul(wz, dt);
    const So3 so = so3_scalars(dwx, dwy, dwz);
    // phase 1: the two hat matrices
    if (g == 0) S[L_W + e] = hat(dwx, dwy, dwz, e);
    if (g == 1) S[L_AH + e] = hat(a[0], a[1], a[2], e);
    WSYNC();
    // phase 2: everything that needs the old dR only
    float v0 = 0.f, v1 = 0.f;
    if (g == 0) v0 = m3(dR, S + L_AH, i, j);
    else if (g == 1) v0 = exp_entry(so, S + L_W, e);
    else if (g == 2) v0 = rightj_entry(so, S + L_W, e);
    else if (g == 3) v0 = mul(dR[e], dt);
    else if (g == 4) v0 = mul(mul(0.5f, dR[e]), dt2);
    else if (g == 5 && e < 3) {
        const float Ra = sum3(mul(dR[3 * e], a[0]), mul(dR[3 * e + 1], a[1]), mul(dR[3 * e + 2], a[2]));
        v0 = add(add(S[F_DP + e], mul(S[F_DV + e], dt)), mul(mul(0.5f, Ra), dt2));
        v1 = add(S[F_DV + e], mul(Ra, dt));
    } else if (g == 6) {
        v0 = sub(add(S[F_JPA + e], mul(S[F_JVA + e], dt)), mul(mul(0.5f, dR[e]), dt2));
        v1 = sub(S[F_JVA + e], mul(dR[e], dt));
    }
    WSYNC();
    if (g == 0) S[L_RA + e] = v0;
    else if (g == 1) S[L_DE + e] = v0;
    else if (g == 2) S[L_JR + e] = v0;
    else if (g == 3) S[L_B11 + e] = v0;
    else if (g == 4) S[L_B21 + e] = v0;
    else if (g == 5 && e < 3) S[F_DP + e] = v0, S[F_DV + e] = v1;
    else if (g == 6) S[F_JPA + e] = v0, S[F_JVA + e] = v1;
    WSYNC();
    // phase 3
    if (g == 0) v0 = m3(S + L_RA, S + F_JRG, i, j);
    else if (g == 1) v0 = m3(dR, S + L_DE, i, j);
    else if (g == 2) v0 = mul(-S[L_RA + e], dt);
    else if (g == 3) v0 = mul(-mul(0.5f, S[L_RA + e]), dt2);
    else if (g == 4) v0 = mul(S[L_JR + e], dt);
    WSYNC();
    if (g == 0) S[L_RAJ + e] = v0;
    else if (g == 1) S[L_M + e] = v0;
    else if (g == 2) S[L_A10 + e] = v0;
    else if (g == 3) S[L_A20 + e] = v0;
    else if (g == 4) S[L_B00 + e] = v0;
    WSYNC();
    // phase 4: the Jacobians that need RAJ, the first Newton step, JRg, and T = A*C
    if (g == 0) {
        v0 = sub(add(S[F_JPG + e], mul(S[F_JVG + e], dt)), mul(mul(0.5f, S[L_RAJ + e]), dt2));
        v1 = sub(S[F_JVG + e], mul(S[L_RAJ + e], dt));
    } else if (g == 1) v0 = newton_entry(S + L_M, i, j);
    else if (g == 2) v0 = sub(m3t(S + L_DE, S + F_JRG, i, j), mul(S[L_JR + e], dt));
    float t[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int x = lane + 64 * h;
        if (x < 81) {
            const int r = x / 9, c = x - 9 * r, ab = r / 3, ii = r - 3 * ab;
            const float *C = S + F_C + c;    // column c of the 9x9 block: C[15 * k]
            if (ab == 0) t[h] = sum3(mul(S[L_DE + ii], C[0]), mul(S[L_DE + 3 + ii], C[15]), mul(S[L_DE + 6 + ii], C[30]));
            else {
                const float *A = S + (ab == 1 ? L_A10 : L_A20) + 3 * ii;
                const float p = sum3(mul(A[0], C[0]), mul(A[1], C[15]), mul(A[2], C[30]));
                t[h] = ab == 1 ? add(p, C[15 * (3 + ii)]) : add(add(p, mul(dt, C[15 * (3 + ii)])), C[15 * (6 + ii)]);
            }
        }
    }
    WSYNC();
    if (g == 0) S[F_JPG + e] = v0, S[F_JVG + e] = v1;
    else if (g == 1) S[L_M2 + e] = v0;
    else if (g == 2) S[F_JRG + e] = v0;
    S[L_T + lane] = t[0];
    if (lane + 64 < 81) S[L_T + lane + 64] = t[1];
    WSYNC();
    // phase 5: the second Newton step, the walk, delta_t, and C = T*A^T + B*N*B^T
    if (g == 1) v0 = newton_entry(S + L_M2, i, j);
    else if (g == 3 && e < 6) v0 = add(S[F_C + 16 * (9 + e)], cal[CAL_WALK + e]);
    else if (g == 4 && e == 0) v0 = add(S[F_DT], dt);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int x = lane + 64 * h;
        if (x < 81) {
            const int r = x / 9, c = x - 9 * r, ab = r / 3, ii = r - 3 * ab, bb = c / 3, jj = c - 3 * bb;
            const float *T = S + L_T + 9 * r;
            float s;
            if (bb == 0) s = sum3(mul(T[0], S[L_DE + jj]), mul(T[1], S[L_DE + 3 + jj]), mul(T[2], S[L_DE + 6 + jj]));
            else {
                const float *A = S + (bb == 1 ? L_A10 : L_A20) + 3 * jj;
                const float p = sum3(mul(T[0], A[0]), mul(T[1], A[1]), mul(T[2], A[2]));
                s = bb == 1 ? add(p, T[3 + jj]) : add(add(p, mul(T[3 + jj], dt)), T[6 + jj]);
            }
            if ((ab == 0) == (bb == 0)) {   // Q_00, Q_11, Q_12, Q_21, Q_22
                const float *X = S + (ab == 0 ? L_B00 : ab == 1 ? L_B11 : L_B21) + 3 * ii;
                const float *Y = S + (bb == 0 ? L_B00 : bb == 1 ? L_B11 : L_B21) + 3 * jj;
                const float *N = cal + (ab == 0 ? CAL_NG : CAL_NA);
                s = add(s, sum3(mul(mul(X[0], N[0]), Y[0]), mul(mul(X[1], N[1]), Y[1]), mul(mul(X[2], N[2]), Y[2])));
            }
            t[h] = s;
        }
    }
    WSYNC();
    if (g == 1) S[F_DR + e] = v0;
    else if (g == 3 && e < 6) S[F_C + 16 * (9 + e)] = v0;
    else if (g == 4 && e == 0) S[F_DT] = v0;
    {
        const int r = lane / 9, c = lane - 9 * r;
        S[F_C + 15 * r + c] = t[0];
        if (lane + 64 < 81) {
            const int x = lane + 64, r1 = x / 9, c1 = x - 9 * r1;
            S[F_C + 15 * r1 + c1] = t[1];
        }
    }
    WSYNC();
}

// reset() with bias = updated_bias = b (Imu.h:137-146) on the LDS image, lane k < 6 holding b[k]; the caller syncs
__device__ __forceinline__ void reset_image(float *S, int lane, float b_lane)
{
    for (int k = lane; k < F_NMEAS; k += 64) S[k] = (k == F_DR || k == F_DR + 4 || k == F_DR + 8) ? 1.f : 0.f;
    WSYNC();
    if (lane < 6) S[F_BIAS + lane] = S[F_UPD + lane] = b_lane;
}

enum { M_RESET = 0, M_INTEGRATE = 1, M_SET_BIAS = 2, M_MERGE = 3 };

struct ImuArgs {
    orbi_calib calib;
    orbi_record *bank;
    float *pool;
    int cap, cap_meas, n;
    const int32_t *ids, *second; // second: reset's src, merge's next
    const float *bias;
    const orbi_job *jobs;
    const orbi_sample *samples;
    int n_samples;
    int32_t *result;
};

// `count` measurements through IntegrateNewMeasurement.  src_pool: pool triples (w, a, dt) from `src_pool`; else the samples from
// `smp` with the dt rule of Frame.cpp:73-88.  `append`: where in the record's own pool row the triples go, or NULL.
__device__ __forceinline__ void run_list(float *S, const float *cal, int lane, int count, const float *src_pool, const orbi_sample *smp,
                                         double start, double end, float *append)
{
    uint32_t *stage = (uint32_t *)(S + L_STAGE);
    for (int c0 = 0; c0 < count; c0 += STAGE) {
        const int m = min(STAGE, count - c0);
        WSYNC();                                   // the chunk before this one has been read
        if (src_pool) {
            for (int k = lane; k < 7 * m; k += 64) stage[8 * (k / 7) + k % 7] = __float_as_uint(src_pool[7 * (size_t)c0 + k]);
        } else if (lane < m + 1 && c0 + lane < count) {   // one more: the time stamp behind the chunk's last sample
            const uint2 *p = (const uint2 *)(smp + c0 + lane);   // a sample is 8-byte aligned
#pragma unroll
            for (int q = 0; q < 4; ++q) ((uint2 *)stage)[4 * lane + q] = p[q];
        }
        WSYNC();
        for (int k = 0; k < m; ++k) {
            const float *f = (const float *)(stage + 8 * k);
            float dt;
            if (src_pool) dt = f[6];
            else {
                const int idx = c0 + k;
                const double t = __hiloint2double((int)stage[8 * k + 7], (int)stage[8 * k + 6]);
                const double tn = __hiloint2double((int)stage[8 * k + 15], (int)stage[8 * k + 14]);   // read only where idx + 1 < count
                if (count == 1) dt = (float)ORB_DSUB(end, start);
                else if (idx == 0) dt = (float)ORB_DSUB(tn, start);
                else if (idx == count - 1) dt = (float)ORB_DSUB(end, t);
                else dt = (float)ORB_DSUB(tn, t);
            }
            const float gx = f[0], gy = f[1], gz = f[2], cx = f[3], cy = f[4], cz = f[5];
            if (append && lane < 7) append[7 * (size_t)(c0 + k) + lane] = lane == 6 ? dt : f[lane];
            integrate_sample(S, cal, lane, gx, gy, gz, cx, cy, cz, dt);
        }
    }
}

template <int MODE> __global__ __launch_bounds__(IMU_T) void k_imu(const ImuArgs a)
{
    __shared__ float s_cal[CAL_WORDS];
    __shared__ int s_cnt[8];
    __shared__ __attribute__((aligned(16))) float s_wave[MODE == M_RESET ? 1 : IMU_WAVES][MODE == M_RESET ? 4 : L_WORDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 6) s_cal[threadIdx.x] = a.calib.cov_noise[threadIdx.x], s_cal[6 + threadIdx.x] = a.calib.cov_walk[threadIdx.x];
    __syncthreads();
    const int job = blockIdx.x * IMU_WAVES + wave;
    int code = -1, need = 0;                         // the counter this job adds to
    if (job < a.n) {
        auto id_of = [&](int k) { return MODE == M_INTEGRATE ? a.jobs[k].id : a.ids[k]; };
        auto second_of = [&](int k) { return (MODE == M_RESET || MODE == M_MERGE) && a.second ? a.second[k] : -1; };
        const int id = __builtin_amdgcn_readfirstlane(id_of(job)), second = __builtin_amdgcn_readfirstlane(second_of(job));
        int first = 0, count = 0;
        bool in_range = id >= 0 && id < a.cap;
        if (MODE == M_RESET) in_range = in_range && second >= -1 && second < a.cap;
        if (MODE == M_MERGE) in_range = in_range && second >= 0 && second < a.cap;
        if (MODE == M_INTEGRATE) {
            first = __builtin_amdgcn_readfirstlane(a.jobs[job].first), count = __builtin_amdgcn_readfirstlane(a.jobs[job].count);
            in_range = in_range && first >= 0 && count >= 0 && first <= a.n_samples && count <= a.n_samples - first;
        }
        bool dup = false;
        if (in_range) {
            for (int k = lane; k < job; k += 64) {
                const int id2 = id_of(k), sec2 = second_of(k);
                dup = dup || id == id2 || (second >= 0 && second == id2) || (sec2 >= 0 && id == sec2);
            }
            dup = __ballot(dup) != 0;
        }
        if (!in_range) code = ORBI_R_RANGE;
        else if (dup) code = ORBI_R_DUPLICATE;
        else if (MODE == M_MERGE && id == second) code = ORBI_R_NOOP;
        else {
            orbi_record *rec = a.bank + id;
            float *recf = (float *)rec;
            if (MODE == M_RESET) {
                if (lane < 6) {   // second == id: a lane reads the word it then writes
                    const float b = second >= 0 ? a.bank[second].updated_bias[lane] : a.bias ? a.bias[6 * (size_t)job + lane] : 0.f;
                    recf[F_BIAS + lane] = recf[F_UPD + lane] = b;
                }
                for (int k = F_DELTA + lane; k < F_NMEAS; k += 64) recf[k] = (k == F_DR || k == F_DR + 4 || k == F_DR + 8) ? 1.f : 0.f;
                if (lane == 0) rec->n_meas = 0;
                code = ORBI_R_DONE;
            } else {
                float *S = s_wave[MODE == M_RESET ? 0 : wave];
                float *row = a.pool + (size_t)id * a.cap_meas * 7;
                const int n1 = min(max(__builtin_amdgcn_readfirstlane(rec->n_meas), 0), a.cap_meas);
                int n2 = 0;
                if (MODE == M_INTEGRATE) n2 = count;
                if (MODE == M_MERGE) n2 = min(max(__builtin_amdgcn_readfirstlane(a.bank[second].n_meas), 0), a.cap_meas);
                if (n2 > a.cap_meas - n1) code = ORBI_R_REFUSED, need = n1 + n2;
                else {
                    for (int k = lane; k < F_NMEAS; k += 64) S[k] = recf[k];
                    WSYNC();
                    bool redo = false;
                    if (MODE == M_SET_BIAS) {
                        const float nb = lane < 6 ? a.bias[6 * (size_t)job + lane] : 0.f;
                        if (lane < 6) S[F_UPD + lane] = nb, S[F_DELTA + lane] = sub(nb, S[F_BIAS + lane]);
                        WSYNC();
                    }
                    if (MODE == M_SET_BIAS || MODE == M_MERGE) {
                        const float x = S[F_DELTA], y = S[F_DELTA + 1], z = S[F_DELTA + 2];
                        redo = (double)sqrtf(sum3(mul(x, x), mul(y, y), mul(z, z))) > (MODE == M_SET_BIAS ? 0.01 : 1e-5);
                        if (redo) {
                            const float b = lane < 6 ? S[F_UPD + lane] : 0.f;
                            WSYNC();
                            reset_image(S, lane, b);
                            WSYNC();
                            run_list(S, s_cal, lane, n1, row, nullptr, 0.0, 0.0, nullptr);
                        }
                    }
                    if (MODE == M_INTEGRATE) {
                        const double start = ORB_DADD(a.jobs[job].timestamp, (double)S[F_DT]);
                        run_list(S, s_cal, lane, count, nullptr, a.samples + first, start, a.jobs[job].end_time, row + 7 * (size_t)n1);
                    }
                    if (MODE == M_MERGE) run_list(S, s_cal, lane, n2, a.pool + (size_t)second * a.cap_meas * 7, nullptr, 0.0, 0.0, row + 7 * (size_t)n1);
                    WSYNC();
                    for (int k = lane; k < F_NMEAS; k += 64) recf[k] = S[k];
                    if (lane == 0) rec->n_meas = n1 + n2;
                    code = ORBI_R_DONE;
                    if (redo && lane == 0) atomicAdd(&s_cnt[ORBI_R_REINTEGRATED], 1);
                }
            }
        }
        if (lane == 0) {
            atomicAdd(&s_cnt[code == ORBI_R_NOOP ? ORBI_R_DONE : code], 1);
            if (code == ORBI_R_NOOP) atomicAdd(&s_cnt[ORBI_R_NOOP], 1);
            if (code == ORBI_R_REFUSED) atomicMax(&s_cnt[ORBI_R_NEED], need);
        }
    }
    __syncthreads();
    if (threadIdx.x < 8) {   // flush_counts (orb_device.h) with the greatest NEED: one workgroup writes, several add to k_counters_clear's zeros
        const int v = s_cnt[threadIdx.x];
        if (gridDim.x == 1) a.result[threadIdx.x] = v;
        else if (v) threadIdx.x == ORBI_R_NEED ? atomicMax(&a.result[threadIdx.x], v) : atomicAdd(&a.result[threadIdx.x], v);
    }
}

// the prediction: one wave, nine lanes per matrix; LDS words
enum { P_REC = 0, P_SRC = 79, P_W = 94, P_E = 103, P_M = 112, P_M2 = 121, P_DRU = 130, P_RWB = 139, P_VEC = 148, P_WORDS = 160 };
// P_VEC: th[3] = JRg*dbg, dVu[3], dPu[3], twb2[3]
__global__ __launch_bounds__(64) void k_imu_predict(const orbi_calib cal, const orbi_record *__restrict__ rec, const float *src, float *dst,
                                                    double *pose_R, double *pose_t)
{
    __shared__ float S[P_WORDS];
    __shared__ float s_cb[12];
    const int lane = threadIdx.x, e = lane % 9, i = e / 3, j = e - 3 * i, g = lane / 9;
    const float *recf = (const float *)rec;
    for (int k = lane; k < F_C; k += 64) S[P_REC + k] = recf[k];
    if (lane < 15) S[P_SRC + lane] = src[lane];
    if (lane < 9) s_cb[lane] = cal.Rcb[lane];
    if (lane < 3) s_cb[9 + lane] = cal.tcb[lane];
    WSYNC();
    const float *dbg = S + F_DELTA, *dba = S + F_DELTA + 3, *Rwb = S + P_SRC, *twb = S + P_SRC + 9, *v = S + P_SRC + 12;
    const float dt = S[F_DT];
    // th = JRg*dbg; dVu, dPu
    if (lane < 3) S[P_VEC + lane] = mv3(S + F_JRG, dbg, lane);
    else if (lane < 6) S[P_VEC + lane] = add(add(S[F_DV + lane - 3], mv3(S + F_JVG, dbg, lane - 3)), mv3(S + F_JVA, dba, lane - 3));
    else if (lane < 9) S[P_VEC + lane] = add(add(S[F_DP + lane - 6], mv3(S + F_JPG, dbg, lane - 6)), mv3(S + F_JPA, dba, lane - 6));
    WSYNC();
    const float tx = S[P_VEC], ty = S[P_VEC + 1], tz = S[P_VEC + 2];
    const So3 so = so3_scalars(tx, ty, tz);
    if (g == 0) S[P_W + e] = hat(tx, ty, tz, e);
    WSYNC();
    if (g == 0) S[P_E + e] = exp_entry(so, S + P_W, e);
    WSYNC();
    if (g == 0) S[P_M + e] = m3(S + F_DR, S + P_E, i, j);
    WSYNC();
    if (g == 0) S[P_M2 + e] = newton_entry(S + P_M, i, j);
    WSYNC();
    if (g == 0) S[P_DRU + e] = newton_entry(S + P_M2, i, j);
    WSYNC();
    if (g == 0) S[P_M + e] = m3(Rwb, S + P_DRU, i, j);
    else if (g == 1 && e < 3) {   // twb2 and v2, g = (0, 0, -gravity)
        const float ge = e == 2 ? -cal.gravity : 0.f;
        S[P_VEC + 9 + e] = add(add(add(twb[e], mul(v[e], dt)), mul(mul(mul(0.5f, ge), dt), dt)), mv3(Rwb, S + P_VEC + 6, e));
        dst[12 + e] = add(add(v[e], mul(ge, dt)), mv3(Rwb, S + P_VEC + 3, e));
    }
    WSYNC();
    if (g == 0) S[P_M2 + e] = newton_entry(S + P_M, i, j);
    WSYNC();
    if (g == 0) S[P_RWB + e] = newton_entry(S + P_M2, i, j);
    WSYNC();
    // T_wb.inverse() = (Rwb2^T, (-(Rwb2^T))*twb2); T_cw = T_cb * that
    const float *R2 = S + P_RWB, *t2 = S + P_VEC + 9;
    if (g == 0) {
        dst[e] = R2[e];
        const float r = sum3(mul(s_cb[3 * i], R2[3 * j]), mul(s_cb[3 * i + 1], R2[3 * j + 1]), mul(s_cb[3 * i + 2], R2[3 * j + 2]));   // Rcb*Rwb2^T
        if (pose_R) pose_R[e] = (double)r;
    } else if (g == 1 && e < 3) {
        dst[9 + e] = t2[e];
        float tbw[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) tbw[k] = sum3(mul(-R2[k], t2[0]), mul(-R2[3 + k], t2[1]), mul(-R2[6 + k], t2[2]));
        const float t = add(sum3(mul(s_cb[3 * e], tbw[0]), mul(s_cb[3 * e + 1], tbw[1]), mul(s_cb[3 * e + 2], tbw[2])), s_cb[9 + e]);
        if (pose_t) pose_t[e] = (double)t;
    }
}

// T_wb = T_cw.inverse() * T_cb
__global__ __launch_bounds__(64) void k_imu_pose(const orbi_calib cal, const double *__restrict__ pose_R, const double *__restrict__ pose_t,
                                                 float *__restrict__ dst)
{
    __shared__ float R[9], t[3], s_cb[12], twc[3];
    const int lane = threadIdx.x;
    if (lane < 9) R[lane] = (float)pose_R[lane], s_cb[lane] = cal.Rcb[lane];
    if (lane < 3) t[lane] = (float)pose_t[lane], s_cb[9 + lane] = cal.tcb[lane];
    WSYNC();
    imu_pose_from_camera(R, t, s_cb, twc, dst, lane);
}

int check_bank(const void *bank, int cap, int n, const void *result)
{
    if (!bank || cap < 1 || n < 0 || !result) return orbx_set_error(ORBX_E_ARG, "null bank or result, cap < 1 or a negative job count");
    if (n > ORBI_MAX_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBI_MAX_JOBS (4096) jobs in one call");
    return ORBX_OK;
}

template <int MODE> int launch(const ImuArgs &a, void *stream)
{
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream; // NULL is stream 0 itself (include/orbx.h, "Streams")
    const int grid = (a.n + IMU_WAVES - 1) / IMU_WAVES;
    LAUNCH_COUNTED(k_imu<MODE>, grid, IMU_T, s, a.result, a);
    return ORBX_OK;
}

} // namespace

extern "C" int orbi_reset_device(orbi_record *d_bank, int cap, const int32_t *d_ids, const int32_t *d_src, const float *d_bias, int n,
                                 int32_t *d_result, void *stream)
{
    if (int rc = check_bank(d_bank, cap, n, d_result)) return rc;
    if (!d_ids) return orbx_set_error(ORBX_E_ARG, "null id array");
    ImuArgs a = {};
    a.bank = d_bank, a.cap = cap, a.n = n, a.ids = d_ids, a.second = d_src, a.bias = d_bias, a.result = d_result;
    return launch<M_RESET>(a, stream);
}

extern "C" int orbi_integrate_device(orbi_calib calib, orbi_record *d_bank, float *d_pool, int cap, int cap_meas, const orbi_job *d_jobs, int n,
                                     const orbi_sample *d_samples, int n_samples, int32_t *d_result, void *stream)
{
    if (int rc = check_bank(d_bank, cap, n, d_result)) return rc;
    if (!d_pool || cap_meas < 1 || !d_jobs || !d_samples || n_samples < 0) return orbx_set_error(ORBX_E_ARG, "null pool, jobs or samples, cap_meas < 1 or a negative sample count");
    ImuArgs a = {};
    a.calib = calib, a.bank = d_bank, a.pool = d_pool, a.cap = cap, a.cap_meas = cap_meas, a.n = n, a.jobs = d_jobs, a.samples = d_samples;
    a.n_samples = n_samples, a.result = d_result;
    return launch<M_INTEGRATE>(a, stream);
}

extern "C" int orbi_set_bias_device(orbi_calib calib, orbi_record *d_bank, float *d_pool, int cap, int cap_meas, const int32_t *d_ids,
                                    const float *d_bias, int n, int32_t *d_result, void *stream)
{
    if (int rc = check_bank(d_bank, cap, n, d_result)) return rc;
    if (!d_pool || cap_meas < 1 || !d_ids || !d_bias) return orbx_set_error(ORBX_E_ARG, "null pool, id or bias array, or cap_meas < 1");
    ImuArgs a = {};
    a.calib = calib, a.bank = d_bank, a.pool = d_pool, a.cap = cap, a.cap_meas = cap_meas, a.n = n, a.ids = d_ids, a.bias = d_bias, a.result = d_result;
    return launch<M_SET_BIAS>(a, stream);
}

extern "C" int orbi_merge_next_device(orbi_calib calib, orbi_record *d_bank, float *d_pool, int cap, int cap_meas, const int32_t *d_ids,
                                      const int32_t *d_next, int n, int32_t *d_result, void *stream)
{
    if (int rc = check_bank(d_bank, cap, n, d_result)) return rc;
    if (!d_pool || cap_meas < 1 || !d_ids || !d_next) return orbx_set_error(ORBX_E_ARG, "null pool, id or next array, or cap_meas < 1");
    ImuArgs a = {};
    a.calib = calib, a.bank = d_bank, a.pool = d_pool, a.cap = cap, a.cap_meas = cap_meas, a.n = n, a.ids = d_ids, a.second = d_next, a.result = d_result;
    return launch<M_MERGE>(a, stream);
}

extern "C" int orbi_predict_device(orbi_calib calib, const orbi_record *d_bank, int cap, int id, const float *d_src, float *d_dst,
                                   double *d_pose_R, double *d_pose_t, void *stream)
{
    if (!d_bank || cap < 1 || id < 0 || id >= cap || !d_src || !d_dst) return orbx_set_error(ORBX_E_ARG, "null bank, source or destination, or id outside [0, cap)");
    if (!d_pose_R != !d_pose_t) return orbx_set_error(ORBX_E_ARG, "d_pose_R and d_pose_t go together");
    if (int rc = orb_need_device()) return rc;
    hipLaunchKernelGGL(k_imu_predict, dim3(1), dim3(64), 0, (hipStream_t)stream, calib, d_bank + id, d_src, d_dst, d_pose_R, d_pose_t);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbi_imu_pose_device(orbi_calib calib, const double *d_pose_R, const double *d_pose_t, float *d_dst, void *stream)
{
    if (!d_pose_R || !d_pose_t || !d_dst) return orbx_set_error(ORBX_E_ARG, "null pose or destination");
    if (int rc = orb_need_device()) return rc;
    hipLaunchKernelGGL(k_imu_pose, dim3(1), dim3(64), 0, (hipStream_t)stream, calib, d_pose_R, d_pose_t, d_dst);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
