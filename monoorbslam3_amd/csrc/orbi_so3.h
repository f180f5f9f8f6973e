// Float SO(3) helpers shared by the IMU kernels (orbi_imu.hip, orbi_factors.hip, orbii.hip, orbm_rescale.hip): the wave-level fence, the IEEE +, -, *, / wrappers
// and the 3x3 products, ExpSO3f, RightJacobianSO3f and the Newton NormalizeRotationf in the evaluation orders include/orbi.h fixes.
// Internal: everything is a macro or a forced-inline device function inside an anonymous namespace, so it adds no symbol.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "orb_math.h"

namespace {

#define WSYNC()                                                \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                       \
    } while (0)

__device__ __forceinline__ float mul(float a, float b) { return ORB_FMUL(a, b); }
__device__ __forceinline__ float add(float a, float b) { return ORB_FADD(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return ORB_FSUB(a, b); }
__device__ __forceinline__ float dvd(float a, float b) { return ORB_FDIV(a, b); }
__device__ __forceinline__ float sum3(float p0, float p1, float p2) { return add(add(p0, p1), p2); }

// entries (i, j) of A*B, A^T*B, A*B^T and (s*A)*B; matrices row-major
__device__ __forceinline__ float m3(const float *A, const float *B, int i, int j) { return sum3(mul(A[3 * i], B[j]), mul(A[3 * i + 1], B[3 + j]), mul(A[3 * i + 2], B[6 + j])); }
__device__ __forceinline__ float m3t(const float *A, const float *B, int i, int j) { return sum3(mul(A[i], B[j]), mul(A[3 + i], B[3 + j]), mul(A[6 + i], B[6 + j])); }
__device__ __forceinline__ float m3s(float s, const float *A, const float *B, int i, int j)
{
    return sum3(mul(mul(s, A[3 * i]), B[j]), mul(mul(s, A[3 * i + 1]), B[3 + j]), mul(mul(s, A[3 * i + 2]), B[6 + j]));
}
__device__ __forceinline__ float mv3(const float *A, const float *x, int i) { return sum3(mul(A[3 * i], x[0]), mul(A[3 * i + 1], x[1]), mul(A[3 * i + 2], x[2])); }

// entry e = 3i + j of Hatf(x, y, z) (LieAlgeBra.cpp:22-28)
__device__ __forceinline__ float hat(float x, float y, float z, int e)
{
    return e == 1 ? -z : e == 2 ? y : e == 3 ? z : e == 5 ? -x : e == 6 ? -y : e == 7 ? x : 0.f;
}
__device__ __forceinline__ float eye(int e) { return (e == 0 || e == 4 || e == 8) ? 1.f : 0.f; }

// the scalars of ExpSO3f / RightJacobianSO3f of the vector whose Hatf is W: small (d < 1e-6 in double), sin(d)/d, (1-cos(d))/d2, (d-sin(d))/(d2*d)
struct So3 {
    bool small;
    float s1, s2, s3;
};
__device__ __forceinline__ So3 so3_scalars(float x, float y, float z)
{
    So3 o;
    const float d2 = sum3(mul(x, x), mul(y, y), mul(z, z));
    const float d = sqrtf(d2);
    o.small = (double)d < 1e-6;
    o.s1 = o.s2 = o.s3 = 0.f;
    if (!o.small) {
        float sn, cs;
        orb_sincosf(d, &sn, &cs);
        o.s1 = dvd(sn, d);
        o.s2 = dvd(sub(1.f, cs), d2);
        o.s3 = dvd(sub(d, sn), mul(d2, d));
    }
    return o;
}
__device__ __forceinline__ float exp_entry(const So3 &s, const float *W, int e)
{
    const int i = e / 3, j = e - 3 * i;
    if (s.small) return add(add(eye(e), W[e]), m3s(0.5f, W, W, i, j));
    return add(add(eye(e), mul(s.s1, W[e])), m3s(s.s2, W, W, i, j));
}
__device__ __forceinline__ float rightj_entry(const So3 &s, const float *W, int e)
{
    const int i = e / 3, j = e - 3 * i;
    if (s.small) return eye(e);
    return add(sub(eye(e), mul(s.s2, W[e])), m3s(s.s3, W, W, i, j));
}
// entry (i, j) of one Newton step towards the polar factor: 0.5f*(X + cof(X)/det(X))
__device__ __forceinline__ float cof(const float *X, int i, int j)
{
    const int p = i == 2 ? 0 : i + 1, r = i == 0 ? 2 : i - 1, q = j == 2 ? 0 : j + 1, s = j == 0 ? 2 : j - 1;
    return sub(mul(X[3 * p + q], X[3 * r + s]), mul(X[3 * p + s], X[3 * r + q]));
}
__device__ __forceinline__ float newton_entry(const float *X, int i, int j)
{
    const float det = sum3(mul(X[0], cof(X, 0, 0)), mul(X[1], cof(X, 0, 1)), mul(X[2], cof(X, 0, 2)));
    return mul(0.5f, add(X[3 * i + j], dvd(cof(X, i, j), det)));
}

// ---- what the kernels on an orbi_record's head share ----------------------------------------------------------------------------------
// the head of an orbi_record in floats (== offsetof(orbi_record, ...) / 4; the sources that use it assert that)
enum { RH_BIAS = 0, RH_UPD = 6, RH_DELTA = 12, RH_DT = 18, RH_DR = 19, RH_DV = 28, RH_DP = 31, RH_JRG = 34, RH_JVG = 43, RH_JVA = 52, RH_JPG = 61, RH_JPA = 70, RH_WORDS = 79 };
// the temporaries of bias_deltas: db[6] = b - bias, th[3] = JRg*dbg, (dV, dP)[6], W, E, M, M2 [9 each], dR [9]
enum { BD_DB = 0, BD_TH = 6, BD_DVP = 9, BD_W = 15, BD_E = 24, BD_M = 33, BD_M2 = 42, BD_DRU = 51, BD_WORDS = 61 };
// getDeltaRotation / Velocity / Position (Imu.cpp:182-192) of the bias whose entry `lane` (< 6) is b, by one wave: H the record's head and
// T the temporaries, both in the wave's LDS.  Leaves dR in T[BD_DRU ..), (dV, dP) in T[BD_DVP ..), b - bias in T[BD_DB ..); ends on a WSYNC
__device__ __forceinline__ void bias_deltas(const float *H, float *T, int lane, float b)
{
    const int g = lane / 9, q = lane - 9 * g, i = q / 3, j = q - 3 * i;
    if (lane < 6) T[BD_DB + lane] = sub(b, H[RH_BIAS + lane]);
    WSYNC();
    if (lane < 3) T[BD_TH + lane] = mv3(H + RH_JRG, T + BD_DB, lane);
    else if (lane < 6) T[BD_DVP + lane - 3] = add(add(H[RH_DV + lane - 3], mv3(H + RH_JVG, T + BD_DB, lane - 3)), mv3(H + RH_JVA, T + BD_DB + 3, lane - 3));
    else if (lane < 9) T[BD_DVP + lane - 3] = add(add(H[RH_DP + lane - 6], mv3(H + RH_JPG, T + BD_DB, lane - 6)), mv3(H + RH_JPA, T + BD_DB + 3, lane - 6));
    WSYNC();
    const float tx = T[BD_TH], ty = T[BD_TH + 1], tz = T[BD_TH + 2];
    const So3 so = so3_scalars(tx, ty, tz);
    if (g == 0) T[BD_W + q] = hat(tx, ty, tz, q);
    WSYNC();
    if (g == 0) T[BD_E + q] = exp_entry(so, T + BD_W, q);
    WSYNC();
    if (g == 0) T[BD_M + q] = m3(H + RH_DR, T + BD_E, i, j);
    WSYNC();
    if (g == 0) T[BD_M2 + q] = newton_entry(T + BD_M, i, j);
    WSYNC();
    if (g == 0) T[BD_DRU + q] = newton_entry(T + BD_M2, i, j);
    WSYNC();
}

// T_wb = T_cw.inverse() * T_cb (Frame.cpp:57-63, KeyFrame.cpp:27-34) by the first twelve lanes of a wave: R[9], t[3] = T_cw, cb[12] = (Rcb, tcb)
// and twc[3] (scratch) in the wave's LDS, filled and fenced by the caller; dst[0..12) receives (Rwb, twb)
__device__ __forceinline__ void imu_pose_from_camera(const float *R, const float *t, const float *cb, float *twc, float *dst, int lane)
{
    const int i = lane / 3, j = lane - 3 * i;
    if (lane < 3) twc[lane] = sum3(mul(-R[lane], t[0]), mul(-R[3 + lane], t[1]), mul(-R[6 + lane], t[2]));
    WSYNC();
    if (lane < 9) dst[lane] = m3t(R, cb, i, j);                                                    // Rcw^T * Rcb
    else if (lane < 12) {
        const int k = lane - 9;
        dst[lane] = add(sum3(mul(R[k], cb[9]), mul(R[3 + k], cb[10]), mul(R[6 + k], cb[11])), twc[k]);   // Rcw^T * tcb + twc
    }
}

} // namespace
