// Float SO(3) helpers shared by the IMU kernels (orbi_imu.hip, orbi_factors.hip): the wave-level fence, the IEEE +, -, *, / wrappers
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

} // namespace
