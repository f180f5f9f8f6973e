// Double SO(3) helpers shared by the kernels behind the cast to double (orbi_factors.hip, orbii.hip): the 3x3 products, Hat, LogSO3,
// RightJacobianSO3, InverseRightJacobianSO3, ExpSO3 and the Newton NormalizeRotation (LieAlgeBra.cpp:30-41, 60-70, 84-112, 124-127) in the evaluation orders include/orbi.h fixes: IEEE +, -, *, /
// without fused multiply-add, a product-sum as (p0 + p1) + p2, Hat's zeros multiplied.  tests/factors_model.py restates them.
// Internal: forced-inline device functions inside an anonymous namespace, so it adds no symbol.  A correction is made here, once.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "orb_math.h"
#include "orbi_graph_device.h"   // dsum3, the ordered three-term sum

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ double dmul(double a, double b) { return ORB_DMUL(a, b); }
// entries (i, j) of A*B, A^T*B, A*B^T and A^T*B^T; matrices row-major
__device__ __forceinline__ double dm3(const double *A, const double *B, int i, int j) { return dsum3(dmul(A[3 * i], B[j]), dmul(A[3 * i + 1], B[3 + j]), dmul(A[3 * i + 2], B[6 + j])); }
__device__ __forceinline__ double dm3t(const double *A, const double *B, int i, int j) { return dsum3(dmul(A[i], B[j]), dmul(A[3 + i], B[3 + j]), dmul(A[6 + i], B[6 + j])); }
__device__ __forceinline__ double dm3nt(const double *A, const double *B, int i, int j) { return dsum3(dmul(-A[3 * i], B[3 * j]), dmul(-A[3 * i + 1], B[3 * j + 1]), dmul(-A[3 * i + 2], B[3 * j + 2])); } // (-A)*B^T
__device__ __forceinline__ double dm3tt(const double *A, const double *B, int i, int j) { return dsum3(dmul(A[i], B[3 * j]), dmul(A[3 + i], B[3 * j + 1]), dmul(A[6 + i], B[3 * j + 2])); }
__device__ __forceinline__ double dmv3t(const double *A, double x0, double x1, double x2, int i) { return dsum3(dmul(A[i], x0), dmul(A[3 + i], x1), dmul(A[6 + i], x2)); } // (A^T*x)_i
__device__ __forceinline__ double dhat(double x, double y, double z, int e)
{
    return e == 1 ? -z : e == 2 ? y : e == 3 ? z : e == 5 ? -x : e == 6 ? -y : e == 7 ? x : 0.0;
}
__device__ __forceinline__ double deye(int e) { return (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0; }
__device__ __forceinline__ double dsww(double s, double x, double y, double z, int i, int j) // ((s*W)*W)_ij, W = Hat(x, y, z), zeros multiplied
{
    return dsum3(dmul(dmul(s, dhat(x, y, z, 3 * i)), dhat(x, y, z, j)), dmul(dmul(s, dhat(x, y, z, 3 * i + 1)), dhat(x, y, z, 3 + j)),
                 dmul(dmul(s, dhat(x, y, z, 3 * i + 2)), dhat(x, y, z, 6 + j)));
}
__device__ __forceinline__ double dnorm2(double x, double y, double z) { return dsum3(dmul(x, x), dmul(y, y), dmul(z, z)); }
// the double Newton step towards the polar factor: NormalizeRotationf's sequence, widened
__device__ __forceinline__ double dcof(const double *X, int i, int j)
{
    const int p = i == 2 ? 0 : i + 1, r = i == 0 ? 2 : i - 1, q = j == 2 ? 0 : j + 1, s = j == 0 ? 2 : j - 1;
    return dmul(X[3 * p + q], X[3 * r + s]) - dmul(X[3 * p + s], X[3 * r + q]);
}
__device__ __forceinline__ double ddet(const double *X) { return dsum3(dmul(X[0], dcof(X, 0, 0)), dmul(X[1], dcof(X, 0, 1)), dmul(X[2], dcof(X, 0, 2))); }
// NormalizeRotation in double: two Newton steps, in registers
__device__ __forceinline__ void dnormalize(double X[9])
{
#pragma unroll
    for (int step = 0; step < 2; ++step) {
        double Y[9];
        const double det = ddet(X);
#pragma unroll
        for (int k = 0; k < 9; ++k) Y[k] = dmul(0.5, X[k] + dcof(X, k / 3, k % 3) / det);
#pragma unroll
        for (int k = 0; k < 9; ++k) X[k] = Y[k];
    }
}
// ExpSO3(x, y, z), which returns NormalizeRotation of its series
__device__ __forceinline__ void dexp_so3(double x, double y, double z, double E[9])
{
    const double d2 = dnorm2(x, y, z), dd = sqrt(d2);
    const bool small = dd < 1e-6;
    const double s1 = small ? 1.0 : sin(dd) / dd, s2 = small ? 0.5 : (1.0 - cos(dd)) / d2;
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = (deye(k) + dmul(s1, dhat(x, y, z, k))) + dsww(s2, x, y, z, k / 3, k % 3);
    dnormalize(E);
}
// LogSO3(R) with its tr == 3 exit and its 1e-6 branch
__device__ __forceinline__ void dlog_so3(const double *R, double &er0, double &er1, double &er2)
{
    const double tr = (R[0] + R[4]) + R[8];
    er0 = 0.0, er1 = 0.0, er2 = 0.0;
    if (tr != 3.0) {
        const double w0 = dmul(0.5, R[7] - R[5]), w1 = dmul(0.5, R[2] - R[6]), w2 = dmul(0.5, R[3] - R[1]);
        const double sn = sqrt(dnorm2(w0, w1, w2)), cs = dmul(0.5, tr - 1.0);
        const double th = atan2(sn, cs);
        if (fabs(th) < 1e-6) er0 = w0, er1 = w1, er2 = w2;
        else er0 = dmul(th, w0) / sn, er1 = dmul(th, w1) / sn, er2 = dmul(th, w2) / sn;
    }
}
// entry q = 3i + j of RightJacobianSO3(x, y, z) and of InverseRightJacobianSO3(x, y, z)
__device__ __forceinline__ double dright_jacobian(double x, double y, double z, int q)
{
    const double d2 = dnorm2(x, y, z), d = sqrt(d2);
    double v = deye(q);
    if (!(d < 1e-6)) v = (deye(q) - dmul((1.0 - cos(d)) / d2, dhat(x, y, z, q))) + dsww((d - sin(d)) / dmul(d2, d), x, y, z, q / 3, q % 3);
    return v;
}
__device__ __forceinline__ double dinverse_right_jacobian(double x, double y, double z, int q)
{
    const double d2 = dnorm2(x, y, z), d = sqrt(d2);
    double v = deye(q);
    if (!(d < 1e-6)) {
        const double coef = 1.0 / d2 - (1.0 + cos(d)) / dmul(dmul(2.0, d), sin(d));
        v = (deye(q) + dhat(x, y, z, q) / 2.0) + dsww(coef, x, y, z, q / 3, q % 3);
    }
    return v;
}

} // namespace
