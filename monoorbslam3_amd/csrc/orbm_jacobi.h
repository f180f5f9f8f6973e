// The one-sided (Hestenes) Jacobi steps that orbm_triangulate.hip, orbm_two_view.hip and orbm_two_view_pose.hip share: a rotation of two
// COLUMNS of a small matrix (stored by column) and of V, fully in registers with constant indices.  Float on 4 x 4 for Triangulate
// (TwoViewReconstruction.cpp:689-705), double on 3 x 3 for the rank-2 step of ComputeF21 and the decompositions of ReconstructH /
// DecomposeE.  The including file sets `#pragma clang fp contract(off)`; the build passes -ffp-contract=off as well.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

constexpr int TR_SWEEPS = 6;   // cyclic sweeps of the 4 x 4: a numpy float32 restatement settles in four on the test clouds

__device__ __forceinline__ float dot4(const float (&a)[4], const float (&b)[4]) { return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]; }

// one Hestenes rotation of the columns p, q of A (stored by column) and of V
__device__ __forceinline__ void rotate(float (&ap)[4], float (&aq)[4], float (&vp)[4], float (&vq)[4])
{
    const float alpha = dot4(ap, ap), beta = dot4(aq, aq), gamma = dot4(ap, aq);
    float t = 0.f;
    if (gamma != 0.f) {   // (NaN takes this branch and spreads)
        const float zeta = (beta - alpha) / (2.f * gamma);
        t = copysignf(1.f, zeta) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
    }
    const float c = 1.f / sqrtf(1.f + t * t), s = c * t;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float x = ap[r], y = aq[r];
        ap[r] = c * x - s * y;
        aq[r] = s * x + c * y;
        const float vx = vp[r], vy = vq[r];
        vp[r] = c * vx - s * vy;
        vq[r] = s * vx + c * vy;
    }
}

// the rotation angle of one Hestenes step from the three dot products
__device__ __forceinline__ void jacobi_cs(double alpha, double beta, double gamma, double &c, double &s)
{
    double t = 0.0;
    if (gamma != 0.0) {
        const double zeta = (beta - alpha) / (2.0 * gamma);
        t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    }
    c = 1.0 / sqrt(1.0 + t * t);
    s = c * t;
}

__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void rotate3(double (&ap)[3], double (&aq)[3], double (&vp)[3], double (&vq)[3])
{
    double c, s;
    jacobi_cs(dot3(ap, ap), dot3(aq, aq), dot3(ap, aq), c, s);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double x = ap[r], y = aq[r];
        ap[r] = c * x - s * y;
        aq[r] = s * x + c * y;
        const double vx = vp[r], vy = vq[r];
        vp[r] = c * vx - s * vy;
        vq[r] = s * vx + c * vy;
    }
}
