// What the kernels on EdgeInertial share beyond orbi_edge.h (k_fac_edge and k_fac_recover of orbi_factors.hip: a bias pair per state;
// k_fi_edge and k_fi_recover of orbfi.hip: one bias pair in a carrier state): the fields of a wave's slices that EdgeInertial adds to
// orbi_edge.h's, ev and ep, the entries of the raw 9 x 30 Jacobian (G2oTypes.cpp:377-445), a job of the optimisers' recovery
// (Optimize.cpp:401-434, :602-607, :1044-1053).  The flush of a workgroup's counters is orb_device.h's.  Every order is the one
// include/orbi.h fixes.
// Internal: forced-inline device functions inside an anonymous namespace, so it adds no symbol.  A correction is made here, once.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbi.h"
#include "orb_device.h"
#include "orbi_edge.h"
#include "orbi_graph_device.h"
#include "orbi_so3.h"
#include "orbi_so3d.h"

#pragma clang fp contract(off)

namespace {

// a wave's LDS slice: floats (orbi_edge.h's X_WORDS) and doubles (orbi_edge.h's shared fields, then (bg, ba) of state i and of state j,
// Rb1w*R2, (-invJr)*R2^T, Rb1w*(v2 - v1 - g*dt), Rb1w*(t2 - t1 - v1*dt - 0.5*g*dt*dt), J and W*J)
enum { D_B1 = D_SHARED, D_B2 = D_B1 + 6, D_RR = D_B2 + 6, D_T3 = D_RR + 9, D_A = D_T3 + 9, D_C = D_A + 3, D_J = D_C + 3, D_WJ = D_J + 270, D_WORDS = D_WJ + 270 };

// entry (r, c) of the raw 9 x 30 Jacobian (G2oTypes.cpp:413-444), columns [dphi1, dt1, dv1, dbg, dba | dphi2, dt2, dv2, -, -]
__device__ __forceinline__ double jac_entry(const double *S, double dt, int r, int c)
{
    const int rb = r / 3, i = r - 3 * rb, cb = c / 3, j = c - 3 * cb;
    if (rb == 0) {
        if (cb == 0) return dm3(S + D_T3, S + D_R1, i, j);             // ((-invJr)*R2^T)*R1
        if (cb == 3) return dm3(S + D_T5, S + D_JRG, i, j);            // (((-invJr)*eR^T)*Jr)*JRg
        if (cb == 5) return S[D_INVJ + 3 * i + j];
        return 0.0;
    }
    if (rb == 1) {
        if (cb == 0) return dhat(S[D_A], S[D_A + 1], S[D_A + 2], 3 * i + j);
        if (cb == 2) return -S[D_R1 + 3 * j + i];                      // -Rb1w
        if (cb == 3) return -S[D_JVG + 3 * i + j];
        if (cb == 4) return -S[D_JVA + 3 * i + j];
        if (cb == 7) return S[D_R1 + 3 * j + i];
        return 0.0;
    }
    if (cb == 0) return dhat(S[D_C], S[D_C + 1], S[D_C + 2], 3 * i + j);
    if (cb == 1) return i == j ? -1.0 : -0.0;                          // -Identity
    if (cb == 2) return dmul(-S[D_R1 + 3 * j + i], dt);                // (-Rb1w)*dt
    if (cb == 3) return -S[D_JPG + 3 * i + j];
    if (cb == 4) return -S[D_JPA + 3 * i + j];
    if (cb == 6) return S[D_RR + 3 * i + j];                           // Rb1w*R2
    return 0.0;
}

// this edge's lines of the phase behind edge_widen, on lane groups 2 .. 4 ahead of edge_rotation: Rb1w*(v2 - v1 - g*dt) with ev,
// Rb1w*(t2 - t1 - v1*dt - 0.5*g*dt*dt) with ep, and Rb1w*R2.  No fence
__device__ __forceinline__ void edge_velocity_position(double *S, int lane, double G, double dt)
{
    const int g = lane / 9, q = lane - 9 * g, i = q / 3, j = q - 3 * i;
    if (g == 2 && q < 3) {
        double d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = (S[D_V2 + k] - S[D_V1 + k]) - dmul(k == 2 ? -G : 0.0, dt);
        const double v = dmv3t(S + D_R1, d[0], d[1], d[2], q);
        S[D_A + q] = v, S[D_E + 3 + q] = v - S[D_DVP + q];
    } else if (g == 3 && q < 3) {
        double d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = ((S[D_T2 + k] - S[D_T1 + k]) - dmul(S[D_V1 + k], dt)) - dmul(dmul(dmul(0.5, k == 2 ? -G : 0.0), dt), dt);
        const double v = dmv3t(S + D_R1, d[0], d[1], d[2], q);
        S[D_C + q] = v, S[D_E + 6 + q] = v - S[D_DVP + 3 + q];
    } else if (g == 4) S[D_RR + q] = dm3t(S + D_R1, S + D_R2, i, j);
}

// one job (state, destination, flags) of the recovery: v, and with ORBI_RECOVER_POSE in `flags` (Rwb, twb), rounded to float into the
// destination row; (bg, ba) of state `bias_st` rounded to float into the job's d_bias row; T_cw = T_cb * T_wb.inverse() of those floats
// (k_imu_predict's orders) where pose_R is given.  Returns the counter the job falls in; a dropped job's d_bias row is zero
__device__ __forceinline__ int recover_job(const orbi_graph &g, const orbi_calib &cal, const int32_t *jobs, int job, int st, int to, int flags,
                                           int bias_st, float *dst, int n_dst, float *bias, double *pose_R, double *pose_t)
{
    int code = ORBI_R_DONE;
    if (st < 0 || st >= g.n_states || to < 0 || to >= n_dst) code = ORBI_R_RANGE;
    else if (job_named_before(jobs, 3, job, 1, to)) code = ORBI_R_DUPLICATE;
    if (code != ORBI_R_DONE) {
        for (int k = 0; k < 6; ++k) bias[6 * (size_t)job + k] = 0.f;
        return code;
    }
    float *o = dst + 15 * (size_t)to;
    for (int k = 0; k < 3; ++k) {
        o[12 + k] = (float)g.v[3 * (size_t)st + k];
        bias[6 * (size_t)job + k] = (float)g.bg[3 * (size_t)bias_st + k];
        bias[6 * (size_t)job + 3 + k] = (float)g.ba[3 * (size_t)bias_st + k];
    }
    if (flags & ORBI_RECOVER_POSE) {
        float R[9], t[3], tbw[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = R[k] = (float)g.Rwb[9 * (size_t)st + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) o[9 + k] = t[k] = (float)g.twb[3 * (size_t)st + k];
        if (pose_R) {
#pragma unroll
            for (int k = 0; k < 3; ++k) tbw[k] = sum3(mul(-R[k], t[0]), mul(-R[3 + k], t[1]), mul(-R[6 + k], t[2]));
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int i = k / 3, j = k % 3;
                pose_R[9 * (size_t)job + k] = (double)sum3(mul(cal.Rcb[3 * i], R[3 * j]), mul(cal.Rcb[3 * i + 1], R[3 * j + 1]), mul(cal.Rcb[3 * i + 2], R[3 * j + 2]));
            }
#pragma unroll
            for (int k = 0; k < 3; ++k)
                pose_t[3 * (size_t)job + k] = (double)add(sum3(mul(cal.Rcb[3 * k], tbw[0]), mul(cal.Rcb[3 * k + 1], tbw[1]), mul(cal.Rcb[3 * k + 2], tbw[2])), cal.tcb[k]);
        }
    }
    return code;
}

} // namespace
