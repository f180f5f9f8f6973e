// What the inertial edge kernels share behind the cast to double (k_fac_edge of orbi_factors.hip: EdgeInertial; k_ii_edge of orbii.hip:
// EdgeInertialGS / EdgeInertialG): the layout of the shared fields of a wave's double slice, the prologue, the widening, the rotation
// residual with its Jacobian factors (G2oTypes.cpp:94-112, 134-141, 377-396, 413-421), Omega*e with chi2 and constructQuadraticForm
// (G2oTypes.h:324-343), in the evaluation orders include/orbi.h fixes: IEEE +, -, *, / without fused multiply-add, every 9-term sum from
// 0.0 in ascending k.  tests/factors_model.py and tests/imu_init_model.py restate them, each on its own.
// One wave per edge: S is the wave's slice of doubles in LDS, the lanes are spread over matrix entries in groups of nine (group g = lane / 9,
// entry q = lane % 9) and the phases are separated by WSYNC only.  ev and ep, the Jacobian's entries, the Huber weight and the walks are the
// kernels' own.  Internal: forced-inline device functions inside an anonymous namespace, so it adds no symbol.  A correction is made here, once.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbi.h"
#include "orbi_so3.h"
#include "orbi_so3d.h"

#pragma clang fp contract(off)

static_assert(offsetof(orbi_record, JPa) == 4 * RH_JPA && offsetof(orbi_record, C) == 4 * RH_WORDS && offsetof(orbi_record, delta_t) == 4 * RH_DT &&
                  offsetof(orbi_record, delta_bias) == 4 * RH_DELTA,
              "the LDS image is the head of the record");

namespace {

// a wave's float slice: the record's head, then the temporaries of bias_deltas
enum { X_T = RH_WORDS, X_WORDS = RH_WORDS + BD_WORDS };
// the shared fields of a wave's double slice; a kernel numbers its own fields from D_SHARED on
enum {
    D_R1 = 0, D_R2 = 9, D_T1 = 18, D_T2 = 21, D_V1 = 24, D_V2 = 27,                                  // the vertices of both states
    D_DR = 30, D_JRG = 39, D_JVG = 48, D_JVA = 57, D_JPG = 66, D_JPA = 75, D_DVP = 84, D_DBG = 90,   // the float part, widened
    D_TH = 93, D_A1 = 96, D_ER = 105, D_JR = 114, D_INVJ = 123, D_T4 = 132, D_T5 = 141,              // the rotation chain
    D_E = 150, D_WE = 159, D_INFO = 168, D_SHARED = 249                                              // e, Omega*e, Omega
};

// ---- the prologue -----------------------------------------------------------------------------------------------------------------------
// what orbi_edge_information_device leaves for a refused edge: zeros, so entry 0 of its information tells
__device__ __forceinline__ bool edge_refused(const double *info, int e) { return info[81 * (size_t)e] == 0.0; }
// the head of record rec to H and the information of edge e to S[D_INFO ..).  No fence: the caller loads its vertices beside them and
// ends the phase with its WSYNC
__device__ __forceinline__ void edge_load(const orbi_record *bank, int rec, const double *info, int e, float *H, double *S, int lane)
{
    const float *recf = (const float *)(bank + rec);
    for (int k = lane; k < RH_WORDS; k += 64) H[k] = recf[k];
    for (int x = lane; x < 81; x += 64) S[D_INFO + x] = info[81 * (size_t)e + x];
}

// ---- behind the cast ----------------------------------------------------------------------------------------------------------------------
// dR, JRg, JVg, JVa, JPg, JPa, (dV, dP) and delta_bg from the record's head H and the temporaries T of bias_deltas to S.  Starts behind the
// WSYNC bias_deltas ends on (a caller may write fields of its own ahead of the call); ends on a WSYNC
__device__ __forceinline__ void edge_widen(const float *H, const float *T, double *S, int lane)
{
    const int g = lane / 9, q = lane - 9 * g;
    if (g == 0) S[D_DR + q] = (double)T[BD_DRU + q];
    else if (g < 6) S[D_JRG + 9 * (g - 1) + q] = (double)H[RH_JRG + 9 * (g - 1) + q];
    else if (g == 6 && q < 6) S[D_DVP + q] = (double)T[BD_DVP + q];
    else if (g == 6) S[D_DBG + q - 6] = (double)T[BD_DB + q - 6];
    WSYNC();
}
// er = LogSO3(dR(bg)^T * Rb1w * R2) to S[D_E .. D_E + 3), Jr = RightJacobianSO3(JRg*dbg) and invJr = InverseRightJacobianSO3(er).  Starts
// behind the WSYNC of edge_widen and uses lane groups 0 and 1: the caller's lines of that phase (ev and ep to S[D_E + 3 .. D_E + 9) among
// them) go ahead of the call on groups 2 .. 6, without a fence.  Ends on a WSYNC
__device__ __forceinline__ void edge_rotation(double *S, int lane)
{
    const int g = lane / 9, q = lane - 9 * g, i = q / 3, j = q - 3 * i;
    if (g == 0) S[D_A1 + q] = dm3tt(S + D_DR, S + D_R1, i, j);                    // dR^T * Rb1w
    else if (g == 1 && q < 3) S[D_TH + q] = dsum3(dmul(S[D_JRG + 3 * q], S[D_DBG]), dmul(S[D_JRG + 3 * q + 1], S[D_DBG + 1]), dmul(S[D_JRG + 3 * q + 2], S[D_DBG + 2]));
    WSYNC();
    if (g == 0) S[D_ER + q] = dm3(S + D_A1, S + D_R2, i, j);                      // eR
    else if (g == 1) S[D_JR + q] = dright_jacobian(S[D_TH], S[D_TH + 1], S[D_TH + 2], q);
    WSYNC();
    {   // LogSO3(eR) and InverseRightJacobianSO3(er), the scalars in every lane
        double er0, er1, er2;
        dlog_so3(S + D_ER, er0, er1, er2);
        if (g == 0) S[D_INVJ + q] = dinverse_right_jacobian(er0, er1, er2, q);
        else if (g == 1 && q < 3) S[D_E + q] = q == 0 ? er0 : q == 1 ? er1 : er2;
    }
    WSYNC();
}
// T4 = (-invJr)*eR^T and T5 = T4*Jr beside Omega*e to S[D_WE ..); returns chi2 = e^T*(Omega*e) in every lane.  Starts behind the WSYNC of
// edge_rotation with the whole of e in S[D_E ..) and uses lane groups 0 and 1: a caller's line on invJr goes ahead of the call on another
// group, without a fence.  Ends on a WSYNC
__device__ __forceinline__ double edge_chi2(double *S, int lane)
{
    const int g = lane / 9, q = lane - 9 * g, i = q / 3, j = q - 3 * i;
    if (g == 0) S[D_T4 + q] = dm3nt(S + D_INVJ, S + D_ER, i, j);
    else if (g == 1) {
        double s = 0.0;
        for (int k = 0; k < 9; ++k) s = s + dmul(S[D_INFO + 9 * q + k], S[D_E + k]);
        S[D_WE + q] = s;
    }
    WSYNC();
    if (g == 0) S[D_T5 + q] = dm3(S + D_T4, S + D_JR, i, j);
    WSYNC();
    double chi = 0.0;
    for (int k = 0; k < 9; ++k) chi = chi + dmul(S[D_E + k], S[D_WE + k]);
    return chi;
}

// ---- constructQuadraticForm on a 9 x C Jacobian J (row-major, in LDS), C = 15 per state of the edge ------------------------------------
// entry (ca, cb) of J^T*WJ
template <int C>
__device__ __forceinline__ double edge_jtwj(const double *J, const double *WJ, int ca, int cb)
{
    double s = 0.0;
    for (int k = 0; k < 9; ++k) s = s + dmul(J[C * k + ca], WJ[C * k + cb]);
    return s;
}
// WJ = w*(Omega*J) (LDS); the diagonal 15 x 15 blocks of J^T*WJ, one behind the other, to H; -J^T*(w*(Omega*e)) to b.  w is the weight of
// the robust kernel, 1.0 where there is none.  Starts behind a WSYNC with J, Omega and Omega*e in place; ends on no fence, with J and WJ
// readable: the block between the two states of an edge is its caller's (edge_jtwj), which has the walks to put there
template <int C>
__device__ __forceinline__ void edge_quadratic_form(const double *S, const double *J, double *WJ, double w, double *H, double *b, int lane)
{
    for (int x = lane; x < 9 * C; x += 64) {
        const int r = x / C, c = x - C * r;
        double s = 0.0;
        for (int k = 0; k < 9; ++k) s = s + dmul(S[D_INFO + 9 * r + k], J[C * k + c]);
        WJ[x] = dmul(w, s);
    }
    WSYNC();
    for (int x = lane; x < 15 * C; x += 64) {
        const int blk = x / 225, y = x - 225 * blk, r = y / 15, c = y - 15 * r;
        H[x] = edge_jtwj<C>(J, WJ, 15 * blk + r, 15 * blk + c);
    }
    if (lane < C) {
        double s = 0.0;
        for (int k = 0; k < 9; ++k) s = s + dmul(J[C * k + lane], dmul(w, S[D_WE + k]));
        b[lane] = -s;
    }
}

} // namespace
