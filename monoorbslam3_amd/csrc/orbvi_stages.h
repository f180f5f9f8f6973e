// The stages of one Levenberg-Marquardt iteration on the tracker's inertial graph as device functions: what a kernel of the staged calls
// (orbi_linearize_device: k_fac_edge, k_fac_gather; orbi_graph_oplus_device: k_fac_oplus; orbvi_linearize_device: k_vi_linearize;
// orbvi_solve_device: k_vi_solve) and the one-launch optimiser (orbvi_pose_optimize_device: k_vi_pose_loop of orbvi_loop.hip) both run.
// A kernel owns its LDS, its launch shape, its counters' flush and nothing else: every formula and every operation order that
// include/orbi.h and include/orbvi.h fix is here, once, so that a stage inside the loop gives the bytes of the staged call on the same
// input.  Internal: forced-inline device functions inside an anonymous namespace, so it adds no symbol.  A correction is made here, once.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/orbvi.h"
#include "orb_device.h"
#include "orb_math.h"
#include "orbba_camera.h"
#include "orbi_edge.h"
#include "orbi_factors_device.h"
#include "orbi_graph_device.h"
#include "orbi_so3.h"
#include "orbi_so3d.h"

#pragma clang fp contract(off)

namespace {

// ---- orbi_linearize_device ---------------------------------------------------------------------------------------------------------------
struct LinArgs {
    orbi_graph g;
    const orbi_record *bank;
    int cap;
    float gravity;
    const orbi_edge *edges;
    int n_edges;
    const double *info, *walk_info;
    const orbi_prior *priors;
    int n_priors;
    const orbi_prior_job *pjobs;
    int n_pjobs;
    double delta;
    int mode;
    double *work, *err, *chi2, *chi2_prior, *total, *H_diag, *H_off, *b, *J;
    float *flt;
    int32_t *result;
};

// the workspace of an edge: H_ii (225), H_jj (225), b_i (15), b_j (15), W_gyro*e_gyro (3), W_acc*e_acc (3), status, Huber weight
enum { W_HII = 0, W_HJJ = 225, W_B = 450, W_WALK = 480, W_STATUS = 486, W_RHO1 = 487 };
static_assert(W_RHO1 + 1 == ORBI_EDGE_WORK, "orbi_factors.h states the workspace of an edge");
enum { ST_OK = 0, ST_RANGE = 1, ST_REFUSED = 3 };   // == ORBI_R_DONE, ORBI_R_RANGE, ORBI_R_REFUSED

// EdgeInertial e by ONE WAVE in its slices S (D_WORDS doubles) and F (X_WORDS floats) of LDS: computeError, and in mode 0 linearizeOplus and
// constructQuadraticForm into the edge's workspace and d_H_off.  Wave-level fences only: no workgroup barrier
__device__ __forceinline__ void fac_edge_wave(const LinArgs &a, int mode, int e, double *S, float *F, int lane)
{
    double *work = a.work + (size_t)ORBI_EDGE_WORK * e;
    const int si = __builtin_amdgcn_readfirstlane(a.edges[e].i), sj = __builtin_amdgcn_readfirstlane(a.edges[e].j);
    const int rec = __builtin_amdgcn_readfirstlane(a.edges[e].rec), flags = __builtin_amdgcn_readfirstlane(a.edges[e].flags);
    const int g = lane / 9, q = lane - 9 * g, i = q / 3, j = q - 3 * i;
    int status = ST_OK;
    if (!edge_valid(si, sj, rec, a.g.n_states, a.cap)) status = ST_RANGE;
    else if (edge_refused(a.info, e)) status = ST_REFUSED;
    if (status != ST_OK) {
        if (lane < 9) a.err[9 * (size_t)e + lane] = 0.0;
        if (lane < 3) a.chi2[3 * (size_t)e + lane] = 0.0;
        if (a.flt && lane < 15) a.flt[15 * (size_t)e + lane] = 0.f;
        if (mode == 0) {
            for (int x = lane; x < 225; x += 64) a.H_off[225 * (size_t)e + x] = 0.0;
            if (a.J)
                for (int x = lane; x < 270; x += 64) a.J[270 * (size_t)e + x] = 0.0;
        }
        if (lane == 0) work[W_STATUS] = (double)status;
        return;
    }
    // ---- load: the head of the record, the vertices of both states, the information
    edge_load(a.bank, rec, a.info, e, F, S, lane);
    if (lane < 9) S[D_R1 + lane] = a.g.Rwb[9 * (size_t)si + lane];
    else if (lane < 18) S[D_R2 + lane - 9] = a.g.Rwb[9 * (size_t)sj + lane - 9];
    else if (lane < 21) S[D_T1 + lane - 18] = a.g.twb[3 * (size_t)si + lane - 18];
    else if (lane < 24) S[D_T2 + lane - 21] = a.g.twb[3 * (size_t)sj + lane - 21];
    else if (lane < 27) S[D_V1 + lane - 24] = a.g.v[3 * (size_t)si + lane - 24];
    else if (lane < 30) S[D_V2 + lane - 27] = a.g.v[3 * (size_t)sj + lane - 27];
    else if (lane < 33) S[D_B1 + lane - 30] = a.g.bg[3 * (size_t)si + lane - 30];
    else if (lane < 36) S[D_B1 + lane - 30] = a.g.ba[3 * (size_t)si + lane - 33];
    else if (lane < 39) S[D_B2 + lane - 36] = a.g.bg[3 * (size_t)sj + lane - 36];
    else if (lane < 42) S[D_B2 + lane - 36] = a.g.ba[3 * (size_t)sj + lane - 39];
    const int fix_i = a.g.fixed[si], fix_j = a.g.fixed[sj];
    WSYNC();
    // ---- the float part: the bias vertices cast to float, getDeltaRotation / Velocity / Position (Imu.cpp:182-192)
    bias_deltas(F, F + X_T, lane, lane < 6 ? (float)S[D_B1 + lane] : 0.f);
    if (a.flt && lane < 15) a.flt[15 * (size_t)e + lane] = lane < 9 ? F[X_T + BD_DRU + lane] : F[X_T + BD_DVP + lane - 9];
    // ---- everything behind the cast to double: this edge's lines on lane groups 2 .. 4, the rotation residual beside them
    const double dt = (double)F[RH_DT], G = (double)a.gravity;
    edge_widen(F, F + X_T, S, lane);
    edge_velocity_position(S, lane, G, dt);                                       // ev, ep and Rb1w*R2
    edge_rotation(S, lane);
    if (g == 2) S[D_T3 + q] = dm3nt(S + D_INVJ, S + D_R2, i, j);                  // (-invJr) * R2^T
    // ---- chi2, the Huber kernel (g2o's RobustKernelHuber), the walks
    const double chi = edge_chi2(S, lane);
    double rho1 = 1.0;
    if (a.delta > 0.0 && chi > dmul(a.delta, a.delta)) rho1 = a.delta / sqrt(chi);
    double we[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, wchi[2] = {0.0, 0.0};
    if (flags & ORBI_EDGE_WALKS) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const double *W = a.walk_info + 18 * (size_t)e + 9 * b;
            const double e0 = S[D_B2 + 3 * b] - S[D_B1 + 3 * b], e1 = S[D_B2 + 3 * b + 1] - S[D_B1 + 3 * b + 1], e2 = S[D_B2 + 3 * b + 2] - S[D_B1 + 3 * b + 2];
#pragma unroll
            for (int k = 0; k < 3; ++k) we[b][k] = dsum3(dmul(W[3 * k], e0), dmul(W[3 * k + 1], e1), dmul(W[3 * k + 2], e2));
            wchi[b] = dsum3(dmul(e0, we[b][0]), dmul(e1, we[b][1]), dmul(e2, we[b][2]));
        }
    }
    if (lane < 9) a.err[9 * (size_t)e + lane] = S[D_E + lane];
    if (lane < 3) a.chi2[3 * (size_t)e + lane] = lane == 0 ? chi : lane == 1 ? wchi[0] : wchi[1];
    if (lane == 0) work[W_STATUS] = (double)ST_OK, work[W_RHO1] = rho1;
    if (lane < 6) work[W_WALK + lane] = lane == 0 ? we[0][0] : lane == 1 ? we[0][1] : lane == 2 ? we[0][2] : lane == 3 ? we[1][0] : lane == 4 ? we[1][1] : we[1][2];
    if (mode != 0) return;
    // ---- the Jacobian: raw to d_J, with the columns of fixed dof zeroed to LDS
#pragma unroll
    for (int h = 0; h < 5; ++h) {
        const int x = lane + 64 * h;
        if (x < 270) {
            const int r = x / 30, c = x - 30 * r;
            const double v = jac_entry(S, dt, r, c);
            if (a.J) a.J[270 * (size_t)e + x] = v;
            S[D_J + x] = dof_fixed(c < 15 ? fix_i : fix_j, c < 15 ? c : c - 15) ? 0.0 : v;
        }
    }
    WSYNC();
    // W = rho1 * Omega: H_ii and H_jj, b_i and b_j to the workspace; H_ij, with the walks' -W, to d_H_off
    edge_quadratic_form<30>(S, S + D_J, S + D_WJ, rho1, work + W_HII, work + W_B, lane);
    for (int y = lane; y < 225; y += 64) {
        const int r = y / 15, c = y - 15 * r;
        double s = edge_jtwj<30>(S + D_J, S + D_WJ, r, 15 + c);
        if ((flags & ORBI_EDGE_WALKS) && r >= 9 && c >= 9 && r / 3 == c / 3 && !dof_fixed(fix_i, r) && !dof_fixed(fix_j, c))
            s = s - a.walk_info[18 * (size_t)e + 9 * (r / 3 - 3) + 3 * (r % 3) + c % 3];
        a.H_off[225 * (size_t)e + y] = s;
    }
}

// the diagonal block and the right-hand side of state s by ONE WAVE: the edges' blocks from their workspaces in ascending edge order, the
// walks beside them, the priors last
__device__ __forceinline__ void fac_gather_state(const LinArgs &a, int s, int lane)
{
    const int fixed = a.g.fixed[s];
    double h[4] = {0.0, 0.0, 0.0, 0.0}, bb = 0.0;       // entries lane + 64k of the 15 x 15 block; entry `lane` of b
    int hr[4], hc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) hr[k] = (lane + 64 * k) / 15, hc[k] = (lane + 64 * k) % 15;
    for (int c0 = 0; c0 < a.n_edges; c0 += 64) {
        const int e = c0 + lane;
        int side = 0;                                     // 1: this state is the edge's i, 2: its j
        if (e < a.n_edges && a.work[(size_t)ORBI_EDGE_WORK * e + W_STATUS] == (double)ST_OK) side = a.edges[e].i == s ? 1 : a.edges[e].j == s ? 2 : 0;
        unsigned long long mi = __ballot(side == 1), mj = __ballot(side == 2), m = mi | mj;
        while (m) {
            const int bit = __builtin_ctzll(m);
            m &= m - 1;
            const int ee = c0 + bit;
            const bool first = (mi >> bit) & 1;
            const double *w = a.work + (size_t)ORBI_EDGE_WORK * ee;
            const int fl = a.edges[ee].flags;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (lane + 64 * k < 225) h[k] = h[k] + w[(first ? W_HII : W_HJJ) + lane + 64 * k];
            if (lane < 15) bb = bb + w[W_B + (first ? 0 : 15) + lane];
            if (fl & ORBI_EDGE_WALKS) {                   // J = -I (first) / +I: H += W, b -= J^T * (W*e)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (lane + 64 * k < 225 && hr[k] >= 9 && hc[k] >= 9 && hr[k] / 3 == hc[k] / 3 && !dof_fixed(fixed, hr[k]))
                        h[k] = h[k] + a.walk_info[18 * (size_t)ee + 9 * (hr[k] / 3 - 3) + 3 * (hr[k] % 3) + hc[k] % 3];
                if (lane >= 9 && lane < 15 && !dof_fixed(fixed, lane)) bb = first ? bb + w[W_WALK + lane - 9] : bb - w[W_WALK + lane - 9];
            }
        }
    }
    for (int c0 = 0; c0 < a.n_pjobs; c0 += 64) {
        const int p = c0 + lane;
        bool hit = false;
        if (p < a.n_pjobs) hit = a.pjobs[p].state == s && a.pjobs[p].prior >= 0 && a.pjobs[p].prior < a.n_priors;
        unsigned long long m = __ballot(hit);
        while (m) {
            const int bit = __builtin_ctzll(m);
            m &= m - 1;
            const orbi_prior_job pj = a.pjobs[c0 + bit];
            const orbi_prior *pr = a.priors + pj.prior;
#pragma unroll
            for (int v = 0; v < 3; ++v) {                 // velocity, gyro, acc: e = priori - estimate, J = -I
                if (!((pj.mask >> v) & 1) || ((fixed >> (v + 1)) & 1)) continue;
                const float *Om = v == 0 ? pr->velo_info : (v == 1 || (pj.mask & ORBI_PRIOR_ACC_GYRO_INFO)) ? pr->gyro_info : pr->acc_info;
                const float *me = v == 0 ? pr->velo_priori : pr->bias_priori + 3 * (v - 1);
                const double *est = (v == 0 ? a.g.v : v == 1 ? a.g.bg : a.g.ba) + 3 * (size_t)s;
                const int base = 6 + 3 * v;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (lane + 64 * k < 225 && hr[k] >= base && hr[k] < base + 3 && hc[k] >= base && hc[k] < base + 3)
                        h[k] = h[k] + (double)Om[3 * (hr[k] - base) + hc[k] - base];
                if (lane >= base && lane < base + 3) {
                    const int r = lane - base;
                    bb = bb + dsum3(dmul((double)Om[3 * r], (double)me[0] - est[0]), dmul((double)Om[3 * r + 1], (double)me[1] - est[1]),
                                    dmul((double)Om[3 * r + 2], (double)me[2] - est[2]));
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (lane + 64 * k < 225) a.H_diag[225 * (size_t)s + lane + 64 * k] = h[k];
    if (lane < 15) a.b[15 * (size_t)s + lane] = bb;
}

// the priors' chi2, the counters of the call into s_cnt (eight ints of LDS, this wave's) and the totals in their one order, by ONE WAVE
// behind the edges.  The flush of s_cnt is the kernel's
__device__ __forceinline__ void fac_gather_tail(const LinArgs &a, int *s_cnt, int lane)
{
    if (lane < 8) s_cnt[lane] = 0;
    WSYNC();
    for (int p = lane; p < a.n_pjobs; p += 64) {
        const orbi_prior_job pj = a.pjobs[p];
        double c[3] = {0.0, 0.0, 0.0};
        const bool ok = pj.state >= 0 && pj.state < a.g.n_states && pj.prior >= 0 && pj.prior < a.n_priors;
        if (ok) {
            const orbi_prior *pr = a.priors + pj.prior;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                if (!((pj.mask >> v) & 1)) continue;
                const float *Om = v == 0 ? pr->velo_info : (v == 1 || (pj.mask & ORBI_PRIOR_ACC_GYRO_INFO)) ? pr->gyro_info : pr->acc_info;
                const float *me = v == 0 ? pr->velo_priori : pr->bias_priori + 3 * (v - 1);
                const double *est = (v == 0 ? a.g.v : v == 1 ? a.g.bg : a.g.ba) + 3 * (size_t)pj.state;
                const double e0 = (double)me[0] - est[0], e1 = (double)me[1] - est[1], e2 = (double)me[2] - est[2];
                double we[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) we[k] = dsum3(dmul((double)Om[3 * k], e0), dmul((double)Om[3 * k + 1], e1), dmul((double)Om[3 * k + 2], e2));
                c[v] = dsum3(dmul(e0, we[0]), dmul(e1, we[1]), dmul(e2, we[2]));
            }
        }
#pragma unroll
        for (int v = 0; v < 3; ++v) a.chi2_prior[3 * (size_t)p + v] = c[v];
        atomicAdd(&s_cnt[ok ? ORBI_R_PRIOR_DONE : ORBI_R_PRIOR_RANGE], 1);
    }
    for (int e = lane; e < a.n_edges; e += 64) atomicAdd(&s_cnt[(int)a.work[(size_t)ORBI_EDGE_WORK * e + W_STATUS]], 1);
    __threadfence();                                          // lane 0 reads what the other lanes wrote to d_chi2_prior
    WSYNC();
    if (lane == 0) {                                          // the totals in their one order
        double plain = 0.0, robust = 0.0;
        const double dsqr = dmul(a.delta, a.delta);
        for (int e = 0; e < a.n_edges; ++e) {
            const double c0 = a.chi2[3 * (size_t)e], c1 = a.chi2[3 * (size_t)e + 1], c2 = a.chi2[3 * (size_t)e + 2];
            const double r0 = (a.delta > 0.0 && c0 > dsqr) ? dmul(dmul(2.0, sqrt(c0)), a.delta) - dsqr : c0;
            plain = ((plain + c0) + c1) + c2;
            robust = ((robust + r0) + c1) + c2;
        }
        for (int p = 0; p < a.n_pjobs; ++p)
            for (int v = 0; v < 3; ++v) {
                const double c = a.chi2_prior[3 * (size_t)p + v];
                plain = plain + c, robust = robust + c;
            }
        a.total[0] = plain, a.total[1] = robust;
    }
}

// ---- orbi_graph_oplus_device: oplusImpl of state s by one thread; true when the state has a free vertex -----------------------------------
__device__ __forceinline__ bool fac_oplus_state(const orbi_graph &g, const double *dx, int32_t *iter, int s)
{
    const int fixed = g.fixed[s];
    const double *d = dx + 15 * (size_t)s;
    if (!(fixed & ORBI_FIX_POSE)) {   // CameraImuPose::update
        double R[9], E[9], N[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = g.Rwb[9 * (size_t)s + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) g.twb[3 * (size_t)s + k] = g.twb[3 * (size_t)s + k] + dsum3(dmul(R[3 * k], d[3]), dmul(R[3 * k + 1], d[4]), dmul(R[3 * k + 2], d[5]));
        dexp_so3(d[0], d[1], d[2], E);   // ExpSO3 returns NormalizeRotation(res)
#pragma unroll
        for (int k = 0; k < 9; ++k) N[k] = dm3(R, E, k / 3, k % 3);
        const int it = iter[s] + 1;
        if (it == 3) dnormalize(N);
        iter[s] = it == 3 ? 0 : it;
#pragma unroll
        for (int k = 0; k < 9; ++k) g.Rwb[9 * (size_t)s + k] = N[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!(fixed & ORBI_FIX_VELO)) g.v[3 * (size_t)s + k] = g.v[3 * (size_t)s + k] + d[6 + k];
        if (!(fixed & ORBI_FIX_GYRO)) g.bg[3 * (size_t)s + k] = g.bg[3 * (size_t)s + k] + d[9 + k];
        if (!(fixed & ORBI_FIX_ACC)) g.ba[3 * (size_t)s + k] = g.ba[3 * (size_t)s + k] + d[12 + k];
    }
    return (fixed & 15) != 15;
}

// ---- orbvi_linearize_device: a 1024-thread workgroup per group ---------------------------------------------------------------------------
constexpr int VI_T = 1024, VI_WAVES = VI_T / 64;
enum { S_PLAIN = 27, S_ROBUST = 28, VI_SUMS = 29 };    // behind quad_accumulate's 21 + 6
enum { P_RCW = 0, P_TCW = 9, P_RCB = 12, P_TBC = 21, P_WORDS = 24 };
enum { W_J = 0, W_W = 12, W_WE = 13, W_USED = 15 };   // an edge's workspace: J (2 x 6), w*Omega, (w*Omega)*e, 1.0 when the edge takes part
static_assert(W_USED + 1 == ORBVI_EDGE_WORK, "orbvi.h states the workspace of an edge");
enum { I_LO = 0, I_DUP = 1, I_INLIERS = 2, I_WORDS = 4 };

struct ViArgs {
    orbi_graph g;
    orbi_calib cal;
    BaCam cam;                      // delta: huber_delta
    int n_groups, cap_edges;
    const int32_t *group_state, *edge_off;
    const double *points, *z, *w;
    uint8_t *active;
    double threshold;
    int mode;
    double *work, *err, *chi2, *total, *H, *b;
    int32_t *n_inliers, *result;
};

// group g of the list by a workgroup of VI_T / VT threads, t the thread's index.  The header's order is written for VI_T threads; with VT > 1
// a thread does the work of the VT threads t, t + VI_T / VT, ... of those, one behind the other, each one's sums filed under its own wave
// (VI_T / VT is a multiple of 64: a lane stays a lane), so the bytes are those of VI_T threads.  s_part, s_pose (P_WORDS), s_cnt (8) and s_i (I_WORDS) are the workgroup's LDS.
// Workgroup barriers inside, every one in uniform control flow; returns behind one, with the call's counters in s_cnt: their flush
// is the kernel's
template <int VT>
__device__ __forceinline__ void vi_linearize_group(const ViArgs &a, int mode, int g, int t, double (&s_part)[VI_WAVES][VI_SUMS], double *s_pose, int *s_cnt, int *s_i)
{
    constexpr int RT = VI_T / VT;                 // the threads there are
    static_assert(RT % 64 == 0 && RT >= 64, "whole waves");
    const int lane = t & 63;
    if (t < 8) s_cnt[t] = 0;
    if (t < I_WORDS) s_i[t] = 0;
    __syncthreads();
    // the group's range: d_edge_off clamped and made non-decreasing; its state against the earlier groups'
    const int st = a.group_state[g];
    {
        int lo = 0, dup = 0;
        for (int k = t; k <= g; k += RT) {
            lo = max(lo, min(max(a.edge_off[k], 0), a.cap_edges));
            if (k < g && a.group_state[k] == st) dup = 1;
        }
        lo = wave_max(lo), dup = wave_max(dup);
        if (lane == 0) {
            if (lo) atomicMax(&s_i[I_LO], lo);
            if (dup) atomicOr(&s_i[I_DUP], 1);
        }
    }
    __syncthreads();
    const int lo = s_i[I_LO], hi = max(lo, min(max(a.edge_off[g + 1], 0), a.cap_edges));
    const int code = (st < 0 || st >= a.g.n_states) ? ORBI_R_RANGE : s_i[I_DUP] ? ORBI_R_DUPLICATE : ORBI_R_DONE;
    if (t == 0) s_cnt[code] = 1;
    if (code != ORBI_R_DONE) {        // uniform: a dropped group leaves zeros
        for (int e = lo + t; e < hi; e += RT) a.err[2 * (size_t)e] = 0.0, a.err[2 * (size_t)e + 1] = 0.0, a.chi2[e] = 0.0;
        if (t < 2 && mode != 2) a.total[2 * (size_t)g + t] = 0.0;
        if (t == 0 && mode == 2) a.n_inliers[g] = 0;
        __syncthreads();
        return;
    }
    // the pose the edges hang on, derived from (R_wb, t_wb) on every call, and the calibration widened
    if (t < 9) {
        s_pose[P_RCW + t] = pose_rcw(a.cal, a.g.Rwb + 9 * (size_t)st, t);
        s_pose[P_RCB + t] = (double)a.cal.Rcb[t];
    } else if (t < 12) s_pose[P_TBC + t - 9] = pose_tbc(a.cal, t - 9);
    __syncthreads();
    if (t < 3) s_pose[P_TCW + t] = pose_tcw(a.cal, s_pose + P_RCW, a.g.twb + 3 * (size_t)st, t);
    __syncthreads();
    const bool accumulate = mode == 0 && !(a.g.fixed[st] & ORBI_FIX_POSE);
    int n_bad = 0, n_in = 0;
#pragma unroll
    for (int v = 0; v < VT; ++v) {                // thread tv of the VI_T
        const int tv = t + v * RT;
        double plain = 0.0, robust = 0.0;
        for (int e = lo + tv; e < hi; e += VI_T) {
            double *work = a.work + (size_t)ORBVI_EDGE_WORK * e;
            if (accumulate) work[W_USED] = 0.0;
            // the trip count is 1 to 3: nothing is worth hoisting out of this loop, and what the compiler hoists (the pose, the camera's
            // constants negated and scaled) it then spills.  An opaque copy per trip keeps the pose in LDS and the camera in SGPRs.
            const double *pose = s_pose;
            BaCam cam = a.cam;
            asm volatile("" : "+v"(pose));
            asm volatile("" : "+s"(cam.fx), "+s"(cam.fy), "+s"(cam.cx), "+s"(cam.cy), "+s"(cam.k[0]), "+s"(cam.k[1]), "+s"(cam.k[2]), "+s"(cam.k[3]));
            const double *R = pose + P_RCW;
            const double Px = a.points[3 * (size_t)e], Py = a.points[3 * (size_t)e + 1], Pz = a.points[3 * (size_t)e + 2];
            const double X = dsum3(R[0] * Px, R[1] * Py, R[2] * Pz) + pose[P_TCW];
            const double Y = dsum3(R[3] * Px, R[4] * Py, R[5] * Pz) + pose[P_TCW + 1];
            const double Z = dsum3(R[6] * Px, R[7] * Py, R[8] * Pz) + pose[P_TCW + 2];
            double u, v;
            ba_project(cam, X, Y, Z, &u, &v);
            const double ex = a.z[2 * (size_t)e] - u, ey = a.z[2 * (size_t)e + 1] - v;
            const double om = a.w[e];
            const double chi = om * (ex * ex + ey * ey);
            a.err[2 * (size_t)e] = ex, a.err[2 * (size_t)e + 1] = ey;
            a.chi2[e] = chi;
            const bool finite = isfinite(ex) && isfinite(ey) && isfinite(chi);
            if (mode == 2) {
                const bool in = !(chi > a.threshold);
                a.active[e] = in ? 1 : 0;
                n_in += in, n_bad += !finite;
                continue;
            }
            if (a.active && !a.active[e]) continue;
            if (!finite) {
                ++n_bad;
                continue;
            }
            double rho, rw;
            huber(chi, cam.delta, rho, rw);
            plain = plain + chi, robust = robust + rho;
            if (!accumulate) continue;
            // left for the next pass: the weights and Pc (in the Jacobian's first slots)
            const double W = rw * om;
            work[W_W] = W, work[W_WE] = W * ex, work[W_WE + 1] = W * ey, work[W_USED] = 1.0;
            work[W_J] = X, work[W_J + 1] = Y, work[W_J + 2] = Z;
        }
        // Three passes, each thread over its own edges and through its own workspace rows: the camera's Jacobian (the Kannala-Brandt one
        // with its atan2 is the largest block of the kernel) is live neither beside the projection nor beside the 27 sums.
        // linearizeOplus, Pc replaced by the Jacobian
        for (int e = lo + tv; accumulate && e < hi; e += VI_T) {
            double *work = a.work + (size_t)ORBVI_EDGE_WORK * e;
            if (work[W_USED] == 0.0) continue;
            const double *pose = s_pose;
            BaCam cam = a.cam;
            asm volatile("" : "+v"(pose));
            asm volatile("" : "+s"(cam.fx), "+s"(cam.fy), "+s"(cam.cx), "+s"(cam.cy), "+s"(cam.k[0]), "+s"(cam.k[1]), "+s"(cam.k[2]), "+s"(cam.k[3]));
            const double X = work[W_J], Y = work[W_J + 1], Z = work[W_J + 2];
            double Jp[6];
            ba_proj_jacobian(cam, X, Y, Z, Jp);
            pose_jacobian(pose + P_RCB, pose + P_TBC, Jp, X, Y, Z, work + W_J);
        }
        double acc[VI_SUMS];
    #pragma unroll
        for (int k = 0; k < VI_SUMS; ++k) acc[k] = 0.0;
        acc[S_PLAIN] = plain, acc[S_ROBUST] = robust;
        if (accumulate) {
            for (int e = lo + tv; e < hi; e += VI_T) {
                const double *work = a.work + (size_t)ORBVI_EDGE_WORK * e;
                if (work[W_USED] == 0.0) continue;
                quad_accumulate(work + W_J, work[W_W], work[W_WE], work[W_WE + 1], acc);
            }
        }
        block_sums_put(acc, s_part, accumulate ? 0 : S_PLAIN, VI_SUMS, tv >> 6);
    }
    block_add(s_cnt, ORBVI_R_NONFINITE, n_bad);
    block_add(s_i, I_INLIERS, n_in);
    __syncthreads();
    if (t < VI_SUMS && mode != 2 && (t >= S_PLAIN || accumulate)) {
        const double s = block_sums_get(s_part, t);
        if (t >= S_PLAIN) a.total[2 * (size_t)g + t - S_PLAIN] = s;
        else quad_scatter(t, s, a.H + 225 * (size_t)st, a.b + 15 * (size_t)st);
    }
    if (t == 0 && mode == 2) a.n_inliers[g] = s_i[I_INLIERS];
}

// ---- orbvi_solve_device: one workgroup assembles, one wave factorises ------------------------------------------------------------------
constexpr int SV_N = 15 * ORBVI_MAX_STATES, SV_LD = SV_N + 1;   // a row stride of 61 doubles spreads a column over the banks

// H of n states into s_A (SV_N x SV_LD doubles of LDS) by a workgroup of T >= 225 threads, t the thread's index, the identity rows of the fixed dof included;
// s_fix (SV_N ints): the fixed flag per dof; s_cnt (8 ints): zeroed, then ORBI_R_RANGE counts the skipped blocks.  Workgroup barriers
// inside, every one in uniform control flow; returns behind one
template <int T>
__device__ __forceinline__ void vi_solve_assemble(int t, int n, const uint8_t *__restrict__ fixed, const orbi_edge *__restrict__ edges, int n_edges, int cap,
                                                  const double *__restrict__ H_diag, const double *__restrict__ H_off, double *s_A, int *s_fix, int *s_cnt)
{
    static_assert(T >= 225, "a thread per entry of an off-diagonal block");
    const int N = 15 * n;
    for (int x = t; x < SV_N * SV_LD; x += T) s_A[x] = 0.0;
    if (t < 8) s_cnt[t] = 0;
    if (t < N) s_fix[t] = dof_fixed(fixed[t / 15], t % 15);
    __syncthreads();
    for (int x = t; x < 225 * n; x += T) {
        const int s = x / 225, y = x - 225 * s, r = y / 15, c = y - 15 * r;
        s_A[(15 * s + r) * SV_LD + 15 * s + c] = H_diag[x];
    }
    __syncthreads();
    for (int e = 0; e < n_edges; ++e) {          // ascending: several edges on one pair add up in edge order
        const int i = edges[e].i, j = edges[e].j;
        if (!edge_valid(i, j, edges[e].rec, n, cap)) {   // uniform
            if (t == 0) ++s_cnt[ORBI_R_RANGE];
            continue;
        }
        if (t < 225) {
            const int r = t / 15, c = t - 15 * r;
            const double v = H_off[225 * (size_t)e + t];
            double *p = s_A + (15 * i + r) * SV_LD + 15 * j + c, *q = s_A + (15 * j + c) * SV_LD + 15 * i + r;
            *p = *p + v, *q = *q + v;
        }
        __syncthreads();
    }
    for (int x = t; x < N * N; x += T) {       // a fixed dof is an identity row and column
        const int r = x / N, c = x - N * r;
        if (s_fix[r] || s_fix[c]) s_A[r * SV_LD + c] = r == c ? 1.0 : 0.0;
    }
    __syncthreads();
}

// lane i of ONE wave on row i of the assembled s_A: the largest H_jj over the free dof before damping, 0 when none is larger -- what
// computeLambdaInit multiplies by tau -- in every lane
__device__ __forceinline__ double vi_solve_largest(int N, const double *s_A, const int *s_fix, int i)
{
    const bool in = i < N, fre = in && !s_fix[in ? i : 0];
    const double hjj = in ? s_A[i * SV_LD + i] : 0.0;
    return wave_max(fre && hjj > 0.0 ? hjj : 0.0);
}

// the damped Cholesky and the substitutions by ONE wave, a lane per row, wave-level fences only: dx (N doubles), out[0] (computeScale
// without its + 1e-3) and out[2] (the smallest pivot, or the one that refused).  s_v is SV_N doubles of LDS.  True when the solve was
// refused (the same in every lane): dx is then all zero and out[0] is 0
__device__ __forceinline__ bool vi_solve_wave(int N, const double *__restrict__ b, double lam, double *__restrict__ dx, double *__restrict__ out,
                                              double *s_A, double *s_v, const int *s_fix, int i)
{
    const bool in = i < N, fre = in && !s_fix[in ? i : 0];
    const double hjj = in ? s_A[i * SV_LD + i] : 0.0;
    const double bi = fre ? b[i] : 0.0;
    wave_order();
    if (fre) s_A[i * SV_LD + i] = hjj + lam;
    wave_order();
    bool refused = false;
    double pivot = INFINITY, my_r = 0.0;
    for (int j = 0; j < N; ++j) {
        double v = 0.0;
        if (in && i >= j) {
            double s = 0.0;
            for (int k = 0; k < j; ++k) s = s + s_A[i * SV_LD + k] * s_A[j * SV_LD + k];
            v = s_A[i * SV_LD + j] - s;
        }
        const double d = __shfl(v, j);
        if (!(d > 0.0) || !isfinite(d)) {         // the same in every lane
            refused = true, pivot = d;
            break;
        }
        pivot = d < pivot ? d : pivot;
        const double l = sqrt(d), r = 1.0 / l;
        wave_order();
        if (i == j) s_A[i * SV_LD + j] = l, my_r = r;
        else if (in && i > j) s_A[i * SV_LD + j] = v * r;
        wave_order();
    }
    double x = 0.0;
    if (!refused) {
        double s = 0.0, y = 0.0;
        for (int k = 0; k < N; ++k) {             // forward: y_i = (b_i - sum_{k<i} l_ik*y_k)*r_i, k ascending
            const double yk = __shfl((bi - s) * my_r, k);
            if (i == k) y = yk;
            if (in && i > k) s = s + s_A[i * SV_LD + k] * yk;
        }
        s = 0.0;
        for (int k = N - 1; k >= 0; --k) {        // backward: x_i = (y_i - sum_{k>i} l_ki*x_k)*r_i, k descending
            const double xk = __shfl((y - s) * my_r, k);
            if (i == k) x = xk;
            if (in && i < k) s = s + s_A[k * SV_LD + i] * xk;
        }
    }
    if (in) dx[i] = x, s_v[i] = x * (lam * x + bi);
    wave_order();
    if (i == 0) {
        double s = 0.0;
        for (int k = 0; k < N; ++k) s = s + s_v[k];
        out[0] = refused ? 0.0 : s, out[2] = pivot;
    }
    return refused;
}

// ---- orbil_chain_solve_device: the damped step of a chain, by a walk along its band -----------------------------------------------------
// H of a chain is block-tridiagonal, and so is its Cholesky factor.  THE BAND (CS_BAND * n doubles of device memory, the caller's):
// row i of the 15n has CS_ROW = 30 doubles, the columns of the block before its own (0 .. 14; zeros for block 0) and of its own (15 .. 29).
// The assembly leaves A there without the damping, the walk replaces it by L, block column by block column: the 30 rows of blocks s and
// s + 1 are one wave's tile in LDS (a lane per row), which it loads from the band, factorises as vi_solve_wave does a matrix, and stores
// back; the backward substitution reads the finished blocks from the band behind the wave's fence.  The terms the dense order adds
// outside the band are products with an exact zero, so for finite values the bytes are vi_solve_wave's.
constexpr int CS_MAX_STATES = 20, CS_N = 15 * CS_MAX_STATES, CS_ROW = 30, CS_BAND = 15 * CS_ROW;   // CS_BAND doubles of band per state
constexpr int CS_LD = CS_ROW + 1;                                                                   // a tile row's stride: 31 spreads a column over the banks
constexpr int CS_TILE = 2 * 15 * CS_LD;                                                             // two blocks of rows, by the parity of the block

// H of n states into the band by a workgroup of T >= 225 threads, t the thread's index, the identity rows and columns of the fixed dof
// included, the damping not.  An edge takes part under edge_valid() when its states are neighbours; any other is skipped and counted:
// s_cnt (8 ints) is zeroed, then ORBI_R_RANGE counts them.  s_fix (CS_N ints): the fixed flag per dof.  Workgroup barriers inside, every
// one in uniform control flow; returns behind one
template <int T>
__device__ __forceinline__ void chain_solve_assemble(int t, int n, const uint8_t *__restrict__ fixed, const orbi_edge *__restrict__ edges, int n_edges, int cap,
                                                     const double *__restrict__ H_diag, const double *__restrict__ H_off, double *band, int *s_fix, int *s_cnt)
{
    static_assert(T >= 225, "a thread per entry of an off-diagonal block");
    const int N = 15 * n;
    if (t < 8) s_cnt[t] = 0;
    for (int i = t; i < N; i += T) s_fix[i] = dof_fixed(fixed[i / 15], i % 15);
    for (int x = t; x < CS_ROW * N; x += T) {
        const int i = x / CS_ROW, q = x - CS_ROW * i;
        band[x] = q < 15 ? 0.0 : H_diag[225 * (size_t)(i / 15) + 15 * (i % 15) + q - 15];
    }
    __syncthreads();
    for (int e = 0; e < n_edges; ++e) {          // ascending: several edges on one pair add up in edge order
        const int i = edges[e].i, j = edges[e].j;
        if (!edge_valid(i, j, edges[e].rec, n, cap) || (i - j != 1 && j - i != 1)) {   // uniform
            if (t == 0) ++s_cnt[ORBI_R_RANGE];
            continue;
        }
        if (t < 225) {                             // the block below the diagonal: the transpose of (i, j) when j is the later state
            const int r = t / 15, c = t - 15 * r;
            double *p = j > i ? band + (size_t)CS_ROW * (15 * j + c) + r : band + (size_t)CS_ROW * (15 * i + r) + c;
            *p = *p + H_off[225 * (size_t)e + t];
        }
        __syncthreads();
    }
    for (int x = t; x < CS_ROW * N; x += T) {      // a fixed dof is an identity row and column
        const int i = x / CS_ROW, q = x - CS_ROW * i, j = 15 * (i / 15) + q - 15;
        if (j >= 0 && (s_fix[i] || s_fix[j])) band[x] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
}

// ONE wave on the assembled band: the largest H_jj over the free dof before damping, 0 when none is larger, in every lane
__device__ __forceinline__ double chain_solve_largest(int N, const double *band, const int *s_fix, int lane)
{
    double m = 0.0;
    for (int i = lane; i < N; i += 64) {
        const double hjj = band[(size_t)CS_ROW * i + 15 + i % 15];
        if (!s_fix[i] && hjj > m) m = hjj;
    }
    return wave_max(m);
}

// the damped Cholesky along the band and the substitutions by ONE wave, wave-level fences only: dx (15n doubles), out[0] (computeScale
// without its + 1e-3) and out[2] (the smallest pivot, or the one that refused), in vi_solve_wave's orders: columns ascending, each inner
// sum ascending over the columns of the band, one sqrt and one reciprocal per column, the forward substitution ascending, the backward one
// descending, computeScale ascending over all 15n rows.  s_T (CS_TILE doubles), s_y, s_r and s_v (CS_N doubles each) are LDS.  True when
// the solve was refused (the same in every lane): dx is then all zero and out[0] is 0
__device__ __forceinline__ bool chain_solve_wave(int n, const double *__restrict__ b, double lam, double *__restrict__ dx, double *__restrict__ out, double *band,
                                                 double *s_T, double *s_y, double *s_r, double *s_v, const int *s_fix, int lane)
{
    const int N = 15 * n;
    const bool mine = lane < 15;                              // a row of block s; lanes 15 .. 29 have the rows of block s + 1
    bool refused = false;
    double pivot = INFINITY;
    for (int s = 0; s < n && !refused; ++s) {                 // block column s: uniform
        const bool theirs = lane >= 15 && lane < 30 && s + 1 < n;
        wave_order();
        for (int blk = s == 0 ? 0 : s + 1; blk <= s + 1 && blk < n; ++blk) {   // the rows that enter the tile, damped
            double *T = s_T + (blk & 1) * 15 * CS_LD;
            for (int x = lane; x < CS_BAND; x += 64) {
                const int r = x / CS_ROW, q = x - CS_ROW * r, i = 15 * blk + r;
                const double v = band[(size_t)CS_ROW * i + q];
                T[r * CS_LD + q] = (q == 15 + r && !s_fix[i]) ? v + lam : v;
            }
        }
        wave_order();
        // a lane keeps its row in registers: w[k] is column k of the tile for a row of block s; a row of block s + 1 has its 15 columns of
        // block s in w[15 ..) behind 15 zeros, so that one sum serves both -- the zeros add nothing to a sum that starts at +0.  LDS holds the
        // rows of block s, which every lane reads as the column's row of L, a broadcast
        double *own = s_T + (s & 1) * 15 * CS_LD, *nxt = s_T + ((s + 1) & 1) * 15 * CS_LD;
        double w[CS_ROW];
#pragma unroll
        for (int k = 0; k < CS_ROW; ++k) w[k] = mine ? own[lane * CS_LD + k] : (theirs && k >= 15) ? nxt[(lane - 15) * CS_LD + k - 15] : 0.0;
        double my_r = 0.0;
#pragma unroll
        for (int c = 0; c < 15; ++c) {                        // column 15s + c; its row of L is own + c * CS_LD.  Unrolled whole: w stays in registers
            if (refused) continue;                            // the same in every lane: nothing behind the pivot that refused
            const double *rc = own + c * CS_LD;
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < 15 + c; ++k) a = a + w[k] * rc[k];
            const double v = w[15 + c] - a;
            const double d = __shfl(v, c);
            if (!(d > 0.0) || !isfinite(d)) {                 // the same in every lane
                refused = true, pivot = d;
                continue;
            }
            pivot = d < pivot ? d : pivot;
            const double l = sqrt(d), r = 1.0 / l;
            wave_order();
            if (lane == c) w[15 + c] = l, my_r = r;
            else if ((mine && lane > c) || theirs) w[15 + c] = v * r;
            if (mine && lane >= c) own[lane * CS_LD + 15 + c] = w[15 + c];
            wave_order();
        }
        if (refused) break;
        // forward: y_i = (b_i - sum_{k<i} l_ik*y_k)*r_i, k ascending: the block before, then this one
        const int i = 15 * s + (mine ? lane : 0);
        const double bi = mine && !s_fix[i] ? b[i] : 0.0;
        double a = 0.0, y = 0.0;
        if (mine && s > 0) {
#pragma unroll
            for (int k = 0; k < 15; ++k) a = a + w[k] * s_y[15 * (s - 1) + k];
        }
#pragma unroll
        for (int k = 0; k < 15; ++k) {
            const double yk = __shfl((bi - a) * my_r, k);
            if (lane == k) y = yk;
            if (mine && lane > k) a = a + w[15 + k] * yk;
        }
        if (mine) s_y[i] = y, s_r[i] = my_r;
        if (theirs) {                                         // L[s+1,s], the first 15 columns of the next step's rows
#pragma unroll
            for (int k = 0; k < 15; ++k) nxt[(lane - 15) * CS_LD + k] = w[15 + k];
        }
        wave_order();
        for (int x = lane; x < CS_BAND; x += 64) {            // the finished rows of block s back to the band
            const int r = x / CS_ROW, q = x - CS_ROW * r;
            band[(size_t)CS_ROW * (15 * s + r) + q] = own[r * CS_LD + q];
        }
    }
    if (!refused) {
        __threadfence();                                      // a lane reads what the other lanes wrote to the band
        wave_order();
        for (int s = n - 1; s >= 0; --s) {                    // backward: x_i = (y_i - sum_{k>i} l_ki*x_k)*r_i, k descending
            const int i = 15 * s + (mine ? lane : 0);
            const double y = mine ? s_y[i] : 0.0, my_r = mine ? s_r[i] : 0.0;
            double a = 0.0, x = 0.0;
            double below[15], within[15];                     // column `lane` of L[s+1,s] and of L[s,s]: the loads ahead of the chain of sums
#pragma unroll
            for (int k = 0; k < 15; ++k) {
                below[k] = mine && s + 1 < n ? band[(size_t)CS_ROW * (15 * (s + 1) + k) + lane] : 0.0;
                within[k] = mine ? band[(size_t)CS_ROW * (15 * s + k) + 15 + lane] : 0.0;
            }
            if (mine && s + 1 < n) {
#pragma unroll
                for (int k = 14; k >= 0; --k) a = a + below[k] * s_y[15 * (s + 1) + k];
            }
#pragma unroll
            for (int k = 14; k >= 0; --k) {
                const double xk = __shfl((y - a) * my_r, k);
                if (lane == k) x = xk;
                if (mine && lane < k) a = a + within[k] * xk;
            }
            wave_order();
            if (mine) s_y[i] = x;                             // x takes the place of y
            wave_order();
        }
    }
    for (int i = lane; i < N; i += 64) {
        const double x = refused ? 0.0 : s_y[i], bi = s_fix[i] ? 0.0 : b[i];
        dx[i] = x, s_v[i] = x * (lam * x + bi);
    }
    wave_order();
    if (lane == 0) {
        double a = 0.0;
        for (int k = 0; k < N; ++k) a = a + s_v[k];
        out[0] = refused ? 0.0 : a, out[2] = pivot;
    }
    return refused;
}

} // namespace
