// The steps of the IMU initialisation on the device (include/orbii.h):
//   orbii_prior_device        the gravity direction and the velocities ahead of it          LocalMapping.cpp:391-407
//   orbii_graph_init_device   the vertices and the edges' constants                         Optimize.cpp:110-153, G2oTypes.cpp:71-82
//   orbii_linearize_device    computeError, linearizeOplus, constructQuadraticForm          G2oTypes.cpp:94-163, :186-246, G2oTypes.h:324-343
//   orbii_damp_device         the damped copy of the system, the largest diagonal entry     (g2o's setLambda, computeLambdaInit)
//   orbii_oplus_device        oplusImpl of the four kinds of vertex                         G2oTypes.h:80-87, :185-205
//   orbii_recover_device      step 4                                                        Optimize.cpp:186-204
//
// The float part of an edge is orbi_imu.hip's arithmetic from the shared orbi_so3.h (bias_deltas, the call k_fac_edge makes); the double
// SO(3) functions are orbi_so3d.h's, shared with orbi_factors.hip.  Everything behind the cast is IEEE double, +, -, *, / in the header's
// orders without fused multiply-add.  What EdgeInertialGS / EdgeInertialG have in common with EdgeInertial (k_fac_edge) -- the widening,
// the rotation residual and its Jacobian factor, Omega*e with chi2, the quadratic form, the refused-edge rule -- is orbi_edge.h's; ev,
// ep (scale, gravity direction, Oc / Pcb) and the Jacobian's entries are here.
//
// Shape: at most 157 key frames and 480 unknowns, so every kernel is latency-bound and the aim is few launches.  An edge is ONE WAVE, four
// per workgroup (k_fac_edge's shape): its constants, the 3x3 temporaries, the 9x15 Jacobian, the 9x9 information and their product live
// in the wave's own slice of LDS, the lanes are spread over matrix entries and the phases are separated by wave-level fences only.  The
// edge leaves J^T*Omega*J and -J^T*Omega*e in the caller's workspace; then ONE THREAD PER ENTRY of the dense system adds up the entry's
// edges in ascending edge order, the priors last, so no floating-point atomic is needed and the same input gives the same bytes.  The
// first workgroup of that launch computes the priors' chi2, the total and d_result in their one order.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "../../include/orbii.h"
#include "../../include/orbx.h"
#include "orb_host.h"
#include "orb_math.h"
#include "orbi_edge.h"
#include "orbi_graph_device.h"
#include "orbi_so3.h"
#include "orbi_so3d.h"

#pragma clang fp contract(off)

static_assert(sizeof(orbii_graph) == 64 && sizeof(orbii_bias) == 24 && sizeof(orbi_edge) == 16 && sizeof(orbi_prior) == 144, "orbii.h fixes these layouts");
static_assert(ORBII_N(ORBII_MAX_KF) == 480 && ORBII_N(2) == 15 && ORBII_N(3) == 30 && ORBII_N(17) == 60, "N = 15 * ceil((9 + 3 n_kf) / 15)");

namespace {

constexpr int II_WAVES = 4, II_T = 64 * II_WAVES, II_JOB = 4;
enum { SH_BG = ORBII_SHARED_BG, SH_BA = ORBII_SHARED_BA, SH_RWG = ORBII_SHARED_RWG, SH_SCALE = ORBII_SHARED_SCALE, SH_WORDS = 16 };

__device__ __forceinline__ bool dof_free(int d, int n_kf, int kind) { return d < 9 + 3 * n_kf && !(kind == ORBII_KIND_G && d == 8); }

// ---- orbii_prior_device: one wave -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_ii_prior(const double *__restrict__ pose_R, const double *__restrict__ pose_t, int n_pose, float *state, int n_src,
                                                 const orbi_record *__restrict__ bank, int cap, orbi_prior *priors, int n_priors,
                                                 const int32_t *__restrict__ jobs, int n, double *__restrict__ Rwg, int32_t *__restrict__ result)
{
    __shared__ int s_code[ORBII_MAX_KF], s_next[ORBII_MAX_KF], s_misc[8];
    __shared__ float s_O[3 * ORBII_MAX_KF], s_RdV[3 * ORBII_MAX_KF], s_dt[ORBII_MAX_KF], s_w[3], s_W[9];
    const int lane = threadIdx.x;
    // the jobs that take part; per job the camera centre and Rwb*dVu
    for (int k = lane; k < n; k += 64) {
        const int pr = jobs[II_JOB * k], sr = jobs[II_JOB * k + 1], rec = jobs[II_JOB * k + 2], sl = jobs[II_JOB * k + 3];
        int code = ORBI_R_DONE;
        if (pr < 0 || pr >= n_pose || sr < 0 || sr >= n_src || sl < 0 || sl >= n_priors || rec < (k == n - 1 ? -1 : 0) || rec >= cap) code = ORBI_R_RANGE;
        else if (job_named_before(jobs, II_JOB, k, 1, sr, 3, sl)) code = ORBI_R_DUPLICATE;
        s_code[k] = code;
        float O[3] = {0.f, 0.f, 0.f}, RdV[3] = {0.f, 0.f, 0.f}, dt = 0.f;
        if (code == ORBI_R_DONE) {
            float R[9], t[3];
#pragma unroll
            for (int e = 0; e < 9; ++e) R[e] = (float)pose_R[9 * (size_t)pr + e];
#pragma unroll
            for (int e = 0; e < 3; ++e) t[e] = (float)pose_t[3 * (size_t)pr + e];
#pragma unroll
            for (int e = 0; e < 3; ++e) O[e] = sum3(mul(-R[e], t[0]), mul(-R[3 + e], t[1]), mul(-R[6 + e], t[2]));
            if (rec >= 0) {
                const float *h = (const float *)(bank + rec), *Rwb = state + 15 * (size_t)sr;
                float dVu[3], Rw[9];
#pragma unroll
                for (int e = 0; e < 3; ++e) dVu[e] = add(add(h[RH_DV + e], mv3(h + RH_JVG, h + RH_DELTA, e)), mv3(h + RH_JVA, h + RH_DELTA + 3, e));
#pragma unroll
                for (int e = 0; e < 9; ++e) Rw[e] = Rwb[e];
#pragma unroll
                for (int e = 0; e < 3; ++e) RdV[e] = mv3(Rw, dVu, e);
                dt = h[RH_DT];
            }
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) s_O[3 * k + e] = O[e], s_RdV[3 * k + e] = RdV[e];
        s_dt[k] = dt;
    }
    WSYNC();
    // the chain of the jobs kept, the counts and the sequential sum, by one lane
    if (lane == 0) {
        int prev = -1, before = -1, cnt[4] = {0, 0, 0, 0};
        float dir[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < n; ++k) {
            const int code = s_code[k];
            ++cnt[code];
            if (code != ORBI_R_DONE) continue;
            s_next[k] = -1;
            if (prev >= 0) {
                s_next[prev] = k;
#pragma unroll
                for (int e = 0; e < 3; ++e) dir[e] = sub(dir[e], s_RdV[3 * prev + e]);
            }
            before = prev, prev = k;
        }
        const float nrm = sqrtf(sum3(mul(dir[0], dir[0]), mul(dir[1], dir[1]), mul(dir[2], dir[2])));
        if (nrm > 0.f) {
#pragma unroll
            for (int e = 0; e < 3; ++e) dir[e] = dvd(dir[e], nrm);
        }
        const float v[3] = {dir[1], -dir[0], 0.f};
        const float nv = sqrtf(sum3(mul(v[0], v[0]), mul(v[1], v[1]), mul(v[2], v[2])));
        const bool refused = nv == 0.f;
        const float theta = (float)asin((double)nv);
#pragma unroll
        for (int e = 0; e < 3; ++e) s_w[e] = refused ? 0.f : dvd(mul(theta, v[e]), nv);
        s_misc[0] = prev, s_misc[1] = before, s_misc[2] = refused;
        result[ORBI_R_DONE] = cnt[ORBI_R_DONE], result[ORBI_R_RANGE] = cnt[ORBI_R_RANGE], result[ORBI_R_DUPLICATE] = cnt[ORBI_R_DUPLICATE];
        result[ORBI_R_REFUSED] = refused;
        result[4] = result[5] = result[6] = result[7] = 0;
    }
    WSYNC();
    const int last = s_misc[0], before = s_misc[1];
    // the velocities: a key frame with a successor from its own pair, the last one from its predecessor's
    for (int k = lane; k < n; k += 64) {
        if (s_code[k] != ORBI_R_DONE) continue;
        const int a = k == last ? before : k;
        if (a < 0) continue;                       // a single key frame: no pair
        const int b = s_next[a], sr = jobs[II_JOB * k + 1], sl = jobs[II_JOB * k + 3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const float velo = dvd(sub(s_O[3 * b + e], s_O[3 * a + e]), s_dt[a]);
            state[15 * (size_t)sr + 12 + e] = velo;
            priors[sl].velo_priori[e] = velo;
        }
    }
    // Rwg = ExpSO3f(w), the identity when refused
    const float wx = s_w[0], wy = s_w[1], wz = s_w[2];
    const So3 so = so3_scalars(wx, wy, wz);
    if (lane < 9) s_W[lane] = hat(wx, wy, wz, lane);
    WSYNC();
    if (lane < 9) Rwg[lane] = s_misc[2] ? (double)eye(lane) : (double)exp_entry(so, s_W, lane);
}

// ---- orbii_graph_init_device / orbii_oplus_device / orbii_recover_device: a thread per key frame ----------------------------------------
__global__ __launch_bounds__(II_T) void k_ii_init(const orbii_graph g, const orbi_calib cal, const double *__restrict__ pose_R, const double *__restrict__ pose_t,
                                                  int n_pose, const float *__restrict__ state, int n_src, const int32_t *__restrict__ jobs,
                                                  const orbii_bias ib, const double *__restrict__ Rwg, double scale, int32_t *__restrict__ result)
{
    const int k = threadIdx.x;
    bool ok = false;
    if (k < g.n_kf) {
        const int pr = jobs[II_JOB * k], sr = jobs[II_JOB * k + 1];
        ok = pr >= 0 && pr < n_pose && sr >= 0 && sr < n_src;
        double R[9], t[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = ok ? (double)(float)pose_R[9 * (size_t)pr + e] : 0.0;
#pragma unroll
        for (int e = 0; e < 3; ++e) t[e] = ok ? (double)(float)pose_t[3 * (size_t)pr + e] : 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) g.Rwb[9 * (size_t)k + e] = ok ? (double)state[15 * (size_t)sr + e] : deye(e);
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            g.twb[3 * (size_t)k + e] = ok ? (double)state[15 * (size_t)sr + 9 + e] : 0.0;
            g.v[3 * (size_t)k + e] = ok ? (double)state[15 * (size_t)sr + 12 + e] : 0.0;
            g.Oc[3 * (size_t)k + e] = ok ? dsum3(dmul(-R[e], t[0]), dmul(-R[3 + e], t[1]), dmul(-R[6 + e], t[2])) : 0.0;
            g.Pcb[3 * (size_t)k + e] = ok ? dsum3(dmul(R[e], (double)cal.tcb[0]), dmul(R[3 + e], (double)cal.tcb[1]), dmul(R[6 + e], (double)cal.tcb[2])) : 0.0;
        }
    }
    const int done = __syncthreads_count(ok);
    if (k < 3) g.shared[SH_BG + k] = (double)ib.bg[k], g.shared[SH_BA + k] = (double)ib.ba[k];
    if (k < 9) g.shared[SH_RWG + k] = Rwg ? Rwg[k] : deye(k);
    if (k == 0) g.shared[SH_SCALE] = scale, g.iter[0] = 0;
    if (k < 8) result[k] = k == ORBI_R_DONE ? done : k == ORBI_R_RANGE ? g.n_kf - done : 0;
}

__global__ __launch_bounds__(II_T) void k_ii_oplus(const orbii_graph g, int kind, const double *__restrict__ dx, int32_t *__restrict__ result)
{
    const int t = blockIdx.x * II_T + threadIdx.x;
    if (t < 3 * g.n_kf) g.v[t] = g.v[t] + dx[9 + t];
    if (t != 0) return;
    double *sh = g.shared;
#pragma unroll
    for (int k = 0; k < 6; ++k) sh[k] = sh[k] + dx[k];
    double R[9], E[9], N[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = sh[SH_RWG + k];
    dexp_so3(dx[6], dx[7], 0.0, E);
#pragma unroll
    for (int k = 0; k < 9; ++k) N[k] = dm3(R, E, k / 3, k % 3);
    const int it = g.iter[0] + 1;
    if (it == 3) dnormalize(N);
    g.iter[0] = it == 3 ? 0 : it;
#pragma unroll
    for (int k = 0; k < 9; ++k) sh[SH_RWG + k] = N[k];
    if (kind == ORBII_KIND_GS) sh[SH_SCALE] = dmul(sh[SH_SCALE], exp(dx[8]));
#pragma unroll
    for (int k = 0; k < 8; ++k) result[k] = k == ORBI_R_DONE ? g.n_kf + 3 + (kind == ORBII_KIND_GS) : 0;
}

__global__ __launch_bounds__(II_T) void k_ii_recover(const orbii_graph g, const int32_t *__restrict__ jobs, float *__restrict__ state, int n_src,
                                                     orbi_prior *__restrict__ priors, int n_priors, float *__restrict__ bias, float *__restrict__ summary,
                                                     int32_t *__restrict__ result)
{
    const int k = threadIdx.x;
    int code = -1;
    if (k < g.n_kf) {
        const int sr = jobs[II_JOB * k + 1], sl = jobs[II_JOB * k + 3];
        code = ORBI_R_DONE;
        if (sr < 0 || sr >= n_src || sl < 0 || sl >= n_priors) code = ORBI_R_RANGE;
        else if (job_named_before(jobs, II_JOB, k, 1, sr, 3, sl)) code = ORBI_R_DUPLICATE;
        if (code == ORBI_R_DONE) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const float v = (float)g.v[3 * (size_t)k + e];
                state[15 * (size_t)sr + 12 + e] = v;
                priors[sl].velo_priori[e] = v;
            }
        }
#pragma unroll
        for (int e = 0; e < 6; ++e) bias[6 * (size_t)k + e] = (float)g.shared[e];
    }
    const int done = __syncthreads_count(code == ORBI_R_DONE), range = __syncthreads_count(code == ORBI_R_RANGE);
    if (k < 9) summary[k] = (float)g.shared[SH_RWG + k];
    if (k == 9) summary[9] = (float)g.shared[SH_SCALE];
    if (k < 8) result[k] = k == ORBI_R_DONE ? done : k == ORBI_R_RANGE ? range : k == ORBI_R_DUPLICATE ? g.n_kf - done - range : 0;
}

// ---- orbii_linearize_device ---------------------------------------------------------------------------------------------------------------
struct LinArgs {
    orbii_graph g;
    const orbi_record *bank;
    int cap;
    float gravity;
    const orbi_edge *edges;
    const double *info;
    orbii_bias ib;
    float priori_g, priori_a;
    int kind, mode;
    double *work, *err, *chi2, *chi2_prior, *total, *H, *b;
    float *flt;
    int32_t *result;
};
enum { W_M = 0, W_R = 225 };
static_assert(W_R + 15 == ORBII_EDGE_WORK, "orbii.h states the workspace of an edge");

// ORBI_R_DONE, _RANGE or _REFUSED of edge e: the rule the edge's wave and the assembly share
__device__ __forceinline__ int edge_status(const LinArgs &a, int e)
{
    const int rec = a.edges[e].rec;
    if (rec < 0 || rec >= a.cap) return ORBI_R_RANGE;
    return edge_refused(a.info, e) ? ORBI_R_REFUSED : ORBI_R_DONE;
}

// a wave's LDS slice: floats (orbi_edge.h's X_WORDS) and doubles (orbi_edge.h's shared fields, then the constants Oc and Pcb of both key
// frames, the shared vertices, g = Rwg*gI, JG = Rwg*gm, v2 - v1, (Oc2 - Oc1) - v1*dt, (-Rb1w)*JG, (c*Rb1w)*JG, J and Omega*J)
enum {
    D_O1 = D_SHARED, D_O2 = D_O1 + 3, D_P1 = D_O2 + 3, D_P2 = D_P1 + 3, D_SH = D_P2 + 3, D_G = D_SH + SH_WORDS, D_JG = D_G + 3, D_DV = D_JG + 6,
    D_DO = D_DV + 3, D_RJG = D_DO + 3, D_CRJG = D_RJG + 6, D_J = D_CRJG + 6, D_WJ = D_J + 135, D_WORDS = D_WJ + 135
};
static_assert(X_WORDS == 140 && D_WORDS == 574, "include/orbii.h states the LDS of k_ii_edge");

// entry (r, c) of the 9 x 15 Jacobian in the local order [v1, bg, ba, v2, gravity, scale] (G2oTypes.cpp:134-162, :222-245)
__device__ __forceinline__ double jac_entry(const double *S, int kind, double dt, int r, int c)
{
    const int rb = r / 3, i = r - 3 * rb, cb = c / 3, j = c - 3 * cb;
    const double s = S[D_SH + SH_SCALE];
    const bool gs = kind == ORBII_KIND_GS;
    if (c == 14) {                                                         // (s*Rb1w)*(v2 - v1), (s*Rb1w)*((Oc2 - Oc1) - v1*dt)
        if (!gs || rb == 0) return 0.0;
        const double *x = S + (rb == 1 ? D_DV : D_DO);
        return dsum3(dmul(dmul(s, S[D_R1 + i]), x[0]), dmul(dmul(s, S[D_R1 + 3 + i]), x[1]), dmul(dmul(s, S[D_R1 + 6 + i]), x[2]));
    }
    if (c >= 12) {
        if (rb == 0) return 0.0;
        return rb == 1 ? dmul(S[D_RJG + 2 * i + c - 12], dt) : S[D_CRJG + 2 * i + c - 12];
    }
    const double rb1w = S[D_R1 + 3 * j + i];                                // entry (i, j) of Rb1w
    if (rb == 0) return cb == 1 ? dm3(S + D_T5, S + D_JRG, i, j) : 0.0;     // (((-invJr)*eR^T)*Jr)*JRg
    if (rb == 1) {
        if (cb == 0) return gs ? dmul(-s, rb1w) : -rb1w;
        if (cb == 1) return -S[D_JVG + 3 * i + j];
        if (cb == 2) return -S[D_JVA + 3 * i + j];
        return gs ? dmul(s, rb1w) : rb1w;
    }
    if (cb == 0) return gs ? dmul(dmul(-s, dt), rb1w) : dmul(-dt, rb1w);
    if (cb == 1) return -S[D_JPG + 3 * i + j];
    if (cb == 2) return gs ? -S[D_JPA + 3 * i + j] : -S[D_JPG + 3 * i + j];  // kind G: -JPg where -JPa belongs, as G2oTypes.cpp:236 has it
    return 0.0;
}

__global__ __launch_bounds__(II_T) void k_ii_edge(const LinArgs a)
{
    __shared__ __attribute__((aligned(16))) double s_d[II_WAVES][D_WORDS];
    __shared__ float s_f[II_WAVES][X_WORDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e = blockIdx.x * II_WAVES + wave;
    if (e >= a.g.n_kf - 1) return;                   // no workgroup barrier in this kernel
    double *S = s_d[wave];
    float *F = s_f[wave];
    double *work = a.work + (size_t)ORBII_EDGE_WORK * e;
    const int g = lane / 9, q = lane - 9 * g;
    const int status = __builtin_amdgcn_readfirstlane(edge_status(a, e));
    if (status != ORBI_R_DONE) {
        if (lane < 9) a.err[9 * (size_t)e + lane] = 0.0;
        if (lane == 0) a.chi2[e] = 0.0;
        if (a.flt && lane < 15) a.flt[15 * (size_t)e + lane] = 0.f;
        return;
    }
    const int rec = __builtin_amdgcn_readfirstlane(a.edges[e].rec), gs = a.kind == ORBII_KIND_GS;
    // ---- load: the head of the record, the constants of both key frames, the vertices, the information
    edge_load(a.bank, rec, a.info, e, F, S, lane);
    if (lane < 18) S[D_R1 + lane] = a.g.Rwb[9 * (size_t)e + lane];                  // R1, R2 are adjacent rows
    else if (lane < 24) S[D_T1 + lane - 18] = a.g.twb[3 * (size_t)e + lane - 18];
    else if (lane < 30) S[D_O1 + lane - 24] = a.g.Oc[3 * (size_t)e + lane - 24];
    else if (lane < 36) S[D_P1 + lane - 30] = a.g.Pcb[3 * (size_t)e + lane - 30];
    else if (lane < 42) S[D_V1 + lane - 36] = a.g.v[3 * (size_t)e + lane - 36];
    else if (lane < 58) S[D_SH + lane - 42] = a.g.shared[lane - 42];
    WSYNC();
    // ---- the float part: the bias vertices cast to float, getDeltaRotation / Velocity / Position (Imu.cpp:182-192)
    bias_deltas(F, F + X_T, lane, lane < 6 ? (float)S[D_SH + lane] : 0.f);
    if (a.flt && lane < 15) a.flt[15 * (size_t)e + lane] = lane < 9 ? F[X_T + BD_DRU + lane] : F[X_T + BD_DVP + lane - 9];
    // ---- everything behind the cast to double: this edge's lines on lane 63 and on lane groups 2 .. 5, the rotation residual beside them
    const double dt = (double)F[RH_DT], G = (double)a.gravity, s = S[D_SH + SH_SCALE];
    const double *Rwg = S + D_SH + SH_RWG;
    if (lane == 63) {                                                             // g = Rwg*gI and JG = Rwg*gm, their zero terms dropped
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            S[D_G + k] = dmul(Rwg[3 * k + 2], -G);
            S[D_JG + 2 * k] = dmul(Rwg[3 * k + 1], G);
            S[D_JG + 2 * k + 1] = dmul(Rwg[3 * k], -G);
        }
    }
    edge_widen(F, F + X_T, S, lane);
    if (g == 2 && q < 3) {                                                        // ev
        double d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double dv = S[D_V2 + k] - S[D_V1 + k];
            d[k] = (gs ? dmul(s, dv) : dv) - dmul(S[D_G + k], dt);
        }
        S[D_E + 3 + q] = dmv3t(S + D_R1, d[0], d[1], d[2], q) - S[D_DVP + q];
    } else if (g == 3 && q < 3) {                                                 // ep
        double d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double grav = dmul(dmul(dmul(0.5, S[D_G + k]), dt), dt);
            if (gs) d[k] = ((((dmul(s, S[D_O2 + k]) + S[D_P2 + k]) - dmul(s, S[D_O1 + k])) - S[D_P1 + k]) - dmul(dmul(s, S[D_V1 + k]), dt)) - grav;
            else d[k] = ((S[D_T2 + k] - S[D_T1 + k]) - dmul(S[D_V1 + k], dt)) - grav;
        }
        S[D_E + 6 + q] = dmv3t(S + D_R1, d[0], d[1], d[2], q) - S[D_DVP + 3 + q];
    } else if (g == 4 && q < 3) {
        S[D_DV + q] = S[D_V2 + q] - S[D_V1 + q];
        S[D_DO + q] = (S[D_O2 + q] - S[D_O1 + q]) - dmul(S[D_V1 + q], dt);
    } else if (g == 5 && q < 6) {                                                 // (-Rb1w)*JG and (c*Rb1w)*JG, c = ((-0.5)*dt)*dt; 3 x 2
        const int r = q / 2, c = q - 2 * r;
        const double cc = dmul(dmul(-0.5, dt), dt);
        S[D_RJG + q] = dsum3(dmul(-S[D_R1 + r], S[D_JG + c]), dmul(-S[D_R1 + 3 + r], S[D_JG + 2 + c]), dmul(-S[D_R1 + 6 + r], S[D_JG + 4 + c]));
        S[D_CRJG + q] = dsum3(dmul(dmul(cc, S[D_R1 + r]), S[D_JG + c]), dmul(dmul(cc, S[D_R1 + 3 + r]), S[D_JG + 2 + c]), dmul(dmul(cc, S[D_R1 + 6 + r]), S[D_JG + 4 + c]));
    }
    edge_rotation(S, lane);
    const double chi = edge_chi2(S, lane);
    if (lane < 9) a.err[9 * (size_t)e + lane] = S[D_E + lane];
    if (lane == 0) a.chi2[e] = chi;
    if (a.mode != 0) return;
    // ---- the Jacobian, Omega*J, J^T*(Omega*J) and -J^T*(Omega*e)
#pragma unroll
    for (int h = 0; h < 3; ++h) {
        const int x = lane + 64 * h;
        if (x < 135) S[D_J + x] = jac_entry(S, a.kind, dt, x / 15, x % 15);
    }
    WSYNC();
    edge_quadratic_form<15>(S, S + D_J, S + D_WJ, 1.0, work + W_M, work + W_R, lane);
}

// the local index of global dof d on edge e, which touches it
__device__ __forceinline__ int local_dof(int d, int e)
{
    if (d < 6) return 3 + d;                      // bg, ba
    if (d < 8) return 6 + d;                      // gravity
    if (d == 8) return 14;
    const int k = (d - 9) / 3, c = (d - 9) - 3 * k;
    return k == e ? c : 9 + c;
}
// the edges [lo, hi] that touch dof d, intersected with [lo, hi]
__device__ __forceinline__ void dof_edges(int d, int &lo, int &hi)
{
    if (d < 9) return;
    const int k = (d - 9) / 3;
    lo = max(lo, k - 1), hi = min(hi, k);
}

// workgroup 0: the priors' chi2, the total, d_result.  Workgroups 1 .. (mode 0): a thread per entry of d_H, then of d_b
__global__ __launch_bounds__(II_T) void k_ii_assemble(const LinArgs a)
{
    const int n_kf = a.g.n_kf, ne = n_kf - 1, N = ORBII_N(n_kf);
    const double wg = (double)a.priori_g, wa = (double)a.priori_a;
    if (blockIdx.x == 0) {
        if (threadIdx.x != 0) return;
        int cnt[4] = {0, 0, 0, 0};
        double total = 0.0;
        for (int e = 0; e < ne; ++e) {
            const int st = edge_status(a, e);
            ++cnt[st];
            if (st == ORBI_R_DONE) total = total + a.chi2[e];
        }
        for (int p = 0; p < 2; ++p) {
            const double w = p == 0 ? wg : wa;
            const float *m = p == 0 ? a.ib.bg : a.ib.ba;
            const double e0 = (double)m[0] - a.g.shared[3 * p], e1 = (double)m[1] - a.g.shared[3 * p + 1], e2 = (double)m[2] - a.g.shared[3 * p + 2];
            const double c = dsum3(dmul(e0, dmul(w, e0)), dmul(e1, dmul(w, e1)), dmul(e2, dmul(w, e2)));
            a.chi2_prior[p] = c;
            total = total + c;
        }
        a.total[0] = total;
        for (int k = 0; k < 8; ++k) a.result[k] = k < 4 ? cnt[k] : 0;
        return;
    }
    const long long idx = (long long)(blockIdx.x - 1) * II_T + threadIdx.x;
    if (idx >= (long long)N * N + N) return;
    const bool is_b = idx >= (long long)N * N;
    const int r = is_b ? (int)(idx - (long long)N * N) : (int)(idx / N), c = is_b ? r : (int)(idx - (long long)r * N);
    double sum;
    if (!dof_free(r, n_kf, a.kind) || !dof_free(c, n_kf, a.kind)) sum = (!is_b && r == c) ? 1.0 : 0.0;
    else {
        int lo = 0, hi = ne - 1;
        dof_edges(r, lo, hi);
        dof_edges(c, lo, hi);
        sum = 0.0;
        for (int e = lo; e <= hi; ++e) {
            if (edge_status(a, e) != ORBI_R_DONE) continue;
            const double *w = a.work + (size_t)ORBII_EDGE_WORK * e;
            sum = sum + (is_b ? w[W_R + local_dof(r, e)] : w[W_M + 15 * local_dof(r, e) + local_dof(c, e)]);
        }
        if (r < 6 && r == c) {
            const double w = r < 3 ? wg : wa;
            if (!is_b) sum = sum + w;
            else sum = sum + dmul(w, (double)(r < 3 ? a.ib.bg[r] : a.ib.ba[r - 3]) - a.g.shared[r]);
        }
    }
    if (is_b) a.b[r] = sum;
    else a.H[idx] = sum;
}

// ---- orbii_damp_device: a thread per entry; the first wave also finds the largest free diagonal entry ----------------------------------------
__global__ __launch_bounds__(II_T) void k_ii_damp(int n_kf, int kind, const double *__restrict__ H, const double *__restrict__ b, const double *__restrict__ lambda,
                                                  double *__restrict__ S, double *__restrict__ rhs, double *__restrict__ out, int32_t *__restrict__ result)
{
    const int N = ORBII_N(n_kf);
    const int idx = blockIdx.x * II_T + threadIdx.x;
    if (idx < N * N) {
        const int r = idx / N, c = idx - r * N;
        const double h = H[idx];
        S[idx] = (r == c && dof_free(r, n_kf, kind)) ? h + lambda[0] : h;
    }
    if (idx < N) rhs[idx] = b[idx];
    if (blockIdx.x != 0 || threadIdx.x >= 64) return;
    double m = 0.0;
    for (int d = threadIdx.x; d < N; d += 64)
        if (dof_free(d, n_kf, kind)) {
            const double h = H[(size_t)d * N + d];
            if (h > m) m = h;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(m, o, 64);
        if (other > m) m = other;
    }
    if (threadIdx.x == 0) out[1] = m;
    if (threadIdx.x < 8) result[threadIdx.x] = threadIdx.x == ORBI_R_DONE ? 1 : 0;
}

int check_graph(const orbii_graph &g, const void *result)
{
    if (!g.v || !g.shared || !g.iter || !g.Rwb || !g.twb || !g.Oc || !g.Pcb || !result) return orbx_set_error(ORBX_E_ARG, "null graph array or result");
    if (g.n_kf < 2) return orbx_set_error(ORBX_E_ARG, "an initialisation has at least two key frames");
    return ORBX_OK;
}
int check_count(int n_kf)
{
    if (n_kf > ORBII_MAX_KF) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBII_MAX_KF (157) key frames: the system has at most 480 unknowns");
    return ORBX_OK;
}
int check_kind(int kind)
{
    if (kind != ORBII_KIND_GS && kind != ORBII_KIND_G) return orbx_set_error(ORBX_E_ARG, "kind is 0 (EdgeInertialGS) or 1 (EdgeInertialG)");
    return ORBX_OK;
}

} // namespace

extern "C" int orbii_prior_device(const double *d_pose_R, const double *d_pose_t, int n_pose, float *d_state, int n_src, const orbi_record *d_bank,
                                  int cap, orbi_prior *d_priors, int n_priors, const int32_t *d_jobs, int n, double *d_Rwg, int32_t *d_result,
                                  void *stream)
{
    if (!d_pose_R || !d_pose_t || !d_state || !d_bank || !d_priors || !d_jobs || !d_Rwg || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (n_pose < 1 || n_src < 1 || cap < 1 || n_priors < 1) return orbx_set_error(ORBX_E_ARG, "n_pose, n_src, cap and n_priors must be positive");
    if (n < 2) return orbx_set_error(ORBX_E_ARG, "an initialisation has at least two key frames");
    if (int rc = check_count(n)) return rc;
    if (int rc = orb_need_device()) return rc;
    hipLaunchKernelGGL(k_ii_prior, dim3(1), dim3(64), 0, (hipStream_t)stream, d_pose_R, d_pose_t, n_pose, d_state, n_src, d_bank, cap, d_priors, n_priors,
                       d_jobs, n, d_Rwg, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbii_graph_init_device(orbii_graph graph, orbi_calib calib, const double *d_pose_R, const double *d_pose_t, int n_pose,
                                       const float *d_state, int n_src, const int32_t *d_jobs, orbii_bias initial_bias, const double *d_Rwg,
                                       double scale, int32_t *d_result, void *stream)
{
    if (int rc = check_graph(graph, d_result)) return rc;
    if (!d_pose_R || !d_pose_t || !d_state || !d_jobs) return orbx_set_error(ORBX_E_ARG, "null pose table, state array or job list");
    if (n_pose < 1 || n_src < 1) return orbx_set_error(ORBX_E_ARG, "n_pose and n_src must be positive");
    if (int rc = check_count(graph.n_kf)) return rc;
    if (int rc = orb_need_device()) return rc;
    hipLaunchKernelGGL(k_ii_init, dim3(1), dim3(II_T), 0, (hipStream_t)stream, graph, calib, d_pose_R, d_pose_t, n_pose, d_state, n_src, d_jobs,
                       initial_bias, d_Rwg, scale, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbii_linearize_device(orbii_graph graph, const orbi_record *d_bank, int cap, float gravity, const orbi_edge *d_edges,
                                      const double *d_info, orbii_bias initial_bias, float priori_g, float priori_a, int kind, int mode,
                                      double *d_work, double *d_err, double *d_chi2, double *d_chi2_prior, double *d_total, double *d_H, double *d_b,
                                      float *d_float, int32_t *d_result, void *stream)
{
    if (int rc = check_graph(graph, d_result)) return rc;
    if (!d_bank || cap < 1 || !d_edges || !d_info || !d_work || !d_err || !d_chi2 || !d_chi2_prior || !d_total)
        return orbx_set_error(ORBX_E_ARG, "null bank, edges, information, workspace or output, or cap < 1");
    if (int rc = check_kind(kind)) return rc;
    if (mode != 0 && mode != 1) return orbx_set_error(ORBX_E_ARG, "mode is 0 (linearise) or 1 (computeError only)");
    if (mode == 0 && (!d_H || !d_b)) return orbx_set_error(ORBX_E_ARG, "mode 0 needs d_H and d_b");
    if (int rc = check_count(graph.n_kf)) return rc;
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    LinArgs a = {};
    a.g = graph, a.bank = d_bank, a.cap = cap, a.gravity = gravity, a.edges = d_edges, a.info = d_info, a.ib = initial_bias;
    a.priori_g = priori_g, a.priori_a = priori_a, a.kind = kind, a.mode = mode, a.work = d_work, a.err = d_err, a.chi2 = d_chi2;
    a.chi2_prior = d_chi2_prior, a.total = d_total, a.H = d_H, a.b = d_b, a.flt = d_float, a.result = d_result;
    const int ne = graph.n_kf - 1, N = ORBII_N(graph.n_kf);
    hipLaunchKernelGGL(k_ii_edge, dim3((ne + II_WAVES - 1) / II_WAVES), dim3(II_T), 0, s, a);
    const int entries = mode == 0 ? N * N + N : 0;
    hipLaunchKernelGGL(k_ii_assemble, dim3(1 + (entries + II_T - 1) / II_T), dim3(II_T), 0, s, a);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbii_damp_device(int n_kf, int kind, const double *d_H, const double *d_b, const double *d_lambda, double *d_S, double *d_rhs,
                                 double *d_out, int32_t *d_result, void *stream)
{
    if (!d_H || !d_b || !d_lambda || !d_S || !d_rhs || !d_out || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (n_kf < 2) return orbx_set_error(ORBX_E_ARG, "an initialisation has at least two key frames");
    if (int rc = check_kind(kind)) return rc;
    if (int rc = check_count(n_kf)) return rc;
    if (int rc = orb_need_device()) return rc;
    const int N = ORBII_N(n_kf);
    hipLaunchKernelGGL(k_ii_damp, dim3((N * N + II_T - 1) / II_T), dim3(II_T), 0, (hipStream_t)stream, n_kf, kind, d_H, d_b, d_lambda, d_S, d_rhs, d_out,
                       d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbii_oplus_device(orbii_graph graph, int kind, const double *d_dx, int32_t *d_result, void *stream)
{
    if (int rc = check_graph(graph, d_result)) return rc;
    if (!d_dx) return orbx_set_error(ORBX_E_ARG, "null d_dx");
    if (int rc = check_kind(kind)) return rc;
    if (int rc = check_count(graph.n_kf)) return rc;
    if (int rc = orb_need_device()) return rc;
    hipLaunchKernelGGL(k_ii_oplus, dim3((3 * graph.n_kf + II_T - 1) / II_T), dim3(II_T), 0, (hipStream_t)stream, graph, kind, d_dx, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbii_recover_device(orbii_graph graph, const int32_t *d_jobs, float *d_state, int n_src, orbi_prior *d_priors, int n_priors,
                                    float *d_bias, float *d_summary, int32_t *d_result, void *stream)
{
    if (int rc = check_graph(graph, d_result)) return rc;
    if (!d_jobs || !d_state || !d_priors || !d_bias || !d_summary) return orbx_set_error(ORBX_E_ARG, "null job list, state array, priors, d_bias or d_summary");
    if (n_src < 1 || n_priors < 1) return orbx_set_error(ORBX_E_ARG, "n_src and n_priors must be positive");
    if (int rc = check_count(graph.n_kf)) return rc;
    if (int rc = orb_need_device()) return rc;
    hipLaunchKernelGGL(k_ii_recover, dim3(1), dim3(II_T), 0, (hipStream_t)stream, graph, d_jobs, d_state, n_src, d_priors, n_priors, d_bias, d_summary,
                       d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
