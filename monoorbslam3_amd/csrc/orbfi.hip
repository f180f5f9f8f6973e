// fullInertialOptimize's shared-bias graph linearised on the device (include/orbfi.h):
//   orbfi_jobs_device        the job lists of this graph shape from the window assembly's      Optimize.cpp:253-367
//   orbfi_linearize_device   computeError, linearizeOplus, constructQuadraticForm              G2oTypes.cpp:377-445, G2oTypes.h:324-343, 452-470
//   orbfi_recover_device     step 4                                                            Optimize.cpp:401-434
//
// The edge is EdgeInertial as k_fac_edge (orbi_factors.hip) evaluates it, out of the same pieces -- orbi_edge.h, orbi_factors_device.h,
// orbi_so3.h -- with the bias vertices read from the carrier state and the carrier's fixed mask on the Jacobian's columns 9..14.  What is
// its own is where the quadratic form goes: the 30 x 30 form of an edge holds the blocks of THREE states (i: dof 0..8, the carrier: dof
// 9..14, j: dof 15..23), so the edge leaves three off-diagonal blocks for the visual window's reduce and the gather takes a key frame's 9 x 9
// and the carrier's 6 x 6 from the two diagonal blocks in the workspace.
//
// Shape: at most 30 edges, latency-bound.  ONE WAVE per edge, four per workgroup, the wave's vertices, temporaries, Jacobian, information
// and their product in its own slice of LDS, wave-level fences only; then ONE WAVE PER STATE adds up in ascending edge order, the carrier
// over all edges with the two priors last, and one more wave computes the priors' chi2 and the totals.  No floating-point atomics.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "../../include/orbfi.h"
#include "../../include/orbx.h"
#include "orb_host.h"
#include "orb_math.h"
#include "orbi_edge.h"
#include "orbi_factors_device.h"
#include "orbi_graph_device.h"
#include "orbi_so3.h"
#include "orbi_so3d.h"

#pragma clang fp contract(off)

namespace {

constexpr int FI_WAVES = 4, FI_T = 64 * FI_WAVES;

struct FiArgs {
    orbi_graph g;
    const orbi_record *bank;
    int cap;
    float gravity;
    const orbi_edge *edges;
    int n_edges;
    const double *info;
    int bias_state, prior_rec;
    double prior_g, prior_a, delta;
    int mode;
    double *work, *err, *chi2, *chi2_prior, *total, *H_diag, *b, *H_off;
    orbi_edge *off_edges;
    float *flt;
    int32_t *result;
};

// the workspace of an edge: the 15 x 15 block of dof 0..14 of its form (state i and the carrier), the one of dof 15..29 (state j), the 30
// right-hand sides, status, Huber weight
enum { W_HII = 0, W_HJJ = 225, W_B = 450, W_STATUS = 480, W_RHO1 = 481 };
static_assert(W_RHO1 + 1 == ORBFI_EDGE_WORK, "orbfi.h states the workspace of an edge");
enum { ST_OK = 0, ST_RANGE = 1, ST_REFUSED = 3 };   // == ORBI_R_DONE, ORBI_R_RANGE, ORBI_R_REFUSED
static_assert(X_WORDS == 140 && D_WORDS == 825, "include/orbfi.h states the LDS of k_fi_edge");

__global__ __launch_bounds__(FI_T) void k_fi_edge(const FiArgs a)
{
    __shared__ __attribute__((aligned(16))) double s_d[FI_WAVES][D_WORDS];
    __shared__ float s_f[FI_WAVES][X_WORDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e = blockIdx.x * FI_WAVES + wave;
    if (e >= a.n_edges) return;                      // no workgroup barrier in this kernel
    double *S = s_d[wave];
    float *F = s_f[wave];
    double *work = a.work + (size_t)ORBFI_EDGE_WORK * e;
    const int si = __builtin_amdgcn_readfirstlane(a.edges[e].i), sj = __builtin_amdgcn_readfirstlane(a.edges[e].j);
    const int rec = __builtin_amdgcn_readfirstlane(a.edges[e].rec), sb = a.bias_state;
    const int g = lane / 9, q = lane - 9 * g, i = q / 3, j = q - 3 * i;
    int status = ST_OK;
    if (!edge_valid(si, sj, rec, a.g.n_states, a.cap) || si == sb || sj == sb) status = ST_RANGE;
    else if (edge_refused(a.info, e)) status = ST_REFUSED;
    if (status != ST_OK) {
        if (lane < 9) a.err[9 * (size_t)e + lane] = 0.0;
        if (lane == 0) a.chi2[e] = 0.0;
        if (a.flt && lane < 15) a.flt[15 * (size_t)e + lane] = 0.f;
        if (a.mode == 0) {
            for (int x = lane; x < 675; x += 64) a.H_off[675 * (size_t)e + x] = 0.0;
            if (lane < 3) a.off_edges[3 * (size_t)e + lane] = orbi_edge{0, 0, 0, 0};
        }
        if (lane == 0) work[W_STATUS] = (double)status;
        return;
    }
    // ---- load: the head of the record, the vertices of both states, the carrier's bias pair, the information
    edge_load(a.bank, rec, a.info, e, F, S, lane);
    if (lane < 9) S[D_R1 + lane] = a.g.Rwb[9 * (size_t)si + lane];
    else if (lane < 18) S[D_R2 + lane - 9] = a.g.Rwb[9 * (size_t)sj + lane - 9];
    else if (lane < 21) S[D_T1 + lane - 18] = a.g.twb[3 * (size_t)si + lane - 18];
    else if (lane < 24) S[D_T2 + lane - 21] = a.g.twb[3 * (size_t)sj + lane - 21];
    else if (lane < 27) S[D_V1 + lane - 24] = a.g.v[3 * (size_t)si + lane - 24];
    else if (lane < 30) S[D_V2 + lane - 27] = a.g.v[3 * (size_t)sj + lane - 27];
    else if (lane < 33) S[D_B1 + lane - 30] = a.g.bg[3 * (size_t)sb + lane - 30];
    else if (lane < 36) S[D_B1 + lane - 30] = a.g.ba[3 * (size_t)sb + lane - 33];
    const int fix_i = a.g.fixed[si], fix_j = a.g.fixed[sj], fix_b = a.g.fixed[sb];
    WSYNC();
    // ---- the float part: the carrier's bias vertices cast to float, getDeltaRotation / Velocity / Position (Imu.cpp:182-192)
    bias_deltas(F, F + X_T, lane, lane < 6 ? (float)S[D_B1 + lane] : 0.f);
    if (a.flt && lane < 15) a.flt[15 * (size_t)e + lane] = lane < 9 ? F[X_T + BD_DRU + lane] : F[X_T + BD_DVP + lane - 9];
    // ---- everything behind the cast to double
    const double dt = (double)F[RH_DT], G = (double)a.gravity;
    edge_widen(F, F + X_T, S, lane);
    edge_velocity_position(S, lane, G, dt);                                       // ev, ep and Rb1w*R2
    edge_rotation(S, lane);
    if (g == 2) S[D_T3 + q] = dm3nt(S + D_INVJ, S + D_R2, i, j);                  // (-invJr) * R2^T
    // ---- chi2 and the Huber kernel (g2o's RobustKernelHuber)
    const double chi = edge_chi2(S, lane);
    double rho1 = 1.0;
    if (a.delta > 0.0 && chi > dmul(a.delta, a.delta)) rho1 = a.delta / sqrt(chi);
    if (lane < 9) a.err[9 * (size_t)e + lane] = S[D_E + lane];
    if (lane == 0) a.chi2[e] = chi, work[W_STATUS] = (double)ST_OK, work[W_RHO1] = rho1;
    if (a.mode != 0) return;
    // ---- the Jacobian with the columns of fixed dof zeroed: 0..8 by state i, 9..14 by the carrier, 15..29 by state j
#pragma unroll
    for (int h = 0; h < 5; ++h) {
        const int x = lane + 64 * h;
        if (x < 270) {
            const int r = x / 30, c = x - 30 * r;
            const double v = jac_entry(S, dt, r, c);
            S[D_J + x] = dof_fixed(c < 9 ? fix_i : c < 15 ? fix_b : fix_j, c < 15 ? c : c - 15) ? 0.0 : v;
        }
    }
    WSYNC();
    // W = rho1 * Omega: the two diagonal blocks and the right-hand sides to the workspace; the blocks (i, j), (i, b), (j, b) to d_H_off
    edge_quadratic_form<30>(S, S + D_J, S + D_WJ, rho1, work + W_HII, work + W_B, lane);
    for (int y = lane; y < 675; y += 64) {
        const int blk = y / 225, z = y - 225 * blk, r = z / 15, c = z - 15 * r;
        double s = 0.0;
        if (r < 9 && (blk == 0 ? c < 9 : c >= 9)) s = edge_jtwj<30>(S + D_J, S + D_WJ, blk == 2 ? 15 + r : r, blk == 0 ? 15 + c : c);
        a.H_off[675 * (size_t)e + y] = s;
    }
    if (lane < 3) a.off_edges[3 * (size_t)e + lane] = orbi_edge{lane == 2 ? sj : si, lane == 0 ? sj : sb, rec, 0};
}

// mode 0: waves [0, n_states) gather a state each; the last wave (the only one of mode 1) does the priors' chi2, the totals, d_result
__global__ __launch_bounds__(FI_T) void k_fi_gather(const FiArgs a)
{
    __shared__ int s_cnt[8];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_gather = a.mode == 0 ? a.g.n_states : 0;
    const int s = blockIdx.x * FI_WAVES + wave;
    const bool prior_ok = a.prior_rec >= 0 && a.prior_rec < a.cap;
    if (s < n_gather) {
        const int fixed = a.g.fixed[s];
        const bool carrier = s == a.bias_state;
        double h[4] = {0.0, 0.0, 0.0, 0.0}, bb = 0.0;       // entries lane + 64k of the 15 x 15 block; entry `lane` of b
        bool mine[4];                                        // the key frame's 9 x 9 or the carrier's 6 x 6 of a diagonal block
        int hr[4], hc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            hr[k] = (lane + 64 * k) / 15, hc[k] = (lane + 64 * k) % 15;
            mine[k] = lane + 64 * k < 225 && (carrier ? hr[k] >= 9 && hc[k] >= 9 : hr[k] < 9 && hc[k] < 9);
        }
        const bool mine_b = carrier ? lane >= 9 && lane < 15 : lane < 9;
        for (int c0 = 0; c0 < a.n_edges; c0 += 64) {
            const int e = c0 + lane;
            int side = 0;                                     // 1: the block of dof 0..14 (state i, the carrier), 2: the one of state j
            if (e < a.n_edges && a.work[(size_t)ORBFI_EDGE_WORK * e + W_STATUS] == (double)ST_OK)
                side = (carrier || a.edges[e].i == s) ? 1 : a.edges[e].j == s ? 2 : 0;
            unsigned long long mi = __ballot(side == 1), m = mi | __ballot(side == 2);
            while (m) {
                const int bit = __builtin_ctzll(m);
                m &= m - 1;
                const bool first = (mi >> bit) & 1;
                const double *w = a.work + (size_t)ORBFI_EDGE_WORK * (c0 + bit);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (mine[k]) h[k] = h[k] + w[(first ? W_HII : W_HJJ) + lane + 64 * k];
                if (mine_b) bb = bb + w[W_B + (first ? 0 : 15) + lane];
            }
        }
        if (carrier && prior_ok) {                            // the two EdgePriori3D: e = priori - estimate, J = -I, Omega = p*I
            const float *me = a.bank[a.prior_rec].updated_bias;
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                if ((fixed >> (v + 2)) & 1) continue;
                const double p = v == 0 ? a.prior_g : a.prior_a;
                const double *est = (v == 0 ? a.g.bg : a.g.ba) + 3 * (size_t)s;
                const int base = 9 + 3 * v;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (lane + 64 * k < 225 && hr[k] >= base && hr[k] < base + 3 && hr[k] == hc[k]) h[k] = h[k] + p;
                if (lane >= base && lane < base + 3) bb = bb + dmul(p, (double)me[3 * v + lane - base] - est[lane - base]);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (lane + 64 * k < 225) a.H_diag[225 * (size_t)s + lane + 64 * k] = h[k];
        if (lane < 15) a.b[15 * (size_t)s + lane] = bb;
    }
    if (s != n_gather) return;                                // uniform per wave; the tail wave alone uses s_cnt
    if (lane < 8) s_cnt[lane] = 0;
    WSYNC();
    for (int e = lane; e < a.n_edges; e += 64) atomicAdd(&s_cnt[(int)a.work[(size_t)ORBFI_EDGE_WORK * e + W_STATUS]], 1);
    WSYNC();
    if (lane < 8) a.result[lane] = lane == ORBI_R_PRIOR_DONE ? (prior_ok ? 2 : 0) : lane == ORBI_R_PRIOR_RANGE ? (prior_ok ? 0 : 2) : s_cnt[lane];
    if (lane == 0) {                                          // the priors' chi2 and the totals in their one order
        double c[2] = {0.0, 0.0};
        if (prior_ok) {
            const float *me = a.bank[a.prior_rec].updated_bias;
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const double p = v == 0 ? a.prior_g : a.prior_a;
                const double *est = (v == 0 ? a.g.bg : a.g.ba) + 3 * (size_t)a.bias_state;
                const double e0 = (double)me[3 * v] - est[0], e1 = (double)me[3 * v + 1] - est[1], e2 = (double)me[3 * v + 2] - est[2];
                c[v] = dsum3(dmul(e0, dmul(p, e0)), dmul(e1, dmul(p, e1)), dmul(e2, dmul(p, e2)));
            }
        }
        a.chi2_prior[0] = c[0], a.chi2_prior[1] = c[1];
        double plain = 0.0, robust = 0.0;
        const double dsqr = dmul(a.delta, a.delta);
        for (int e = 0; e < a.n_edges; ++e) {
            const double c0 = a.chi2[e];
            const double r0 = (a.delta > 0.0 && c0 > dsqr) ? dmul(dmul(2.0, sqrt(c0)), a.delta) - dsqr : c0;
            plain = plain + c0, robust = robust + r0;
        }
        plain = (plain + c[0]) + c[1], robust = (robust + c[0]) + c[1];
        a.total[0] = plain, a.total[1] = robust;
    }
}

// ---- orbfi_recover_device: one workgroup, a thread per job ------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_fi_recover(const orbi_graph g, const orbi_calib cal, int bias_state, const int32_t *__restrict__ jobs, int n,
                                                   float *__restrict__ dst, int n_dst, float *__restrict__ bias, double *__restrict__ pose_R,
                                                   double *__restrict__ pose_t, int32_t *__restrict__ result)
{
    __shared__ int s_cnt[8];
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int job = threadIdx.x; job < n; job += 64) {
        const int st = jobs[3 * job], to = jobs[3 * job + 1];
        const int code = recover_job(g, cal, jobs, job, st, to, ORBI_RECOVER_POSE, bias_state, dst, n_dst, bias, pose_R, pose_t);
        atomicAdd(&s_cnt[code], 1);
    }
    __syncthreads();
    flush_counts(s_cnt, result);
}

// ---- orbfi_jobs_device: one wave ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_fi_jobs(const int32_t *__restrict__ init_in, const orbi_edge *__restrict__ edges_in, const int32_t *__restrict__ rec_in,
                                                int n_kf, int fix_first, int n_src, int cap, uint8_t *__restrict__ fixed, int32_t *__restrict__ init_out,
                                                orbi_edge *__restrict__ edges_out, int32_t *__restrict__ rec_out, int32_t *__restrict__ prior_rec,
                                                int32_t *__restrict__ result)
{
    __shared__ int s_cnt[8];
    const int lane = threadIdx.x;
    if (lane < 8) s_cnt[lane] = 0;
    WSYNC();
    for (int k = lane; k <= n_kf; k += 64) {
        const int from = k < n_kf ? k : n_kf - 1;             // the carrier takes the last key frame's row and record
        int row = init_in[3 * from + 1], rec = init_in[3 * from + 2];
        if (row < 0 || row >= n_src) row = -1;                // orbi_graph_init_device drops such a job
        if (rec < 0 || rec >= cap) rec = -1;
        if (k < n_kf) {
            fixed[k] = ORBI_FIX_GYRO | ORBI_FIX_ACC | (k == 0 && fix_first ? ORBI_FIX_POSE | ORBI_FIX_VELO : 0);
            init_out[3 * k] = k, init_out[3 * k + 1] = row, init_out[3 * k + 2] = -1;
            atomicAdd(&s_cnt[row < 0 ? ORBI_R_RANGE : ORBI_R_DONE], 1);
        } else {
            fixed[k] = ORBI_FIX_POSE | ORBI_FIX_VELO;
            init_out[3 * k] = k, init_out[3 * k + 1] = row, init_out[3 * k + 2] = rec < 0 ? -2 : rec;   // -2: no bias to start from, dropped there too
            *prior_rec = rec;
            atomicAdd(&s_cnt[row < 0 || rec < 0 ? ORBI_R_RANGE : ORBI_R_DONE], 1);
        }
    }
    for (int e = lane; e < n_kf - 1; e += 64) {
        const orbi_edge ed = edges_in[e];
        const bool ok = edge_valid(ed.i, ed.j, ed.rec, n_kf, cap);
        edges_out[e] = ok ? orbi_edge{ed.i, ed.j, ed.rec, 0} : orbi_edge{-1, -1, -1, 0};
        if (!ok) atomicAdd(&s_cnt[ORBI_R_RANGE], 1);
    }
    for (int k = lane; k < 3 * n_kf; k += 64) rec_out[k] = rec_in[k];
    WSYNC();
    if (lane < 8) result[lane] = s_cnt[lane];
}

int check_fi_graph(const orbi_graph &g, const void *result)
{
    if (!g.Rwb || !g.twb || !g.v || !g.bg || !g.ba || !g.fixed || g.n_states < 0 || !result)
        return orbx_set_error(ORBX_E_ARG, "null graph array or result, or a negative state count");
    return ORBX_OK;
}

} // namespace

extern "C" int orbfi_jobs_device(const int32_t *d_init_jobs, const orbi_edge *d_inertial_edges, const int32_t *d_recover_jobs, int n_kf, int fix_first,
                                 int n_src, int cap, uint8_t *d_fixed, int32_t *d_init_out, orbi_edge *d_edges_out, int32_t *d_recover_out,
                                 int32_t *d_prior_rec, int32_t *d_result, void *stream)
{
    if (!d_init_jobs || !d_inertial_edges || !d_recover_jobs || !d_fixed || !d_init_out || !d_edges_out || !d_recover_out || !d_prior_rec || !d_result)
        return orbx_set_error(ORBX_E_ARG, "null list, output or result");
    if (n_kf < 1 || n_src < 1 || cap < 1) return orbx_set_error(ORBX_E_ARG, "n_kf, n_src or cap < 1");
    if (n_kf > ORBFI_MAX_KEYFRAMES) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBFI_MAX_KEYFRAMES (31) key frames");
    if (int rc = orb_need_device()) return rc;
    hipLaunchKernelGGL(k_fi_jobs, dim3(1), dim3(64), 0, (hipStream_t)stream, d_init_jobs, d_inertial_edges, d_recover_jobs, n_kf, fix_first, n_src, cap,
                       d_fixed, d_init_out, d_edges_out, d_recover_out, d_prior_rec, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbfi_linearize_device(orbi_graph graph, const orbi_record *d_bank, int cap, float gravity, const orbi_edge *d_edges, int n_edges,
                                      const double *d_info, int bias_state, int prior_rec, float prior_g, float prior_a, double huber_delta, int mode,
                                      double *d_work, double *d_err, double *d_chi2, double *d_chi2_prior, double *d_total, double *d_H_diag, double *d_b,
                                      orbi_edge *d_off_edges, double *d_H_off, float *d_float, int32_t *d_result, void *stream)
{
    if (int rc = check_fi_graph(graph, d_result)) return rc;
    if (!d_edges || n_edges < 0) return orbx_set_error(ORBX_E_ARG, "null edge list or a negative edge count");
    if (!d_bank || cap < 1 || !d_info || !d_work || !d_err || !d_chi2 || !d_chi2_prior || !d_total || !(huber_delta == huber_delta) ||
        !(prior_g == prior_g) || !(prior_a == prior_a))
        return orbx_set_error(ORBX_E_ARG, "null bank, information, workspace or output, cap < 1, or huber_delta or a prior weight is not a number");
    if (bias_state < 0 || bias_state >= graph.n_states) return orbx_set_error(ORBX_E_ARG, "bias_state outside [0, n_states)");
    if (mode != 0 && mode != 1) return orbx_set_error(ORBX_E_ARG, "mode is 0 (linearise) or 1 (computeError only)");
    if (mode == 0 && (!d_H_diag || !d_b || !d_off_edges || !d_H_off)) return orbx_set_error(ORBX_E_ARG, "mode 0 needs d_H_diag, d_b, d_off_edges and d_H_off");
    if (graph.n_states > ORBFI_MAX_KEYFRAMES + 1) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBFI_MAX_KEYFRAMES (31) key frames beside the carrier");
    if (n_edges > ORBI_MAX_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBI_MAX_JOBS (4096) edges in one call");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    FiArgs a = {};
    a.g = graph, a.bank = d_bank, a.cap = cap, a.gravity = gravity, a.edges = d_edges, a.n_edges = n_edges, a.info = d_info;
    a.bias_state = bias_state, a.prior_rec = prior_rec, a.prior_g = (double)prior_g, a.prior_a = (double)prior_a, a.delta = huber_delta, a.mode = mode;
    a.work = d_work, a.err = d_err, a.chi2 = d_chi2, a.chi2_prior = d_chi2_prior, a.total = d_total, a.H_diag = d_H_diag, a.b = d_b;
    a.off_edges = d_off_edges, a.H_off = d_H_off, a.flt = d_float, a.result = d_result;
    if (n_edges > 0) hipLaunchKernelGGL(k_fi_edge, dim3((n_edges + FI_WAVES - 1) / FI_WAVES), dim3(FI_T), 0, s, a);
    const int waves = (mode == 0 ? graph.n_states : 0) + 1;
    hipLaunchKernelGGL(k_fi_gather, dim3((waves + FI_WAVES - 1) / FI_WAVES), dim3(FI_T), 0, s, a);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbfi_recover_device(orbi_graph graph, orbi_calib calib, int bias_state, const int32_t *d_jobs, int n, float *d_dst, int n_dst,
                                    float *d_bias, double *d_pose_R, double *d_pose_t, int32_t *d_result, void *stream)
{
    if (int rc = check_fi_graph(graph, d_result)) return rc;
    if (!d_jobs || n < 0) return orbx_set_error(ORBX_E_ARG, "null job list or a negative job count");
    if (!d_dst || n_dst < 1 || !d_bias) return orbx_set_error(ORBX_E_ARG, "null destination or bias array, or n_dst < 1");
    if (!d_pose_R != !d_pose_t) return orbx_set_error(ORBX_E_ARG, "d_pose_R and d_pose_t go together");
    if (bias_state < 0 || bias_state >= graph.n_states) return orbx_set_error(ORBX_E_ARG, "bias_state outside [0, n_states)");
    if (graph.n_states > ORBFI_MAX_KEYFRAMES + 1) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBFI_MAX_KEYFRAMES (31) key frames beside the carrier");
    if (n > ORBI_MAX_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBI_MAX_JOBS (4096) jobs in one call");
    if (int rc = orb_need_device()) return rc;
    hipLaunchKernelGGL(k_fi_recover, dim3(1), dim3(64), 0, (hipStream_t)stream, graph, calib, bias_state, d_jobs, n, d_dst, n_dst, d_bias, d_pose_R, d_pose_t,
                       d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
