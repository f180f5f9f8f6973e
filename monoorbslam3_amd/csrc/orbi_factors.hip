// Inertial factors linearised on the device (include/orbi.h, "Inertial factors linearised on the device"; include/orbi_factors.h):
//   orbi_prior_information_device   KeyFrame::setPrioriInformation, the constructor's priors          KeyFrame.cpp:23-24, 86-98
//   orbi_graph_init_device          the vertices of the inertial optimisers                           Optimize.cpp:557-573, 623-651, 992-1007
//   orbi_edge_information_device    the information of EdgeInertial[Only] and of the bias walks       G2oTypes.cpp:366-367, Optimize.cpp:1022, 1028
//   orbi_linearize_device           computeError, linearizeOplus, constructQuadraticForm              G2oTypes.cpp:377-445, G2oTypes.h:324-343, 452-470
//   orbi_graph_oplus_device         oplusImpl                                                         G2oTypes.cpp:10-25
//   orbi_graph_recover_device       step 5 of the optimisers                                          Optimize.cpp:602-607, 1044-1053
//
// The float part of an edge (the deltas of the bias vertices cast to float) is orbi_imu.hip's arithmetic, from the shared orbi_so3.h;
// everything behind the cast is IEEE double, +, -, *, / in the header's orders without fused multiply-add, and the device's sin, cos,
// atan2 and sqrt.  What EdgeInertial has in common with the edges of the IMU initialisation (orbii.hip) -- the widening, the rotation
// residual and its Jacobian factors, Omega*e with chi2, the quadratic form, the refused-edge rule -- is orbi_edge.h's; ev, ep, the
// Jacobian's entries and a job of the recovery, which fullInertialOptimize's shared-bias edge (orbfi.hip) takes as they are, are
// orbi_factors_device.h's; the Huber weight and the walks are here.  The eight counters of a d_result -- the flush at a kernel's end,
// the clear kernel ahead of several workgroups and the launch of the pair (LAUNCH_COUNTED) -- are orb_device.h's and orb_host.h's.
//
// Shape: the graphs are tiny (two states for the tracker, a few tens for a local window), so every kernel is latency-bound and the
// aim is few launches and short dependent chains, not throughput.  An inertial edge is ONE WAVE, four per workgroup (k_imu's shape):
// its vertices, the 3x3 temporaries, the 9x30 Jacobian, the 9x9 information and their product live in the wave's own slice of LDS,
// the lanes are spread over matrix entries and the phases are separated by wave-level fences only.  The edge leaves its two diagonal
// blocks and its right-hand sides in the caller's workspace; then ONE WAVE PER STATE adds them up in ascending edge order, the priors
// last, so no floating-point atomic is needed and the same input gives the same bytes.  One more wave computes the priors' chi2 and
// the totals in their fixed order.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "../../include/orbi.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orb_math.h"
#include "orbi_edge.h"
#include "orbi_factors_device.h"
#include "orbi_graph_device.h"
#include "orbi_so3.h"
#include "orbi_so3d.h"

#pragma clang fp contract(off)

static_assert(sizeof(orbi_edge) == 16 && sizeof(orbi_prior) == 144 && sizeof(orbi_prior_job) == 12 && sizeof(orbi_graph) == 56,
              "orbi_factors.h fixes these layouts");

namespace {

constexpr int FAC_WAVES = 4, FAC_T = 64 * FAC_WAVES;

// ---- orbi_prior_information_device: a thread per job ---------------------------------------------------------------------------------
// one cyclic Jacobi rotation of the symmetric A on the pair (P, Q), R the third index; V collects the eigenvectors in its columns
#define JROT(P, Q, R)                                                                             \
    do {                                                                                          \
        const double apq = A[P][Q];                                                               \
        if (apq != 0.0) {                                                                         \
            const double th = (A[Q][Q] - A[P][P]) / (2.0 * apq);                                  \
            const double t = (th < 0.0 ? -1.0 : 1.0) / (fabs(th) + sqrt(th * th + 1.0));          \
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;                                  \
            const double arp = A[R][P], arq = A[R][Q];                                            \
            A[P][P] = A[P][P] - t * apq, A[Q][Q] = A[Q][Q] + t * apq;                             \
            A[P][Q] = A[Q][P] = 0.0;                                                              \
            A[R][P] = A[P][R] = c * arp - s * arq;                                                \
            A[R][Q] = A[Q][R] = s * arp + c * arq;                                                \
            _Pragma("unroll") for (int k = 0; k < 3; ++k) {                                       \
                const double vp = V[k][P], vq = V[k][Q];                                          \
                V[k][P] = c * vp - s * vq, V[k][Q] = s * vp + c * vq;                             \
            }                                                                                     \
        }                                                                                         \
    } while (0)

// the inverse of the 3x3 block of the float C at (o, o) by cofactors, in double; false when its determinant is 0
__device__ __forceinline__ bool inverse3(const float *C, int o, double inv[9])
{
    double X[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) X[k] = (double)C[15 * (o + k / 3) + o + k % 3];
    const double det = ddet(X);
#pragma unroll
    for (int k = 0; k < 9; ++k) inv[k] = dcof(X, k % 3, k / 3) / det;   // the adjugate: cofactor (j, i)
    return det != 0.0;
}

__global__ __launch_bounds__(64) void k_fac_prior_info(orbi_prior *__restrict__ priors, int n_priors, const orbi_record *__restrict__ bank, int cap,
                                                       const float *__restrict__ src, int n_src, const int32_t *__restrict__ jobs, int n,
                                                       int32_t *__restrict__ result)
{
    __shared__ int s_cnt[8];
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int job = blockIdx.x * 64 + threadIdx.x;
    if (job < n) {
        const int slot = jobs[3 * job], rec = jobs[3 * job + 1], st = jobs[3 * job + 2];
        int code = ORBI_R_DONE;
        if (slot < 0 || slot >= n_priors || rec < 0 || rec >= cap || st < -1 || st >= n_src || (st >= 0 && !src)) code = ORBI_R_RANGE;
        else if (job_named_before(jobs, 3, job, 0, slot)) code = ORBI_R_DUPLICATE;
        if (code == ORBI_R_DONE) {
            const float *C = bank[rec].C;
            double gi[9], ai[9];
            const bool ok_g = inverse3(C, 9, gi), ok_a = inverse3(C, 12, ai);
            if (!ok_g || !ok_a) code = ORBI_R_REFUSED;
            else {
                double A[3][3], V[3][3];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        A[i][j] = ((double)C[15 * (3 + i) + 3 + j] + (double)C[15 * (3 + j) + 3 + i]) / 2.0;
                        V[i][j] = i == j ? 1.0 : 0.0;
                    }
                for (int sweep = 0; sweep < ORBI_JACOBI_SWEEPS; ++sweep) {
                    JROT(0, 1, 2);
                    JROT(0, 2, 1);
                    JROT(1, 2, 0);
                }
                double lam[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) lam[k] = A[k][k] < 1e-12 ? 0.0 : A[k][k];
                orbi_prior *p = priors + slot;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        p->velo_info[3 * i + j] = (float)dsum3(dmul(dmul(V[i][0], lam[0]), V[j][0]), dmul(dmul(V[i][1], lam[1]), V[j][1]),
                                                               dmul(dmul(V[i][2], lam[2]), V[j][2]));
#pragma unroll
                for (int k = 0; k < 9; ++k) p->gyro_info[k] = (float)gi[k], p->acc_info[k] = (float)ai[k];
#pragma unroll
                for (int k = 0; k < 6; ++k) p->bias_priori[k] = bank[rec].updated_bias[k];
                if (st >= 0) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) p->velo_priori[k] = src[15 * (size_t)st + 12 + k];
                }
            }
        }
        atomicAdd(&s_cnt[code], 1);
    }
    __syncthreads();
    flush_counts(s_cnt, result);
}

// ---- orbi_graph_init_device / orbi_graph_oplus_device / orbi_graph_recover_device: a thread per job or state ------------------------------
__global__ __launch_bounds__(64) void k_fac_init(const orbi_graph g, const orbi_record *__restrict__ bank, int cap, const float *__restrict__ src,
                                                 int n_src, const int32_t *__restrict__ jobs, int n, int32_t *__restrict__ result)
{
    __shared__ int s_cnt[8];
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int job = blockIdx.x * 64 + threadIdx.x;
    if (job < n) {
        const int st = jobs[3 * job], from = jobs[3 * job + 1], rec = jobs[3 * job + 2];
        int code = ORBI_R_DONE;
        if (st < 0 || st >= g.n_states || from < 0 || from >= n_src || rec < -1 || rec >= cap) code = ORBI_R_RANGE;
        else if (job_named_before(jobs, 3, job, 0, st)) code = ORBI_R_DUPLICATE;
        if (code == ORBI_R_DONE) {
            const float *f = src + 15 * (size_t)from;
            for (int k = 0; k < 9; ++k) g.Rwb[9 * (size_t)st + k] = (double)f[k];
            for (int k = 0; k < 3; ++k) {
                g.twb[3 * (size_t)st + k] = (double)f[9 + k];
                g.v[3 * (size_t)st + k] = (double)f[12 + k];
                g.bg[3 * (size_t)st + k] = rec >= 0 ? (double)bank[rec].updated_bias[k] : 0.0;
                g.ba[3 * (size_t)st + k] = rec >= 0 ? (double)bank[rec].updated_bias[3 + k] : 0.0;
            }
        }
        atomicAdd(&s_cnt[code], 1);
    }
    __syncthreads();
    flush_counts(s_cnt, result);
}

__global__ __launch_bounds__(64) void k_fac_oplus(const orbi_graph g, const double *__restrict__ dx, int32_t *__restrict__ iter,
                                                  int32_t *__restrict__ result)
{
    __shared__ int s_cnt[8];
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s < g.n_states) {
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
        if ((fixed & 15) != 15) atomicAdd(&s_cnt[ORBI_R_DONE], 1);
    }
    __syncthreads();
    flush_counts(s_cnt, result);
}

__global__ __launch_bounds__(64) void k_fac_recover(const orbi_graph g, const orbi_calib cal, const int32_t *__restrict__ jobs, int n,
                                                    float *__restrict__ dst, int n_dst, float *__restrict__ bias, double *__restrict__ pose_R,
                                                    double *__restrict__ pose_t, int32_t *__restrict__ result)
{
    __shared__ int s_cnt[8];
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int job = blockIdx.x * 64 + threadIdx.x;
    if (job < n) {
        const int st = jobs[3 * job], to = jobs[3 * job + 1], flags = jobs[3 * job + 2];
        const int code = recover_job(g, cal, jobs, job, st, to, flags, st, dst, n_dst, bias, pose_R, pose_t);   // the biases are the state's own
        atomicAdd(&s_cnt[code], 1);
    }
    __syncthreads();
    flush_counts(s_cnt, result);
}

// ---- orbi_edge_information_device: a wave per edge -------------------------------------------------------------------------------------
// Gauss-Jordan with partial pivoting on the augmented [C | I] (9 x 18) in the wave's LDS slice; then the two walk blocks by cofactors
__global__ __launch_bounds__(FAC_T) void k_fac_edge_info(const orbi_record *__restrict__ bank, int cap, const orbi_edge *__restrict__ edges, int n_edges,
                                                         double *__restrict__ info, double *__restrict__ walk_info, int32_t *__restrict__ result)
{
    __shared__ int s_cnt[8];
    __shared__ double s_m[FAC_WAVES][162 + 18];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int e = blockIdx.x * FAC_WAVES + wave;
    if (e < n_edges) {
        double *M = s_m[wave], *Wk = s_m[wave] + 162;
        const int rec = __builtin_amdgcn_readfirstlane(edges[e].rec), flags = __builtin_amdgcn_readfirstlane(edges[e].flags);
        int code = ORBI_R_DONE;
        bool walk_ok[2] = {false, false};
        if (rec < 0 || rec >= cap) code = ORBI_R_RANGE;
        else {
            const float *C = bank[rec].C;
            for (int x = lane; x < 162; x += 64) {
                const int r = x / 18, c = x - 18 * r;
                M[x] = c < 9 ? (double)C[15 * r + c] : (c - 9 == r ? 1.0 : 0.0);
            }
            if (lane < 18) Wk[lane] = (double)C[15 * (9 + 3 * (lane / 9) + (lane % 9) / 3) + 9 + 3 * (lane / 9) + lane % 3];
            WSYNC();
            for (int k = 0; k < 9; ++k) {
                int p = k;                       // the first row of the largest |entry| in column k, rows k .. 8: the same in every lane
                double best = fabs(M[18 * k + k]);
                for (int r = k + 1; r < 9; ++r) {
                    const double v = fabs(M[18 * r + k]);
                    if (v > best) best = v, p = r;
                }
                if (!(best > 0.0)) { code = ORBI_R_REFUSED; break; }
                if (p != k) {
                    double u = 0.0, v = 0.0;
                    if (lane < 18) u = M[18 * k + lane], v = M[18 * p + lane];
                    WSYNC();
                    if (lane < 18) M[18 * k + lane] = v, M[18 * p + lane] = u;
                    WSYNC();
                }
                const double piv = M[18 * k + k];
                double val[3];
#pragma unroll
                for (int h = 0; h < 3; ++h) {
                    const int x = lane + 64 * h;
                    val[h] = 0.0;
                    if (x < 162) {
                        const int r = x / 18, c = x - 18 * r;
                        const double pr = M[18 * k + c] / piv;
                        val[h] = r == k ? pr : M[x] - dmul(M[18 * r + k], pr);
                    }
                }
                WSYNC();
#pragma unroll
                for (int h = 0; h < 3; ++h)
                    if (lane + 64 * h < 162) M[lane + 64 * h] = val[h];
                WSYNC();
            }
            const double d0 = ddet(Wk), d1 = ddet(Wk + 9);
            walk_ok[0] = d0 != 0.0, walk_ok[1] = d1 != 0.0;
            if (code == ORBI_R_DONE && (flags & ORBI_EDGE_WALKS) && !(walk_ok[0] && walk_ok[1])) code = ORBI_R_REFUSED;
        }
        for (int x = lane; x < 81; x += 64) {
            const int r = x / 9, c = x - 9 * r;
            info[81 * (size_t)e + x] = code == ORBI_R_DONE ? (M[18 * r + 9 + c] + M[18 * c + 9 + r]) / 2.0 : 0.0;
        }
        if (lane < 18) {
            const int b = lane / 9, k = lane - 9 * b;
            double v = 0.0;
            if (code == ORBI_R_DONE && (b == 0 ? walk_ok[0] : walk_ok[1])) v = dcof(Wk + 9 * b, k % 3, k / 3) / ddet(Wk + 9 * b);
            walk_info[18 * (size_t)e + lane] = v;
        }
        if (lane == 0) atomicAdd(&s_cnt[code], 1);
    }
    __syncthreads();
    flush_counts(s_cnt, result);
}

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

static_assert(X_WORDS == 140 && D_WORDS == 825, "include/orbi.h states the LDS of k_fac_edge");

__global__ __launch_bounds__(FAC_T) void k_fac_edge(const LinArgs a)
{
    __shared__ __attribute__((aligned(16))) double s_d[FAC_WAVES][D_WORDS];
    __shared__ float s_f[FAC_WAVES][X_WORDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e = blockIdx.x * FAC_WAVES + wave;
    if (e >= a.n_edges) return;                      // no workgroup barrier in this kernel
    double *S = s_d[wave];
    float *F = s_f[wave];
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
        if (a.mode == 0) {
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
    if (a.mode != 0) return;
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

// mode 0: waves [0, n_states) gather a state each; the last wave (the only one of mode 1) does the priors' chi2, the totals, d_result
__global__ __launch_bounds__(FAC_T) void k_fac_gather(const LinArgs a)
{
    __shared__ int s_cnt[8];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_gather = a.mode == 0 ? a.g.n_states : 0;
    const int s = blockIdx.x * FAC_WAVES + wave;
    if (s < n_gather) {
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
    if (s != n_gather) return;                                // uniform per wave; the tail wave alone uses s_cnt
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
    if (lane < 8) a.result[lane] = s_cnt[lane];
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

int check_graph(const orbi_graph &g, const void *result)
{
    if (!g.Rwb || !g.twb || !g.v || !g.bg || !g.ba || !g.fixed || g.n_states < 0 || !result)
        return orbx_set_error(ORBX_E_ARG, "null graph array or result, or a negative state count");
    if (g.n_states > ORBI_MAX_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBI_MAX_JOBS (4096) states");
    return ORBX_OK;
}

int check_jobs(const void *jobs, int n, const void *result)
{
    if (!jobs || n < 0 || !result) return orbx_set_error(ORBX_E_ARG, "null job list or result, or a negative job count");
    if (n > ORBI_MAX_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBI_MAX_JOBS (4096) jobs in one call");
    return ORBX_OK;
}

} // namespace

extern "C" int orbi_prior_information_device(orbi_prior *d_priors, int n_priors, const orbi_record *d_bank, int cap, const float *d_src, int n_src,
                                             const int32_t *d_jobs, int n, int32_t *d_result, void *stream)
{
    if (int rc = check_jobs(d_jobs, n, d_result)) return rc;
    if (!d_priors || n_priors < 1 || !d_bank || cap < 1 || n_src < 0) return orbx_set_error(ORBX_E_ARG, "null priors or bank, n_priors or cap < 1, or a negative n_src");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int grid = (n + 63) / 64;
    LAUNCH_COUNTED(k_fac_prior_info, grid, 64, s, d_result, d_priors, n_priors, d_bank, cap, d_src, n_src, d_jobs, n, d_result);
    return ORBX_OK;
}

extern "C" int orbi_graph_init_device(orbi_graph graph, const orbi_record *d_bank, int cap, const float *d_src, int n_src, const int32_t *d_jobs, int n,
                                      int32_t *d_result, void *stream)
{
    if (int rc = check_graph(graph, d_result)) return rc;
    if (int rc = check_jobs(d_jobs, n, d_result)) return rc;
    if (!d_bank || cap < 1 || !d_src || n_src < 1) return orbx_set_error(ORBX_E_ARG, "null bank or source states, or cap or n_src < 1");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int grid = (n + 63) / 64;
    LAUNCH_COUNTED(k_fac_init, grid, 64, s, d_result, graph, d_bank, cap, d_src, n_src, d_jobs, n, d_result);
    return ORBX_OK;
}

extern "C" int orbi_edge_information_device(const orbi_record *d_bank, int cap, const orbi_edge *d_edges, int n_edges, double *d_info,
                                            double *d_walk_info, int32_t *d_result, void *stream)
{
    if (int rc = check_jobs(d_edges, n_edges, d_result)) return rc;
    if (!d_bank || cap < 1 || !d_info || !d_walk_info) return orbx_set_error(ORBX_E_ARG, "null bank, d_info or d_walk_info, or cap < 1");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int grid = (n_edges + FAC_WAVES - 1) / FAC_WAVES;
    LAUNCH_COUNTED(k_fac_edge_info, grid, FAC_T, s, d_result, d_bank, cap, d_edges, n_edges, d_info, d_walk_info, d_result);
    return ORBX_OK;
}

extern "C" int orbi_linearize_device(orbi_graph graph, const orbi_record *d_bank, int cap, float gravity, const orbi_edge *d_edges, int n_edges,
                                     const double *d_info, const double *d_walk_info, const orbi_prior *d_priors, int n_priors,
                                     const orbi_prior_job *d_prior_jobs, int n_prior_jobs, double huber_delta, int mode, double *d_work,
                                     double *d_err, double *d_chi2, double *d_chi2_prior, double *d_total, double *d_H_diag, double *d_H_off,
                                     double *d_b, double *d_J, float *d_float, int32_t *d_result, void *stream)
{
    if (int rc = check_graph(graph, d_result)) return rc;
    if (int rc = check_jobs(d_edges, n_edges, d_result)) return rc;
    if (n_prior_jobs < 0 || n_priors < 0 || (n_prior_jobs > 0 && (!d_prior_jobs || !d_priors || !d_chi2_prior)))
        return orbx_set_error(ORBX_E_ARG, "prior jobs without their list, the priors or d_chi2_prior, or a negative count");
    if (n_prior_jobs > ORBI_MAX_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBI_MAX_JOBS (4096) prior jobs in one call");
    if (!d_bank || cap < 1 || !d_info || !d_walk_info || !d_work || !d_err || !d_chi2 || !d_total || !(huber_delta == huber_delta))
        return orbx_set_error(ORBX_E_ARG, "null bank, information, workspace or output, cap < 1, or huber_delta is not a number");
    if (mode != 0 && mode != 1) return orbx_set_error(ORBX_E_ARG, "mode is 0 (linearise) or 1 (computeError only)");
    if (mode == 0 && (!d_H_diag || !d_H_off || !d_b)) return orbx_set_error(ORBX_E_ARG, "mode 0 needs d_H_diag, d_H_off and d_b");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    LinArgs a = {};
    a.g = graph, a.bank = d_bank, a.cap = cap, a.gravity = gravity, a.edges = d_edges, a.n_edges = n_edges, a.info = d_info, a.walk_info = d_walk_info;
    a.priors = d_priors, a.n_priors = n_priors, a.pjobs = d_prior_jobs, a.n_pjobs = n_prior_jobs, a.delta = huber_delta, a.mode = mode;
    a.work = d_work, a.err = d_err, a.chi2 = d_chi2, a.chi2_prior = d_chi2_prior, a.total = d_total, a.H_diag = d_H_diag, a.H_off = d_H_off;
    a.b = d_b, a.J = mode == 0 ? d_J : nullptr, a.flt = d_float, a.result = d_result;
    if (n_edges > 0) hipLaunchKernelGGL(k_fac_edge, dim3((n_edges + FAC_WAVES - 1) / FAC_WAVES), dim3(FAC_T), 0, s, a);
    const int waves = (mode == 0 ? graph.n_states : 0) + 1;
    hipLaunchKernelGGL(k_fac_gather, dim3((waves + FAC_WAVES - 1) / FAC_WAVES), dim3(FAC_T), 0, s, a);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbi_graph_oplus_device(orbi_graph graph, const double *d_dx, int32_t *d_iter, int32_t *d_result, void *stream)
{
    if (int rc = check_graph(graph, d_result)) return rc;
    if (!d_dx || !d_iter) return orbx_set_error(ORBX_E_ARG, "null d_dx or d_iter");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int grid = (graph.n_states + 63) / 64;
    LAUNCH_COUNTED(k_fac_oplus, grid, 64, s, d_result, graph, d_dx, d_iter, d_result);
    return ORBX_OK;
}

extern "C" int orbi_graph_recover_device(orbi_graph graph, orbi_calib calib, const int32_t *d_jobs, int n, float *d_dst, int n_dst, float *d_bias,
                                         double *d_pose_R, double *d_pose_t, int32_t *d_result, void *stream)
{
    if (int rc = check_graph(graph, d_result)) return rc;
    if (int rc = check_jobs(d_jobs, n, d_result)) return rc;
    if (!d_dst || n_dst < 1 || !d_bias) return orbx_set_error(ORBX_E_ARG, "null destination or bias array, or n_dst < 1");
    if (!d_pose_R != !d_pose_t) return orbx_set_error(ORBX_E_ARG, "d_pose_R and d_pose_t go together");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int grid = (n + 63) / 64;
    LAUNCH_COUNTED(k_fac_recover, grid, 64, s, d_result, graph, calib, d_jobs, n, d_dst, n_dst, d_bias, d_pose_R, d_pose_t, d_result);
    return ORBX_OK;
}
