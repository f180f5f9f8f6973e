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
#include "orbvi_stages.h"

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
        if (fac_oplus_state(g, dx, iter, s)) atomicAdd(&s_cnt[ORBI_R_DONE], 1);
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

// ---- orbi_linearize_device: the wave of an edge, the wave of a state and the tail wave are orbvi_stages.h's ----------------------------------
// which k_vi_pose_loop (orbvi_loop.hip) runs as well: a kernel here owns its LDS, its launch shape and its counters.  fac_edge_wave is, in
// the order k_fac_edge had them: edge_valid(), edge_refused(), edge_load(), bias_deltas(), edge_widen(), edge_velocity_position(),
// edge_rotation(), edge_chi2(), jac_entry() under dof_fixed(), edge_quadratic_form<30>() and edge_jtwj<30>(); fac_oplus_state is
// CameraImuPose::update on dexp_so3().
static_assert(X_WORDS == 140 && D_WORDS == 825, "include/orbi.h states the LDS of k_fac_edge");

__global__ __launch_bounds__(FAC_T) void k_fac_edge(const LinArgs a)
{
    __shared__ __attribute__((aligned(16))) double s_d[FAC_WAVES][D_WORDS];
    __shared__ float s_f[FAC_WAVES][X_WORDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e = blockIdx.x * FAC_WAVES + wave;
    if (e >= a.n_edges) return;                      // no workgroup barrier in this kernel
    fac_edge_wave(a, a.mode, e, s_d[wave], s_f[wave], lane);
}

// mode 0: waves [0, n_states) gather a state each; the last wave (the only one of mode 1) does the priors' chi2, the totals, d_result
__global__ __launch_bounds__(FAC_T) void k_fac_gather(const LinArgs a)
{
    __shared__ int s_cnt[8];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_gather = a.mode == 0 ? a.g.n_states : 0;
    const int s = blockIdx.x * FAC_WAVES + wave;
    if (s < n_gather) fac_gather_state(a, s, lane);
    if (s != n_gather) return;                                // uniform per wave; the tail wave alone uses s_cnt
    fac_gather_tail(a, s_cnt, lane);
    if (lane < 8) a.result[lane] = s_cnt[lane];
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
