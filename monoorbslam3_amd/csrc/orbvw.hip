// The visual window of the inertial local bundle adjustment on the device (include/orbvw.h):
//   orbvw_linearize_device   EdgeMono on a VertexPose and a Vertex3D: computeError, linearizeOplus, constructQuadraticForm   G2oTypes.cpp:59-69
//                            and the outlier classification of localFullBundleAdjustment                                   Optimize.cpp:1255-1261
//   orbvw_reduce_device      the Schur complement over the marginalised points of g2o's BlockSolverX                       Optimize.cpp:1073-1078
//   orbvw_solve_device       the reduced system, by orbvi.h's ordered Cholesky, for up to 480 unknowns
//   orbvw_backsub_device     the points' step and their share of computeScale
//
// Everything is IEEE double in the header's orders without fused multiply-add; the camera is csrc/orbba_camera.h; the pose derivation,
// the pose Jacobian, the quadratic form on a pose and the host checks are the ones k_vi_linearize uses, from csrc/orbi_graph_device.h.
//
// Shape: every call is latency-bound.  An edge is a thread; a point is a thread that walks its edges in order; a state's 6 x 6 block and
// a pair's Schur block are ONE workgroup each with k_vi_linearize's register partials, wave butterfly and ordered wave slots, so no
// floating-point atomic is needed and the same input gives the same bytes.  The solve keeps the matrix in the caller's d_S, a thread
// per row: a column of L is mirrored into the upper triangle so that the inner product of a step reads along rows.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include <string>

#include "../../include/orbvw.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orb_math.h"
#include "orbba_camera.h"
#include "orbi_graph_device.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- orbvw_linearize_device ------------------------------------------------------------------------------------------------------------
enum { W_JP = 0, W_JL = 12, W_W = 18, W_WE = 19, W_USED = 21, W_FREE = 22 };   // an edge's workspace: J_p (2 x 6), J_l (2 x 3), w*Omega, (w*Omega)*e, flags
static_assert(W_FREE + 2 == ORBVW_EDGE_WORK, "orbvw.h states the workspace of an edge");
constexpr int ST_T = 1024, ST_WAVES = ST_T / 64, ST_SUMS = 27;                  // k_vw_state: H's upper triangle row by row (21), g (6)

struct VwArgs {
    orbi_graph g;
    orbi_calib cal;
    BaCam cam;                      // delta: huber_delta
    int n_solve, n_points, n_edges;
    const double *points;
    const int32_t *edge_state, *edge_point;
    const double *z, *w;
    const uint8_t *active;
    double threshold;
    int mode;
    int32_t *off;
    double *work, *err, *chi2, *total, *H, *b, *Hll, *bl, *Hlp;
    uint8_t *outlier;
    int32_t *result;
};

// d_point_off: every entry starts at the edge count (and d_result at zero) ...
__global__ __launch_bounds__(256) void k_vw_off_init(int n, int n_edges, int32_t *__restrict__ off, int32_t *__restrict__ result)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l < n) off[l] = n_edges;
    if (blockIdx.x == 0 && threadIdx.x < 8) result[threadIdx.x] = 0;
}
// ... takes the first edge of every clamped point index (an integer minimum: no order reaches the result) ...
__global__ __launch_bounds__(256) void k_vw_off_first(int n_edges, int n_points, const int32_t *__restrict__ edge_point, int32_t *__restrict__ off)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n_edges) atomicMin(&off[clampi(edge_point[e], 0, n_points - 1)], e);
}
// ... and the suffix minimum makes off[l] the first edge whose clamped index is >= l: the edge's point is then the running maximum.
// One workgroup; thread t owns a contiguous chunk.
__global__ __launch_bounds__(1024) void k_vw_off_scan(int n, int32_t *__restrict__ off)
{
    __shared__ int s_min[1024];
    const int t = threadIdx.x, chunk = (n + 1023) / 1024, lo = min(t * chunk, n), hi = min(lo + chunk, n);
    int m = INT_MAX;
    for (int k = lo; k < hi; ++k) m = min(m, off[k]);
    s_min[t] = m;
    __syncthreads();
    int run = INT_MAX;
    for (int k = t + 1; k < 1024; ++k) run = min(run, s_min[k]);
    for (int k = hi - 1; k >= lo; --k) {
        run = min(run, off[k]);
        off[k] = run;
    }
}

// an edge is a thread: its point, its status, computeError and (mode 0) linearizeOplus into the workspace
__global__ __launch_bounds__(256) void k_vw_edge(const VwArgs a)
{
    __shared__ int s_cnt[8];
    const int t = threadIdx.x, e = blockIdx.x * 256 + t;
    if (t < 8) s_cnt[t] = 0;
    __syncthreads();
    int n_done = 0, n_range = 0, n_dup = 0, n_ref = 0, n_bad = 0, n_out = 0;
    if (e < a.n_edges) {
        int l = 0, above = a.n_points;                    // off[l] <= e < off[above]
        while (above - l > 1) {
            const int mid = (l + above) >> 1;
            if (a.off[mid] <= e) l = mid; else above = mid;
        }
        const int lo = a.off[l], hi = a.off[l + 1], st = a.edge_state[e];
        int code = ORBI_R_DONE;
        if (hi - lo > ORBVW_MAX_OBS) code = ORBI_R_REFUSED, n_ref = e == lo;
        else if (st < 0 || st >= a.g.n_states) code = ORBI_R_RANGE, n_range = 1;
        else {
            for (int k = lo; k < e; ++k)
                if (a.edge_state[k] == st) code = ORBI_R_DUPLICATE;
            n_dup = code == ORBI_R_DUPLICATE;
        }
        double *work = a.mode == 0 ? a.work + (size_t)ORBVW_EDGE_WORK * e : nullptr;
        double *Hlp = a.mode == 0 ? a.Hlp + 18 * (size_t)e : nullptr;
        bool used = false;
        if (code != ORBI_R_DONE) {
            a.err[2 * (size_t)e] = 0.0, a.err[2 * (size_t)e + 1] = 0.0, a.chi2[e] = 0.0;
            if (a.mode == 2) a.outlier[e] = 0;
        } else {
            n_done = 1;
            // the pose the edge hangs on, derived from (R_wb, t_wb), and the calibration widened
            const double *Rwb = a.g.Rwb + 9 * (size_t)st, *twb = a.g.twb + 3 * (size_t)st;
            double R[9], C[9], tcw[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = pose_rcw(a.cal, Rwb, k), C[k] = (double)a.cal.Rcb[k];
#pragma unroll
            for (int i = 0; i < 3; ++i) tcw[i] = pose_tcw(a.cal, R, twb, i);
            const double Px = a.points[3 * (size_t)l], Py = a.points[3 * (size_t)l + 1], Pz = a.points[3 * (size_t)l + 2];
            const double X = dsum3(R[0] * Px, R[1] * Py, R[2] * Pz) + tcw[0];
            const double Y = dsum3(R[3] * Px, R[4] * Py, R[5] * Pz) + tcw[1];
            const double Z = dsum3(R[6] * Px, R[7] * Py, R[8] * Pz) + tcw[2];
            double u, v;
            ba_project(a.cam, X, Y, Z, &u, &v);
            const double ex = a.z[2 * (size_t)e] - u, ey = a.z[2 * (size_t)e + 1] - v;
            const double om = a.w[e];
            const double chi = om * (ex * ex + ey * ey);
            a.err[2 * (size_t)e] = ex, a.err[2 * (size_t)e + 1] = ey;
            a.chi2[e] = chi;
            const bool finite = isfinite(ex) && isfinite(ey) && isfinite(chi);
            if (a.mode == 2) {
                const bool out = chi > a.threshold;
                a.outlier[e] = out ? 1 : 0;
                n_out = out, n_bad = !finite;
            } else if (!a.active || a.active[e]) {
                n_bad = !finite;
                used = finite;
            }
            if (a.mode == 0 && used) {
                double rho, rw;
                huber(chi, a.cam.delta, rho, rw);
                const double W = rw * om;
                const bool pose_free = st < a.n_solve && !(a.g.fixed[st] & ORBI_FIX_POSE);
                double Jp[6], Jl[6], J[12];
                ba_proj_jacobian(a.cam, X, Y, Z, Jp);
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) Jl[3 * r + c] = dsum3(-Jp[3 * r] * R[c], -Jp[3 * r + 1] * R[3 + c], -Jp[3 * r + 2] * R[6 + c]);
#pragma unroll
                for (int k = 0; k < 12; ++k) J[k] = 0.0;
                if (pose_free) {            // linearizeOplus on the pose
                    double tbc[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) tbc[i] = pose_tbc(a.cal, i);
                    pose_jacobian(C, tbc, Jp, X, Y, Z, J);
                }
#pragma unroll
                for (int k = 0; k < 12; ++k) work[W_JP + k] = J[k];
#pragma unroll
                for (int k = 0; k < 6; ++k) work[W_JL + k] = Jl[k];
                work[W_W] = W, work[W_WE] = W * ex, work[W_WE + 1] = W * ey, work[W_FREE] = pose_free ? 1.0 : 0.0, work[W_FREE + 1] = 0.0;
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 6; ++c) Hlp[6 * r + c] = pose_free ? Jl[r] * (W * J[c]) + Jl[3 + r] * (W * J[6 + c]) : 0.0;
            }
        }
        if (a.mode == 0) {
            work[W_USED] = used ? 1.0 : 0.0;
            if (!used) {
#pragma unroll
                for (int k = 0; k < 18; ++k) Hlp[k] = 0.0;
            }
        }
    }
    block_add(s_cnt, {ORBI_R_DONE, ORBI_R_RANGE, ORBI_R_DUPLICATE, ORBI_R_REFUSED, ORBVI_R_NONFINITE, ORBVW_R_OUTLIER}, {n_done, n_range, n_dup, n_ref, n_bad, n_out});
    __syncthreads();
    if (t < 8 && s_cnt[t]) atomicAdd(&a.result[t], s_cnt[t]);
}

// a point is a thread: H_ll and b_l over its used edges in ascending order
__global__ __launch_bounds__(256) void k_vw_point(const VwArgs a)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= a.n_points) return;
    const int lo = a.off[l], hi = a.off[l + 1];
    double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
    for (int e = lo; e < hi && hi - lo <= ORBVW_MAX_OBS; ++e) {
        const double *work = a.work + (size_t)ORBVW_EDGE_WORK * e;
        if (work[W_USED] == 0.0) continue;
        double J[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) J[k] = work[W_JL + k];
        const double W = work[W_W], wex = work[W_WE], wey = work[W_WE + 1];
        int k = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c, ++k) h[k] = h[k] + (J[r] * (W * J[c]) + J[3 + r] * (W * J[3 + c]));
#pragma unroll
        for (int r = 0; r < 3; ++r) g[r] = g[r] + (J[r] * wex + J[3 + r] * wey);
    }
    double *H = a.Hll + 9 * (size_t)l;
    H[0] = h[0], H[1] = h[1], H[2] = h[2], H[3] = h[1], H[4] = h[3], H[5] = h[4], H[6] = h[2], H[7] = h[4], H[8] = h[5];
#pragma unroll
    for (int r = 0; r < 3; ++r) a.bl[3 * (size_t)l + r] = 0.0 - g[r];
}

// a state's pose block is a workgroup that walks all edges; the workgroup behind the last state sums the totals
__global__ __launch_bounds__(ST_T) void k_vw_state(const VwArgs a, int n_state_blocks)
{
    __shared__ double s_part[ST_WAVES][ST_SUMS];
    const int t = threadIdx.x, s = blockIdx.x;
    const bool totals = s == n_state_blocks;
    if (!totals && (a.g.fixed[s] & ORBI_FIX_POSE)) return;    // uniform
    double acc[ST_SUMS];
#pragma unroll
    for (int k = 0; k < ST_SUMS; ++k) acc[k] = 0.0;
    if (totals) {
        for (int e = t; e < a.n_edges; e += ST_T) {
            if (a.active && !a.active[e]) continue;
            const double chi = a.chi2[e], ex = a.err[2 * (size_t)e], ey = a.err[2 * (size_t)e + 1];
            if (!(isfinite(ex) && isfinite(ey) && isfinite(chi))) continue;
            double rho, rw;
            huber(chi, a.cam.delta, rho, rw);
            acc[0] = acc[0] + chi, acc[1] = acc[1] + rho;
        }
    } else {
        for (int e = t; e < a.n_edges; e += ST_T) {
            if (a.edge_state[e] != s) continue;
            const double *work = a.work + (size_t)ORBVW_EDGE_WORK * e;
            if (work[W_USED] == 0.0) continue;
            quad_accumulate(work + W_JP, work[W_W], work[W_WE], work[W_WE + 1], acc);
        }
    }
    block_sums_put(acc, s_part, 0, totals ? 2 : ST_SUMS);
    __syncthreads();
    if (t >= (totals ? 2 : ST_SUMS)) return;
    const double sum = block_sums_get(s_part, t);
    if (totals) a.total[t] = sum;
    else quad_scatter(t, sum, a.H + 225 * (size_t)s, a.b + 15 * (size_t)s);
}

// ---- orbvw_reduce_device ------------------------------------------------------------------------------------------------------------------
struct RdArgs {
    int n_solve, n_edges, cap, n_points, cap_edges;
    const uint8_t *fixed;
    const orbi_edge *edges;
    const double *H_diag, *H_off, *b, *lambda;
    const int32_t *off, *edge_state;
    const double *Hll, *bl, *Hlp;
    double *S, *rhs, *inv, *tl, *out;
    int32_t *result;
};

__device__ __forceinline__ bool point_skipped(const double *__restrict__ inv)
{
    bool any = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) any |= inv[k] != 0.0;
    return !any;
}

__global__ __launch_bounds__(256) void k_vw_point_inv(int n_points, const double *__restrict__ lambda, const double *__restrict__ Hll,
                                                      const double *__restrict__ bl, double *__restrict__ inv, double *__restrict__ tl)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n_points) return;
    const double lam = *lambda;
    const double *h = Hll + 9 * (size_t)l;
    const double a = h[0] + lam, b = h[1], c = h[2], d = h[4] + lam, e = h[5], f = h[8] + lam;
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
    const double det = dsum3(a * c00, b * c01, c * c02);
    double m[9], t[3];
    if (det > 0.0 && isfinite(det)) {
        const double id = 1.0 / det;
        m[0] = c00 * id, m[1] = c01 * id, m[2] = c02 * id;
        m[3] = m[1], m[4] = (a * f - c * c) * id, m[5] = (b * c - a * e) * id;
        m[6] = m[2], m[7] = m[5], m[8] = (a * d - b * b) * id;
        const double b0 = bl[3 * (size_t)l], b1 = bl[3 * (size_t)l + 1], b2 = bl[3 * (size_t)l + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r) t[r] = dsum3(m[3 * r] * b0, m[3 * r + 1] * b1, m[3 * r + 2] * b2);
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = 0.0;
        t[0] = t[1] = t[2] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) inv[9 * (size_t)l + k] = m[k];
#pragma unroll
    for (int r = 0; r < 3; ++r) tl[3 * (size_t)l + r] = t[r];
}

// the base: a thread per entry of d_S; the block behind the last writes the right-hand side, d_out[1] and d_result
__global__ __launch_bounds__(256) void k_vw_base(const RdArgs a)
{
    __shared__ double s_max[4];
    __shared__ int s_cnt[8];
    const int t = threadIdx.x, N = 15 * a.n_solve;
    if (blockIdx.x + 1 < gridDim.x) {
        const int x = blockIdx.x * 256 + t;
        if (x >= N * N) return;
        const int R = x / N, C = x - N * R, si = R / 15, r = R - 15 * si, sj = C / 15, c = C - 15 * sj;
        double v = 0.0;
        if (dof_fixed(a.fixed[si], r) || dof_fixed(a.fixed[sj], c)) v = R == C ? 1.0 : 0.0;
        else if (si == sj) v = a.H_diag[225 * (size_t)si + 15 * r + c] + (r == c ? *a.lambda : 0.0);
        else
            for (int e = 0; e < a.n_edges; ++e) {     // ascending: several edges on one pair add up in edge order
                const int i = a.edges[e].i, j = a.edges[e].j;
                if (!edge_valid(i, j, a.edges[e].rec, a.n_solve, a.cap)) continue;
                if (i == si && j == sj) v = v + a.H_off[225 * (size_t)e + 15 * r + c];
                else if (i == sj && j == si) v = v + a.H_off[225 * (size_t)e + 15 * c + r];
            }
        a.S[x] = v;
        return;
    }
    if (t < 8) s_cnt[t] = 0;
    __syncthreads();
    int n_range = 0, n_sing = 0;
    double h_max = 0.0;
    for (int e = t; e < a.n_edges; e += 256) n_range += !edge_valid(a.edges[e].i, a.edges[e].j, a.edges[e].rec, a.n_solve, a.cap);
    for (int R = t; R < N; R += 256) {
        const int s = R / 15, r = R - 15 * s;
        const bool fre = !dof_fixed(a.fixed[s], r);
        a.rhs[R] = fre ? a.b[R] : 0.0;
        const double h = a.H_diag[225 * (size_t)s + 16 * r];
        if (fre && h > h_max) h_max = h;
    }
    for (int l = t; l < a.n_points; l += 256) {
        n_sing += point_skipped(a.inv + 9 * (size_t)l);
#pragma unroll
        for (int k = 0; k < 9; k += 4) {
            const double h = a.Hll[9 * (size_t)l + k];
            if (h > h_max) h_max = h;
        }
    }
    h_max = wave_max(h_max);
    if ((t & 63) == 0) s_max[t >> 6] = h_max;
    block_add(s_cnt, {ORBI_R_RANGE, ORBVW_R_POINT_SINGULAR}, {n_range, n_sing});
    __syncthreads();
    if (t == 0) a.out[1] = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    if (t < 8) a.result[t] = t == ORBI_R_DONE ? 1 : s_cnt[t];
}

constexpr int SC_T = 256, SC_WAVES = SC_T / 64, SC_SUMS = 42;
__global__ __launch_bounds__(SC_T) void k_vw_schur(const RdArgs a)
{
    __shared__ double s_part[SC_WAVES][SC_SUMS];
    int i = 0, rem = blockIdx.x;                   // block index -> (i, j >= i)
    while (rem >= a.n_solve - i) rem -= a.n_solve - i, ++i;
    const int j = i + rem, t = threadIdx.x, N = 15 * a.n_solve;
    if ((a.fixed[i] & ORBI_FIX_POSE) || (a.fixed[j] & ORBI_FIX_POSE)) return;     // uniform
    double acc[SC_SUMS];
#pragma unroll
    for (int k = 0; k < SC_SUMS; ++k) acc[k] = 0.0;
    for (int l = t; l < a.n_points; l += SC_T) {
        const int lo = clampi(a.off[l], 0, a.cap_edges), hi = max(lo, clampi(a.off[l + 1], 0, a.cap_edges));
        if (hi - lo > ORBVW_MAX_OBS) continue;
        int ea = -1, eb = -1;
        for (int e = hi - 1; e >= lo; --e) {      // descending, so that the first edge of the range on a state stays
            const int st = a.edge_state[e];
            if (st == i) ea = e;
            if (st == j) eb = e;
        }
        if (ea < 0 || eb < 0) continue;
        const double *m = a.inv + 9 * (size_t)l;
        if (point_skipped(m)) continue;
        const double *A = a.Hlp + 18 * (size_t)ea, *B = a.Hlp + 18 * (size_t)eb;
        double Cm[18];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) Cm[6 * r + c] = dsum3(m[3 * r] * B[c], m[3 * r + 1] * B[6 + c], m[3 * r + 2] * B[12 + c]);
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) acc[6 * r + c] = acc[6 * r + c] + dsum3(A[r] * Cm[c], A[6 + r] * Cm[6 + c], A[12 + r] * Cm[12 + c]);
        if (i == j) {
            const double *tl = a.tl + 3 * (size_t)l;
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[36 + r] = acc[36 + r] + dsum3(A[r] * tl[0], A[6 + r] * tl[1], A[12 + r] * tl[2]);
        }
    }
    block_sums_put(acc, s_part);
    __syncthreads();
    if (t >= SC_SUMS) return;
    const double sum = block_sums_get(s_part, t);
    if (t < 36) {
        const int r = t / 6, c = t - 6 * r;
        if (i == j && r > c) return;
        double *p = a.S + (size_t)(15 * i + r) * N + 15 * j + c, *q = a.S + (size_t)(15 * j + c) * N + 15 * i + r;
        *p = *p - sum;
        if (p != q) *q = *q - sum;
    } else if (i == j) {
        double *p = a.rhs + 15 * i + t - 36;
        *p = *p - sum;
    }
}

// ---- orbvw_solve_device: one workgroup, a thread per row, the matrix in global memory ------------------------------------------------------
// Left-looking in block columns of 15.  For a block starting at column B a thread first adds, for all 15 columns at once, the products
// over k < B (its own row of L read along the mirror rows, the block's 15 rows of L from LDS): one load feeds 15 independent sums.  The
// 15 columns then follow one by one, each continuing its sum over the block's earlier columns from registers and LDS, so every
// element's sum still ascends over k from zero.  The right-hand side rides along as row N of the matrix (thread N): its l_Nk IS y_k,
// by the same expression in the same order, so the forward substitution needs no pass of its own.
constexpr int SW_N = 15 * ORBVW_MAX_SOLVE_STATES, SW_T = 512, SW_B = 15;
static_assert(SW_N < SW_T, "a thread per row and one for the right-hand side");

__global__ __launch_bounds__(SW_T) void k_vw_solve(int N, double *__restrict__ S, const double *__restrict__ rhs, const double *__restrict__ b,
                                                   const double *__restrict__ lambda, double *__restrict__ dx, double *__restrict__ out,
                                                   int32_t *__restrict__ result)
{
    __shared__ double s_rows[SW_B][SW_N];      // rows B .. B + 14 of L, columns k < B; the backward substitution's x afterwards
    __shared__ double s_blk[SW_B][SW_B + 1];   // s_blk[c][k] = l_(B + c)(B + k): the block's own triangle
    __shared__ double s_y[SW_N];
    __shared__ double s_d;
    const int i = threadIdx.x;
    const bool row = i < N, rider = i == N;
    bool refused = false;
    double pivot = INFINITY, my_r = 0.0;
    for (int B = 0; B < N && !refused; B += SW_B) {
        const int nb = min(SW_B, N - B);
        for (int x = i; x < nb * B; x += SW_T) {
            const int c = x / B, k = x - c * B;
            s_rows[c][k] = S[(size_t)(B + c) * N + k];
        }
        __syncthreads();
        const bool act = (row && i >= B) || rider;
        double acc[SW_B], a[SW_B], l[SW_B];
#pragma unroll
        for (int c = 0; c < SW_B; ++c) acc[c] = 0.0, a[c] = 0.0, l[c] = 0.0;
        if (act) {
#pragma unroll
            for (int c = 0; c < SW_B; ++c)
                if (c < nb) a[c] = rider ? rhs[B + c] : S[(size_t)i * N + B + c];
            for (int k = 0; k < B; ++k) {
                const double lik = rider ? s_y[k] : S[(size_t)k * N + i];     // l_ik from the mirror: along row k
#pragma unroll
                for (int c = 0; c < SW_B; ++c) acc[c] = acc[c] + lik * s_rows[c][k];
            }
        }
#pragma unroll
        for (int c = 0; c < SW_B; ++c) {
            if (c >= nb || refused) continue;          // uniform
            const int j = B + c;
            double v = 0.0;
            if (act && i >= j) {
                double s = acc[c];
#pragma unroll
                for (int k = 0; k < c; ++k) s = s + l[k] * s_blk[c][k];
                v = a[c] - s;
                if (i == j) s_d = v;
            }
            __syncthreads();
            const double d = s_d;
            if (!(d > 0.0) || !isfinite(d)) {          // the same in every thread
                refused = true, pivot = d;
                continue;
            }
            pivot = d < pivot ? d : pivot;
            const double ljj = sqrt(d), r = 1.0 / ljj;
            if (i == j) S[(size_t)j * N + j] = ljj, my_r = r;
            else if (act && i > j) {
                const double lij = v * r;
                l[c] = lij;
                if (rider) s_y[j] = lij;
                else {
                    S[(size_t)i * N + j] = lij, S[(size_t)j * N + i] = lij;
                    if (i - B < SW_B) s_blk[i - B][c] = lij;
                }
            }
            __syncthreads();
        }
    }
    const double lam = *lambda;
    const double bi = row ? b[i] : 0.0;
    double x = 0.0;
    if (!refused) {
        double *s_x = s_rows[0];
        const double yi = row ? s_y[i] : 0.0;
        double s = 0.0;
        for (int k0 = N - 1; k0 >= 0; k0 -= SW_B) {        // backward: x_i = (y_i - sum_{k>i} l_ki*x_k)*r_i, k descending
            double lk[SW_B];
#pragma unroll
            for (int c = 0; c < SW_B; ++c) lk[c] = row && k0 - c > i ? S[(size_t)(k0 - c) * N + i] : 0.0;
#pragma unroll
            for (int c = 0; c < SW_B; ++c) {
                const int k = k0 - c;
                if (k < 0) continue;                       // uniform
                if (i == k) x = (yi - s) * my_r, s_x[k] = x;
                __syncthreads();
                if (row && i < k) s = s + lk[c] * s_x[k];
            }
        }
    }
    __syncthreads();
    if (row) dx[i] = x, s_y[i] = x * (lam * x + bi);
    __syncthreads();
    if (i == 0) {
        double s = 0.0;
        for (int k = 0; k < N; ++k) s = s + s_y[k];
        out[0] = refused ? 0.0 : s, out[2] = pivot;
    }
    if (i < 8) result[i] = i == ORBI_R_DONE ? !refused : i == ORBI_R_REFUSED ? refused : 0;
}

// ---- orbvw_backsub_device -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vw_backsub(int n_solve, int n_points, int cap_edges, const int32_t *__restrict__ off,
                                                    const int32_t *__restrict__ edge_state, const double *__restrict__ Hlp, const double *__restrict__ inv,
                                                    const double *__restrict__ bl, const double *__restrict__ dx, const double *__restrict__ points,
                                                    double *__restrict__ xl, double *__restrict__ points_out)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n_points) return;
    const double *m = inv + 9 * (size_t)l;
    double x[3] = {0.0, 0.0, 0.0};
    const bool skipped = point_skipped(m);
    if (!skipped) {
        const int lo = clampi(off[l], 0, cap_edges), hi = max(lo, clampi(off[l + 1], 0, cap_edges));
        double s[3] = {0.0, 0.0, 0.0};
        for (int e = lo; e < hi && hi - lo <= ORBVW_MAX_OBS; ++e) {
            const int st = edge_state[e];
            if (st < 0 || st >= n_solve) continue;
            const double *A = Hlp + 18 * (size_t)e, *q = dx + 15 * (size_t)st;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                double p = 0.0;
#pragma unroll
                for (int c = 0; c < 6; ++c) p = p + A[6 * r + c] * q[c];
                s[r] = s[r] + p;
            }
        }
        const double r0 = bl[3 * (size_t)l] - s[0], r1 = bl[3 * (size_t)l + 1] - s[1], r2 = bl[3 * (size_t)l + 2] - s[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) x[r] = dsum3(m[3 * r] * r0, m[3 * r + 1] * r1, m[3 * r + 2] * r2);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double p = points[3 * (size_t)l + r];
        xl[3 * (size_t)l + r] = x[r];
        points_out[3 * (size_t)l + r] = skipped ? p : p + x[r];
    }
}

// the points' share of computeScale and the counters: one workgroup
constexpr int BS_T = 1024, BS_WAVES = BS_T / 64;
__global__ __launch_bounds__(BS_T) void k_vw_scale(int n_points, const double *__restrict__ inv, const double *__restrict__ bl, const double *__restrict__ xl,
                                                   const double *__restrict__ lambda, double *__restrict__ out_points, int32_t *__restrict__ result)
{
    __shared__ double s_part[BS_WAVES][1];
    __shared__ int s_cnt[8];
    const int t = threadIdx.x;
    if (t < 8) s_cnt[t] = 0;
    __syncthreads();
    const double lam = *lambda;
    double acc[1] = {0.0};
    int n_done = 0, n_sing = 0;
    for (int l = t; l < n_points; l += BS_T) {
        if (point_skipped(inv + 9 * (size_t)l)) {
            ++n_sing;
            continue;
        }
        ++n_done;
        const double *x = xl + 3 * (size_t)l, *b = bl + 3 * (size_t)l;
        acc[0] = acc[0] + dsum3(x[0] * (lam * x[0] + b[0]), x[1] * (lam * x[1] + b[1]), x[2] * (lam * x[2] + b[2]));
    }
    block_sums_put(acc, s_part);
    block_add(s_cnt, {ORBI_R_DONE, ORBVW_R_POINT_SINGULAR}, {n_done, n_sing});
    __syncthreads();
    if (t == 0) out_points[0] = block_sums_get(s_part, 0);
    if (t < 8) result[t] = s_cnt[t];
}

inline unsigned blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }

} // namespace

extern "C" int orbvw_linearize_device(orbi_graph graph, orbi_calib calib, orbvi_camera camera, int n_solve, int n_points, int cap_edges, const double *d_points,
                                      const int32_t *d_edge_state, const int32_t *d_edge_point, const double *d_edge_z, const double *d_edge_inv_sigma2,
                                      const uint8_t *d_active, double huber_delta, double chi2_threshold, int mode, int32_t *d_point_off, double *d_work,
                                      double *d_err, double *d_chi2, double *d_total, double *d_H_diag, double *d_b, double *d_Hll, double *d_bl, double *d_Hlp,
                                      uint8_t *d_outlier, int32_t *d_result, void *stream)
{
    const char *own = nullptr;
    if (n_points < 1 || cap_edges < 0 || !d_points || !d_edge_state || !d_edge_point || !d_edge_z || !d_edge_inv_sigma2 || !d_point_off || !d_err || !d_chi2)
        own = "null point or edge array, d_point_off, d_err or d_chi2, n_points < 1 or a negative edge count";
    else if (n_solve < 1 || n_solve > graph.n_states) own = "n_solve outside [1, n_states]";
    if (int rc = graph_check_linearize(graph, d_result, own, mode, huber_delta, chi2_threshold, camera)) return rc;
    if (mode == 0 && (!d_work || !d_H_diag || !d_b || !d_Hll || !d_bl || !d_Hlp)) return orbx_set_error(ORBX_E_ARG, "mode 0 needs d_work, d_H_diag, d_b, d_Hll, d_bl and d_Hlp");
    if (mode != 2 && !d_total) return orbx_set_error(ORBX_E_ARG, "modes 0 and 1 need d_total");
    if (mode == 2 && !d_outlier) return orbx_set_error(ORBX_E_ARG, "mode 2 needs d_outlier");
    if (n_solve > ORBVW_MAX_SOLVE_STATES) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVW_MAX_SOLVE_STATES (32) solve states");
    if (cap_edges > ORBVW_MAX_EDGES || n_points > ORBVW_MAX_POINTS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVW_MAX_EDGES (2^20) edges or ORBVW_MAX_POINTS (2^18) points");
    if (graph.n_states > ORBI_MAX_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBI_MAX_JOBS (4096) states");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    VwArgs a = {};
    a.g = graph, a.cal = calib;
    a.cam = graph_camera(camera, huber_delta);
    a.n_solve = n_solve, a.n_points = n_points, a.n_edges = cap_edges, a.points = d_points, a.edge_state = d_edge_state, a.edge_point = d_edge_point;
    a.z = d_edge_z, a.w = d_edge_inv_sigma2, a.active = d_active, a.threshold = chi2_threshold, a.mode = mode, a.off = d_point_off, a.work = d_work;
    a.err = d_err, a.chi2 = d_chi2, a.total = d_total, a.H = d_H_diag, a.b = d_b, a.Hll = d_Hll, a.bl = d_bl, a.Hlp = d_Hlp, a.outlier = d_outlier, a.result = d_result;
    hipLaunchKernelGGL(k_vw_off_init, dim3(blocks(n_points + 1, 256)), dim3(256), 0, s, n_points + 1, cap_edges, d_point_off, d_result);
    if (cap_edges > 0) hipLaunchKernelGGL(k_vw_off_first, dim3(blocks(cap_edges, 256)), dim3(256), 0, s, cap_edges, n_points, d_edge_point, d_point_off);
    hipLaunchKernelGGL(k_vw_off_scan, dim3(1), dim3(1024), 0, s, n_points + 1, d_point_off);
    if (cap_edges > 0) hipLaunchKernelGGL(k_vw_edge, dim3(blocks(cap_edges, 256)), dim3(256), 0, s, a);
    if (mode == 0) hipLaunchKernelGGL(k_vw_point, dim3(blocks(n_points, 256)), dim3(256), 0, s, a);
    if (mode == 0) hipLaunchKernelGGL(k_vw_state, dim3(n_solve + 1), dim3(ST_T), 0, s, a, n_solve);
    if (mode == 1) hipLaunchKernelGGL(k_vw_state, dim3(1), dim3(ST_T), 0, s, a, 0);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbvw_reduce_device(int n_solve, const uint8_t *d_fixed, const orbi_edge *d_edges, int n_edges, int cap, const double *d_H_diag,
                                   const double *d_H_off, const double *d_b, const double *d_lambda, int n_points, int cap_edges, const int32_t *d_point_off,
                                   const int32_t *d_edge_state, const double *d_Hll, const double *d_bl, const double *d_Hlp, double *d_S, double *d_rhs,
                                   double *d_Hll_inv, double *d_tl, double *d_out, int32_t *d_result, void *stream)
{
    if (n_solve < 1 || !d_fixed || n_edges < 0 || cap < 1 || !d_H_diag || !d_b || !d_lambda || !d_result)
        return orbx_set_error(ORBX_E_ARG, "null array or result, n_solve or cap < 1, or a negative edge count");
    if (n_edges > 0 && (!d_edges || !d_H_off)) return orbx_set_error(ORBX_E_ARG, "edges without their list or d_H_off");
    if (n_points < 1 || cap_edges < 0 || !d_point_off || !d_edge_state || !d_Hll || !d_bl || !d_Hlp || !d_S || !d_rhs || !d_Hll_inv || !d_tl || !d_out)
        return orbx_set_error(ORBX_E_ARG, "null point or edge array or output, n_points < 1 or a negative edge count");
    if (n_solve > ORBVW_MAX_SOLVE_STATES) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVW_MAX_SOLVE_STATES (32) solve states");
    if (cap_edges > ORBVW_MAX_EDGES || n_points > ORBVW_MAX_POINTS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVW_MAX_EDGES (2^20) edges or ORBVW_MAX_POINTS (2^18) points");
    if (n_edges > ORBI_MAX_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBI_MAX_JOBS (4096) inertial edges in one call");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    RdArgs a = {n_solve, n_edges, cap, n_points, cap_edges, d_fixed, d_edges, d_H_diag, d_H_off, d_b, d_lambda, d_point_off, d_edge_state, d_Hll, d_bl, d_Hlp,
                d_S, d_rhs, d_Hll_inv, d_tl, d_out, d_result};
    const int N = 15 * n_solve;
    hipLaunchKernelGGL(k_vw_point_inv, dim3(blocks(n_points, 256)), dim3(256), 0, s, n_points, d_lambda, d_Hll, d_bl, d_Hll_inv, d_tl);
    hipLaunchKernelGGL(k_vw_base, dim3(blocks((long)N * N, 256) + 1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_vw_schur, dim3(n_solve * (n_solve + 1) / 2), dim3(SC_T), 0, s, a);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbvw_solve_device(int n_solve, double *d_S, const double *d_rhs, const double *d_b, const double *d_lambda, double *d_dx, double *d_out,
                                  int32_t *d_result, void *stream)
{
    if (n_solve < 1 || !d_S || !d_rhs || !d_b || !d_lambda || !d_dx || !d_out || !d_result) return orbx_set_error(ORBX_E_ARG, "null array or result, or n_solve < 1");
    if (n_solve > ORBVW_MAX_SOLVE_STATES) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVW_MAX_SOLVE_STATES (32) solve states");
    if (int rc = orb_need_device()) return rc;
    hipLaunchKernelGGL(k_vw_solve, dim3(1), dim3(SW_T), 0, (hipStream_t)stream, 15 * n_solve, d_S, d_rhs, d_b, d_lambda, d_dx, d_out, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbvw_backsub_device(int n_solve, int n_points, int cap_edges, const int32_t *d_point_off, const int32_t *d_edge_state, const double *d_Hlp,
                                    const double *d_Hll_inv, const double *d_bl, const double *d_dx, const double *d_lambda, const double *d_points,
                                    double *d_xl, double *d_points_out, double *d_out_points, int32_t *d_result, void *stream)
{
    if (n_solve < 1 || n_points < 1 || cap_edges < 0 || !d_point_off || !d_edge_state || !d_Hlp || !d_Hll_inv || !d_bl || !d_dx || !d_lambda || !d_points || !d_xl ||
        !d_points_out || !d_out_points || !d_result)
        return orbx_set_error(ORBX_E_ARG, "null array or result, n_solve or n_points < 1, or a negative edge count");
    if (d_points_out == d_points) return orbx_set_error(ORBX_E_ARG, "d_points_out must not be d_points: a trial leaves the estimate intact");
    if (n_solve > ORBVW_MAX_SOLVE_STATES) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVW_MAX_SOLVE_STATES (32) solve states");
    if (cap_edges > ORBVW_MAX_EDGES || n_points > ORBVW_MAX_POINTS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVW_MAX_EDGES (2^20) edges or ORBVW_MAX_POINTS (2^18) points");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_vw_backsub, dim3(blocks(n_points, 256)), dim3(256), 0, s, n_solve, n_points, cap_edges, d_point_off, d_edge_state, d_Hlp, d_Hll_inv, d_bl,
                       d_dx, d_points, d_xl, d_points_out);
    hipLaunchKernelGGL(k_vw_scale, dim3(1), dim3(BS_T), 0, s, n_points, d_Hll_inv, d_bl, d_xl, d_lambda, d_out_points, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

// =====================================================================================================================
// The window loop (include/orbwl.h): localFullBundleAdjustment's Levenberg-Marquardt loop closed by the host over the staged entry
// points above and orbi.h's, which it CALLS -- no stage kernel is launched or restated here.  The host driver lives in this file
// because this is the one source that includes orbvw.h; what runs on the device between the stage calls (the policy, push and pop,
// the trace, the counters) is orbwl.hip's, reached through orbwl_kernels.h.  It waits on the caller's stream once per trial, for one
// 16-byte verdict in page-locked memory, and once at the end.
// =====================================================================================================================
#include "orbwl_kernels.h"

static_assert(ORBWL_R_OUTLIER == ORBVW_R_OUTLIER && ORBWL_R_POINT_SINGULAR == ORBVW_R_POINT_SINGULAR && ORBWL_R_REJECTED == ORBI_R_DUPLICATE,
              "orbwl.h restates these slots of a d_result");

namespace {

// the caller's scratch carved into the intermediates of the chain, in doubles; every slice starts on an even double
enum { WLR_LIN_I, WLR_LIN_V, WLR_REDUCE, WLR_SOLVE, WLR_BACKSUB, WLR_OPLUS, WLR_TRY_I, WLR_TRY_V, WLR_CLASSIFY, WLR_SLOTS };
struct WlPlan {
    int64_t n = 0;
    int64_t H_diag, H_off, b, iwork, ierr, ichi2, ichi2_prior, itotal, vwork, verr, vtotal, Hll, bl, Hlp, point_off, S, rhs, Hll_inv, tl, dx, xl, points2,
        out, out_points, lambda, saved, saved_iter, ctrl, results;
    int64_t add(int64_t doubles) { const int64_t o = n; n += (doubles + 1) & ~(int64_t)1; return o; }
    WlPlan(int64_t S_, int64_t ns, int64_t L, int64_t E, int64_t J, int64_t P)
    {
        const int64_t N = 15 * ns;
        H_diag = add(225 * S_), H_off = add(225 * J), b = add(15 * S_);
        iwork = add(ORBI_EDGE_WORK * J), ierr = add(9 * J), ichi2 = add(3 * J), ichi2_prior = add(3 * P), itotal = add(4);
        vwork = add(ORBVW_EDGE_WORK * E), verr = add(2 * E), vtotal = add(4), Hll = add(9 * L), bl = add(3 * L), Hlp = add(18 * E), point_off = add((L + 1 + 1) / 2);
        S = add(N * N), rhs = add(N), Hll_inv = add(9 * L), tl = add(3 * L), dx = add(N), xl = add(3 * L);
        points2 = add(3 * L);
        out = add(3), out_points = add(1), lambda = add(1);
        saved = add(21 * ns), saved_iter = add((ns + 1) / 2);
        ctrl = add(WL_CTRL_DOUBLES);
        results = add(8 * WLR_SLOTS / 2);
    }
};

// a page-locked block for the verdict, leased for a call and pooled per device: nothing is allocated per call
struct WlWork {
    int device = 0;
    hipStream_t stream = nullptr;          // none of its own: the call runs on the caller's stream
    PinBuf h;
    hipError_t init() { return h.need(64, 64); }
};
LeasePool<WlWork> g_wl_work; // per process, keyed by device; never freed: the HIP runtime may be gone when static destructors run

inline bool wl_number(double x) { return x == x; }

} // namespace

extern "C" int64_t orbwl_window_work_doubles(int n_states, int n_solve, int n_points, int cap_edges, int n_edges, int n_prior_jobs)
{
    if (n_states < 1 || n_solve < 1 || n_solve > n_states || n_points < 1 || cap_edges < 0 || n_edges < 0 || n_prior_jobs < 0) return -1;
    return WlPlan(n_states, n_solve, n_points, cap_edges, n_edges, n_prior_jobs).n;
}

extern "C" int orbwl_window_optimize_device(orbi_graph graph, int32_t *d_iter, const orbi_record *d_bank, int cap, const orbi_edge *d_edges, int n_edges,
                                            const double *d_info, const double *d_walk_info, const orbi_prior *d_priors, int n_priors,
                                            const orbi_prior_job *d_prior_jobs, int n_prior_jobs, orbi_calib calib, orbvi_camera camera, int n_solve,
                                            int n_points, int cap_edges, double *d_points, const int32_t *d_edge_state, const int32_t *d_edge_point,
                                            const double *d_edge_z, const double *d_edge_inv_sigma2, const uint8_t *d_active, orbwl_loop_options options,
                                            double *d_work, double *d_chi2, uint8_t *d_outlier, double *d_trace, int cap_trace, double *d_summary,
                                            int32_t *d_result, const volatile int32_t *stop, void *stream)
{
    const orbwl_loop_options &o = options;
    if (!graph.Rwb || !graph.twb || !graph.v || !graph.bg || !graph.ba || !graph.fixed || graph.n_states < 0 || !d_result)
        return orbx_set_error(ORBX_E_ARG, "null graph array or result, or a negative state count");
    if (!d_iter || !d_bank || cap < 1 || !d_edges || n_edges < 0 || !d_info || !d_walk_info)
        return orbx_set_error(ORBX_E_ARG, "null d_iter, bank, inertial edge list or information, cap < 1, or a negative inertial edge count");
    if (n_prior_jobs < 0 || n_priors < 0 || (n_prior_jobs > 0 && (!d_prior_jobs || !d_priors)))
        return orbx_set_error(ORBX_E_ARG, "prior jobs without their list or the priors, or a negative count");
    if (n_points < 1 || cap_edges < 0 || !d_points || !d_edge_state || !d_edge_point || !d_edge_z || !d_edge_inv_sigma2)
        return orbx_set_error(ORBX_E_ARG, "null point or EdgeMono array, n_points < 1 or a negative cap_edges");
    if (n_solve < 1 || n_solve > graph.n_states) return orbx_set_error(ORBX_E_ARG, "n_solve outside [1, n_states]");
    if (!d_work || ((uintptr_t)d_work & 15)) return orbx_set_error(ORBX_E_ARG, "d_work is null or not 16-byte aligned");
    if (!d_chi2 || !d_outlier || !d_summary || cap_trace < 0 || (cap_trace > 0 && !d_trace))
        return orbx_set_error(ORBX_E_ARG, "null d_chi2, d_outlier, summary or trace, or a negative cap_trace");
    if (o.iterations < 1 || o.max_trials < 1) return orbx_set_error(ORBX_E_ARG, "iterations or max_trials < 1");
    if (!wl_number(o.lambda_init) || !wl_number(o.huber_delta_visual) || !wl_number(o.huber_delta_inertial) || !wl_number(o.chi2_threshold) || !wl_number(o.gravity))
        return orbx_set_error(ORBX_E_ARG, "lambda_init, a huber_delta, chi2_threshold or gravity is not a number");
    if (camera.camera_model != 0 && camera.camera_model != 1) return orbx_set_error(ORBX_E_ARG, "camera_model is 0 (Pinhole) or 1 (Kannala-Brandt)");
    if (n_solve > ORBVW_MAX_SOLVE_STATES) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVW_MAX_SOLVE_STATES (32) solve states");
    if (cap_edges > ORBVW_MAX_EDGES || n_points > ORBVW_MAX_POINTS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVW_MAX_EDGES (2^20) edges or ORBVW_MAX_POINTS (2^18) points");
    if (graph.n_states > ORBI_MAX_JOBS || n_edges > ORBI_MAX_JOBS || n_prior_jobs > ORBI_MAX_JOBS)
        return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBI_MAX_JOBS (4096) states, inertial edges or prior jobs");
    if (o.iterations > ORBWL_MAX_ITERATIONS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBWL_MAX_ITERATIONS (100) iterations");
    if (o.max_trials > ORBWL_MAX_TRIALS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBWL_MAX_TRIALS (10) trials in an iteration");
    if (o.lambda_init == 0) return orbx_set_error(ORBX_E_UNSUPPORTED, "lambda_init == 0 (computeLambdaInit): this optimiser always sets a user value");
    int device = -1;
    if (int rc = orb_need_device(&device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    Lease<WlWork> lease(g_wl_work);
    ORB_TRY(lease.acquire(device));
    lease.stream = s;                      // the call runs on the caller's stream: that one is waited on before the block goes back
    volatile int32_t *const verdict = lease.w->h.as<int32_t>();
    int32_t *d_verdict = nullptr;
    ORB_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&d_verdict), lease.w->h.p, 0));

    const WlPlan q(graph.n_states, n_solve, n_points, cap_edges, n_edges, n_prior_jobs);
    double *const w = d_work;
    int32_t *const slots = reinterpret_cast<int32_t *>(w + q.results);
    auto slot = [&](int k) { return slots + 8 * k; };
    int32_t *const point_off = reinterpret_cast<int32_t *>(w + q.point_off);
    int32_t *const saved_iter = reinterpret_cast<int32_t *>(w + q.saved_iter);
    double *pts[2] = {d_points, w + q.points2};
    orbi_graph solve_states = graph;       // the update reaches the states [0, n_solve) only
    solve_states.n_states = n_solve;

    // both linearisations at the estimate (mode 0) or their errors at the trial point (mode 1, on `points`)
    auto evaluate = [&](int mode, const double *points) -> int {
        double *const ti = w + q.itotal + 2 * mode, *const tv = w + q.vtotal + 2 * mode;
        if (int rc = orbi_linearize_device(graph, d_bank, cap, o.gravity, d_edges, n_edges, d_info, d_walk_info, d_priors, n_priors, d_prior_jobs, n_prior_jobs,
                                           o.huber_delta_inertial, mode, w + q.iwork, w + q.ierr, w + q.ichi2, w + q.ichi2_prior, ti, mode ? nullptr : w + q.H_diag,
                                           mode ? nullptr : w + q.H_off, mode ? nullptr : w + q.b, nullptr, nullptr, slot(mode ? WLR_TRY_I : WLR_LIN_I), stream))
            return rc;
        return orbvw_linearize_device(graph, calib, camera, n_solve, n_points, cap_edges, points, d_edge_state, d_edge_point, d_edge_z, d_edge_inv_sigma2, d_active,
                                      o.huber_delta_visual, o.chi2_threshold, mode, point_off, mode ? nullptr : w + q.vwork, w + q.verr, d_chi2, tv,
                                      mode ? nullptr : w + q.H_diag, mode ? nullptr : w + q.b, mode ? nullptr : w + q.Hll, mode ? nullptr : w + q.bl,
                                      mode ? nullptr : w + q.Hlp, nullptr, slot(mode ? WLR_TRY_V : WLR_LIN_V), stream);
    };
    auto raised = [&]() { return stop && *stop != 0; };

    ORB_TRY(wl_launch_begin(w + q.ctrl, d_summary, w + q.lambda, o.lambda_init > 0 ? o.lambda_init : 0.0, s));
    WlDecide dc = {};
    dc.g = solve_states, dc.iter = d_iter, dc.n_solve = n_solve;
    dc.lin_inertial = w + q.itotal, dc.lin_visual = w + q.vtotal, dc.try_inertial = w + q.itotal + 2, dc.try_visual = w + q.vtotal + 2;
    dc.out = w + q.out, dc.out_points = w + q.out_points, dc.solve_result = slot(WLR_SOLVE), dc.lambda = w + q.lambda, dc.ctrl = w + q.ctrl;
    dc.saved = w + q.saved, dc.saved_iter = saved_iter, dc.trace = d_trace, dc.cap_trace = cap_trace, dc.max_trials = o.max_trials, dc.iterations = o.iterations;
    dc.verdict = d_verdict;
    int live = 0, stopped = 0, next = WL_NEXT_ITERATION;
    for (int it = 0; it < o.iterations && next == WL_NEXT_ITERATION; ++it) {
        if (raised()) { stopped = 1; break; }
        if (int rc = evaluate(0, pts[live])) return rc;
        next = WL_NEXT_TRIAL;
        for (int trial = 0; trial < o.max_trials && next == WL_NEXT_TRIAL; ++trial) {
            if (trial > 0 && raised()) { stopped = 1; break; }
            if (int rc = orbvw_reduce_device(n_solve, graph.fixed, d_edges, n_edges, cap, w + q.H_diag, w + q.H_off, w + q.b, w + q.lambda, n_points, cap_edges, point_off,
                                             d_edge_state, w + q.Hll, w + q.bl, w + q.Hlp, w + q.S, w + q.rhs, w + q.Hll_inv, w + q.tl, w + q.out, slot(WLR_REDUCE), stream))
                return rc;
            if (int rc = orbvw_solve_device(n_solve, w + q.S, w + q.rhs, w + q.b, w + q.lambda, w + q.dx, w + q.out, slot(WLR_SOLVE), stream)) return rc;
            if (int rc = orbvw_backsub_device(n_solve, n_points, cap_edges, point_off, d_edge_state, w + q.Hlp, w + q.Hll_inv, w + q.bl, w + q.dx, w + q.lambda, pts[live],
                                              w + q.xl, pts[1 - live], w + q.out_points, slot(WLR_BACKSUB), stream))
                return rc;
            if (trial == 0) ORB_TRY(wl_launch_push(solve_states, d_iter, n_solve, w + q.saved, saved_iter, s));   // a popped estimate is the pushed one
            if (int rc = orbi_graph_oplus_device(solve_states, w + q.dx, d_iter, slot(WLR_OPLUS), stream)) return rc;
            if (int rc = evaluate(1, pts[1 - live])) return rc;
            dc.first = trial == 0;
            verdict[WLV_NEXT] = -1;
            ORB_TRY(wl_launch_decide(dc, s));
            ORB_TRY(hipStreamSynchronize(s));                      // the wait of a trial: the verdict is in host memory
            next = verdict[WLV_NEXT];
            if (next != WL_NEXT_TRIAL && next != WL_NEXT_ITERATION && next != WL_NEXT_END)
                return orbx_set_error(ORBX_E_NO_DEVICE, "the trial's verdict did not reach the page-locked block");
            if (verdict[WLV_ACCEPTED]) live = 1 - live;            // the updated points are the estimate
        }
        if (stopped) break;
    }
    if (live != 0) ORB_TRY(hipMemcpyAsync(d_points, pts[1], 24 * (size_t)n_points, hipMemcpyDeviceToDevice, s));
    // step 5 of the reference at the final estimate, whatever ended the loop
    if (int rc = orbvw_linearize_device(graph, calib, camera, n_solve, n_points, cap_edges, d_points, d_edge_state, d_edge_point, d_edge_z, d_edge_inv_sigma2, nullptr,
                                        o.huber_delta_visual, o.chi2_threshold, 2, point_off, nullptr, w + q.verr, d_chi2, nullptr, nullptr, nullptr, nullptr, nullptr,
                                        nullptr, d_outlier, slot(WLR_CLASSIFY), stream))
        return rc;
    const WlEnd e = {w + q.lambda, w + q.ctrl, slot(WLR_CLASSIFY), slot(WLR_TRY_I), slot(WLR_REDUCE), cap_trace, stopped, d_summary, d_result};
    ORB_TRY(wl_launch_end(e, s));
    ORB_TRY(hipStreamSynchronize(s));      // the wait at the end: the page-locked block goes back to the pool
    return ORBX_OK;
}
