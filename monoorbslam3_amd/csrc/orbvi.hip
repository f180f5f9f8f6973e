// The visual edges of the inertial optimisers and their damped step on the device (include/orbvi.h):
//   orbvi_linearize_device   EdgeMonoOnlyPose on a VertexPose: computeError, linearizeOplus, constructQuadraticForm   G2oTypes.cpp:49-57, G2oTypes.h:41-54
//                            and the inlier classification of poseFullOptimize                                      Optimize.cpp:722-735
//   orbvi_solve_device       (H + lambda*I)*dx = b of g2o's BlockSolverX with nothing marginalised                  Optimize.cpp:613-615
//
// Everything is IEEE double in the header's orders without fused multiply-add; the camera is csrc/orbba_camera.h, the one orbba.hip
// evaluates; the edge's pose path, quadratic form and host checks are csrc/orbi_graph_device.h's.
//
// Shape: both calls are latency-bound.  A group of edges (the tracker has one, of a few hundred to 2000) is ONE 1024-thread workgroup,
// like k_project and k_triangulate: a thread takes the edges t, t + 1024, ... and keeps its 21 + 6 + 2 partial sums in registers; a
// wave butterfly and sixteen LDS slots summed in wave order finish them, so no floating-point atomic is needed and the same input
// gives the same bytes.  The pose the edges hang on is derived once per workgroup into LDS.  The solve assembles its at most 60 x 60
// matrix in LDS with the whole workgroup and factorises it with ONE WAVE, a lane per row: the pivot and the substitutions' unknowns
// travel by cross-lane reads, the phases are separated by wave-level fences only.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "../../include/orbvi.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orb_math.h"
#include "orbba_camera.h"
#include "orbi_graph_device.h"

#pragma clang fp contract(off)

static_assert(sizeof(orbvi_camera) == 72, "orbvi.h fixes this layout");

namespace {

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

__global__ __launch_bounds__(VI_T) void k_vi_linearize(const ViArgs a)
{
    __shared__ double s_part[VI_WAVES][VI_SUMS];
    __shared__ double s_pose[P_WORDS];
    __shared__ int s_cnt[8];
    __shared__ int s_i[I_WORDS];
    const int t = threadIdx.x, lane = t & 63, g = blockIdx.x;
    if (t < 8) s_cnt[t] = 0;
    if (t < I_WORDS) s_i[t] = 0;
    __syncthreads();
    // the group's range: d_edge_off clamped and made non-decreasing; its state against the earlier groups'
    const int st = a.group_state[g];
    {
        int lo = 0, dup = 0;
        for (int k = t; k <= g; k += VI_T) {
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
        for (int e = lo + t; e < hi; e += VI_T) a.err[2 * (size_t)e] = 0.0, a.err[2 * (size_t)e + 1] = 0.0, a.chi2[e] = 0.0;
        if (t < 2 && a.mode != 2) a.total[2 * (size_t)g + t] = 0.0;
        if (t == 0 && a.mode == 2) a.n_inliers[g] = 0;
        __syncthreads();
        if (t < 8) {
            if (gridDim.x == 1) a.result[t] = s_cnt[t];
            else if (s_cnt[t]) atomicAdd(&a.result[t], s_cnt[t]);
        }
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
    const bool accumulate = a.mode == 0 && !(a.g.fixed[st] & ORBI_FIX_POSE);
    double plain = 0.0, robust = 0.0;
    int n_bad = 0, n_in = 0;
    for (int e = lo + t; e < hi; e += VI_T) {
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
        if (a.mode == 2) {
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
    for (int e = lo + t; accumulate && e < hi; e += VI_T) {
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
        for (int e = lo + t; e < hi; e += VI_T) {
            const double *work = a.work + (size_t)ORBVI_EDGE_WORK * e;
            if (work[W_USED] == 0.0) continue;
            quad_accumulate(work + W_J, work[W_W], work[W_WE], work[W_WE + 1], acc);
        }
    }
    block_sums_put(acc, s_part, accumulate ? 0 : S_PLAIN);
    block_add(s_cnt, ORBVI_R_NONFINITE, n_bad);
    block_add(s_i, I_INLIERS, n_in);
    __syncthreads();
    if (t < VI_SUMS && a.mode != 2 && (t >= S_PLAIN || accumulate)) {
        const double s = block_sums_get(s_part, t);
        if (t >= S_PLAIN) a.total[2 * (size_t)g + t - S_PLAIN] = s;
        else quad_scatter(t, s, a.H + 225 * (size_t)st, a.b + 15 * (size_t)st);
    }
    if (t == 0 && a.mode == 2) a.n_inliers[g] = s_i[I_INLIERS];
    if (t < 8) {
        if (gridDim.x == 1) a.result[t] = s_cnt[t];
        else if (s_cnt[t]) atomicAdd(&a.result[t], s_cnt[t]);
    }
}

// ---- orbvi_solve_device: one workgroup assembles, one wave factorises ------------------------------------------------------------------
constexpr int SV_N = 15 * ORBVI_MAX_STATES, SV_LD = SV_N + 1, SV_T = 256;   // a row stride of 61 doubles spreads a column over the banks

__global__ __launch_bounds__(SV_T) void k_vi_solve(int n, const uint8_t *__restrict__ fixed, const orbi_edge *__restrict__ edges, int n_edges, int cap,
                                                   const double *__restrict__ H_diag, const double *__restrict__ H_off, const double *__restrict__ b,
                                                   const double *__restrict__ lambda, double *__restrict__ dx, double *__restrict__ out,
                                                   int32_t *__restrict__ result)
{
    __shared__ double s_A[SV_N * SV_LD];
    __shared__ double s_v[SV_N];
    __shared__ int s_fix[SV_N];
    __shared__ int s_cnt[8];
    const int t = threadIdx.x, N = 15 * n;
    for (int x = t; x < SV_N * SV_LD; x += SV_T) s_A[x] = 0.0;
    if (t < 8) s_cnt[t] = 0;
    if (t < N) s_fix[t] = dof_fixed(fixed[t / 15], t % 15);
    __syncthreads();
    for (int x = t; x < 225 * n; x += SV_T) {
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
    for (int x = t; x < N * N; x += SV_T) {       // a fixed dof is an identity row and column
        const int r = x / N, c = x - N * r;
        if (s_fix[r] || s_fix[c]) s_A[r * SV_LD + c] = r == c ? 1.0 : 0.0;
    }
    __syncthreads();
    if (t >= 64) return;                          // one wave from here on, a lane per row: no workgroup barrier below
    const int i = t;
    const bool in = i < N, fre = in && !s_fix[in ? i : 0];
    const double lam = *lambda;
    const double hjj = in ? s_A[i * SV_LD + i] : 0.0;
    const double h_max = wave_max(fre && hjj > 0.0 ? hjj : 0.0);
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
        out[0] = refused ? 0.0 : s, out[1] = h_max, out[2] = pivot;
    }
    if (i < 8) result[i] = i == ORBI_R_DONE ? !refused : i == ORBI_R_REFUSED ? refused : i == ORBI_R_RANGE ? s_cnt[ORBI_R_RANGE] : 0;
}

} // namespace

extern "C" int orbvi_linearize_device(orbi_graph graph, orbi_calib calib, orbvi_camera camera, int n_groups, int cap_edges, const int32_t *d_group_state,
                                      const int32_t *d_edge_off, const double *d_points, const double *d_edge_z, const double *d_edge_inv_sigma2,
                                      uint8_t *d_active, double huber_delta, double chi2_threshold, int mode, double *d_work, double *d_err,
                                      double *d_chi2, double *d_total, double *d_H_diag, double *d_b, int32_t *d_n_inliers, int32_t *d_result, void *stream)
{
    const char *own = nullptr;
    if (n_groups < 0 || cap_edges < 0 || !d_group_state || !d_edge_off || !d_points || !d_edge_z || !d_edge_inv_sigma2 || !d_err || !d_chi2)
        own = "null group list, edge array, d_err or d_chi2, or a negative count";
    if (int rc = graph_check_linearize(graph, d_result, own, mode, huber_delta, chi2_threshold, camera)) return rc;
    if (mode == 0 && (!d_work || !d_H_diag || !d_b)) return orbx_set_error(ORBX_E_ARG, "mode 0 needs d_work, d_H_diag and d_b");
    if (mode != 2 && !d_total) return orbx_set_error(ORBX_E_ARG, "modes 0 and 1 need d_total");
    if (mode == 2 && (!d_active || !d_n_inliers)) return orbx_set_error(ORBX_E_ARG, "mode 2 needs d_active and d_n_inliers");
    if (graph.n_states > ORBI_MAX_JOBS || n_groups > ORBI_MAX_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBI_MAX_JOBS (4096) states or groups");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    ViArgs a = {};
    a.g = graph, a.cal = calib;
    a.cam = graph_camera(camera, huber_delta);
    a.n_groups = n_groups, a.cap_edges = cap_edges, a.group_state = d_group_state, a.edge_off = d_edge_off, a.points = d_points, a.z = d_edge_z;
    a.w = d_edge_inv_sigma2, a.active = d_active, a.threshold = chi2_threshold, a.mode = mode, a.work = d_work, a.err = d_err, a.chi2 = d_chi2, a.total = d_total;
    a.H = d_H_diag, a.b = d_b, a.n_inliers = d_n_inliers, a.result = d_result;
    LAUNCH_COUNTED(k_vi_linearize, n_groups, VI_T, s, d_result, a);
    return ORBX_OK;
}

extern "C" int orbvi_solve_device(int n_states, const uint8_t *d_fixed, const orbi_edge *d_edges, int n_edges, int cap, const double *d_H_diag,
                                  const double *d_H_off, const double *d_b, const double *d_lambda, double *d_dx, double *d_out, int32_t *d_result,
                                  void *stream)
{
    if (n_states < 1 || !d_fixed || n_edges < 0 || cap < 1 || !d_H_diag || !d_b || !d_lambda || !d_dx || !d_out || !d_result)
        return orbx_set_error(ORBX_E_ARG, "null array or result, n_states or cap < 1, or a negative edge count");
    if (n_edges > 0 && (!d_edges || !d_H_off)) return orbx_set_error(ORBX_E_ARG, "edges without their list or d_H_off");
    if (n_states > ORBVI_MAX_STATES) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBVI_MAX_STATES (4) states: a local window needs the Schur complement");
    if (n_edges > ORBI_MAX_JOBS) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBI_MAX_JOBS (4096) edges in one call");
    if (int rc = orb_need_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_vi_solve, dim3(1), dim3(SV_T), 0, s, n_states, d_fixed, d_edges, n_edges, cap, d_H_diag, d_H_off, d_b, d_lambda, d_dx, d_out, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
