// Optional second kernel set: per-edge reprojection residual + analytic Jacobians and the block J^T W J
// reduction of local bundle adjustment, in double precision (see include/orbba.h for the reference
// lines replaced).  Two kernels:
//   k_ba_edges        thread = edge: residual, chi2, Huber weight, J_point (2x3), J_pose (2x6); writes H_lp
//                     (3x6) and the edge's contribution to its pose block (21 upper-triangular + 6) and to
//                     its point block (6 + 3) into edge-major scratch;
//   k_ba_reduce_pose  workgroup = pose: sums its edges' contributions in a fixed order (CSR built on the
//                     host), wave shuffles + LDS, so results are reproducible run to run;
//   k_ba_reduce_point thread = point: sums its (contiguous) edges.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbba.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orb_lm_policy.h"
#include "orbba_camera.h"
#include "orbba_problem.h"

// kernel-choice switches of the BA entry points (include/orbba.h: orbba_set_variant); the entry points take no handle, so the
// switches are per process and read per call
static std::atomic<int> g_ba_chol{0};        // ORBBA_VAR_CHOL: 0 = reduced system in LDS when it fits, 1 = global-memory kernel
static std::atomic<int> g_ba_pose_lds{3000}; // ORBBA_VAR_POSE_LDS: edges of a frame k_pose_optimize stages in LDS (0 .. 3000)
extern "C" int orbba_set_variant(int which, int value)
{
    if (which == ORBBA_VAR_CHOL && (value == 0 || value == 1)) { g_ba_chol.store(value); return ORBX_OK; }
    if (which == ORBBA_VAR_POSE_LDS && value >= 0 && value <= 3000) { g_ba_pose_lds.store(value); return ORBX_OK; }
    return orbx_set_error(ORBX_E_ARG, "unknown BA variant switch or value out of range");
}

template <typename Problem> static BaCam make_cam(const Problem *p) // orbba_problem and orbba_pose_problem name the camera alike
{
    return {p->fx, p->fy, p->cx, p->cy, p->huber_delta, p->camera_model, {p->fisheye_k[0], p->fisheye_k[1], p->fisheye_k[2], p->fisheye_k[3]}};
}

__global__ __launch_bounds__(256) void k_ba_edges(BaCam cam, int n_edges, const double *__restrict__ pose_R,
                                                  const double *__restrict__ pose_t, const uint8_t *__restrict__ pose_fixed,
                                                  const double *__restrict__ points, const int *__restrict__ edge_pose,
                                                  const int *__restrict__ edge_point, const double *__restrict__ edge_z,
                                                  const double *__restrict__ edge_w,
                                                  const uint8_t *__restrict__ edge_active, double *__restrict__ chi2_out,
                                                  double *__restrict__ err_out, double *__restrict__ Hlp,
                                                  double *__restrict__ Cpp /* n_edges x 27 */,
                                                  double *__restrict__ Cll /* n_edges x 9 */)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_edges) return;
    const int ip = edge_pose[e], il = edge_point[e];
    double R[9], t[3], P[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = pose_R[9 * ip + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { t[i] = pose_t[3 * ip + i]; P[i] = points[3 * il + i]; }
    // Pc = Tcw.map(Pw)  (G2oTypes.cpp:41)
    const double X = R[0] * P[0] + R[1] * P[1] + R[2] * P[2] + t[0];
    const double Y = R[3] * P[0] + R[4] * P[1] + R[5] * P[2] + t[1];
    const double Z = R[6] * P[0] + R[7] * P[1] + R[8] * P[2] + t[2];
    // camera->project and the residual (G2oTypes.h:250)
    double u, v;
    ba_project(cam, X, Y, Z, &u, &v);
    const double ex = edge_z[2 * e] - u, ey = edge_z[2 * e + 1] - v;
    const double om = edge_w[e];
    const double chi2 = om * (ex * ex + ey * ey);
    // g2o RobustKernelHuber: rho'(chi2) = 1 inside delta^2, delta / sqrt(chi2) outside
    double rw = 1.0;
    if (cam.delta > 0.0 && chi2 > cam.delta * cam.delta) rw = cam.delta / sqrt(chi2);
    // an edge at level 1 (Optimize.cpp:900-902) is not part of the active set: its chi2 is still reported
    const double W = (edge_active && !edge_active[e]) ? 0.0 : rw * om;
    // camera->getProjJacobian (G2oTypes.cpp:42)
    double Jp[6];
    ba_proj_jacobian(cam, X, Y, Z, Jp);
    // J_point = -Jp * R  (G2oTypes.cpp:44)
    double Jl[6];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            Jl[3 * r + c] = -(Jp[3 * r] * R[c] + Jp[3 * r + 1] * R[3 + c] + Jp[3 * r + 2] * R[6 + c]);
    // J_pose = [Jp * Hat(Pc), -Jp]  (G2oTypes.cpp:45-46); Hat(Pc) = [0 -Z Y; Z 0 -X; -Y X 0]
    double Jq[12];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const double a = Jp[3 * r], b = Jp[3 * r + 1], c = Jp[3 * r + 2];
        Jq[6 * r + 0] = b * Z - c * Y;
        Jq[6 * r + 1] = -a * Z + c * X;
        Jq[6 * r + 2] = a * Y - b * X;
        Jq[6 * r + 3] = -a; Jq[6 * r + 4] = -b; Jq[6 * r + 5] = -c;
    }
    if (chi2_out) chi2_out[e] = chi2;
    if (err_out) { err_out[2 * e] = ex; err_out[2 * e + 1] = ey; }
    const bool fixed = pose_fixed[ip] != 0;
    // point block: H_ll += Jl^T W Jl (6 unique), b_l -= Jl^T W e
    if (!Cll || !Cpp) return; // error-only evaluation (an LM trial): the linearisation of the iteration is kept
    double *cl = Cll + (size_t)e * 9;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) cl[k++] = W * (Jl[i] * Jl[j] + Jl[3 + i] * Jl[3 + j]);
#pragma unroll
    for (int i = 0; i < 3; ++i) cl[6 + i] = -W * (Jl[i] * ex + Jl[3 + i] * ey);
    // pose block (21 unique + 6) and the off-diagonal block H_lp = Jl^T W Jq (3x6)
    double *cp = Cpp + (size_t)e * 27;
    k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) cp[k++] = fixed ? 0.0 : W * (Jq[i] * Jq[j] + Jq[6 + i] * Jq[6 + j]);
#pragma unroll
    for (int i = 0; i < 6; ++i) cp[21 + i] = fixed ? 0.0 : -W * (Jq[i] * ex + Jq[6 + i] * ey);
    if (Hlp) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j)
                Hlp[(size_t)e * 18 + 6 * i + j] = fixed ? 0.0 : W * (Jl[i] * Jq[j] + Jl[3 + i] * Jq[6 + j]);
    }
}

__global__ __launch_bounds__(256) void k_ba_reduce_pose(const int *__restrict__ pose_off, const int *__restrict__ pose_edges,
                                                        const double *__restrict__ Cpp, double *__restrict__ Hpp,
                                                        double *__restrict__ bp)
{
    __shared__ double red[4][27];
    const int ip = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    for (int i = pose_off[ip] + tid; i < pose_off[ip + 1]; i += 256) {
        const double *c = Cpp + (size_t)pose_edges[i] * 27;
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[k] += c[k];
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wv][k] = v;
    }
    __syncthreads();
    if (tid < 27) {
        const double v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        if (tid < 21) {
            int i = 0, k = tid; // unpack the upper-triangular index
            while (k >= 6 - i) { k -= 6 - i; ++i; }
            const int j = i + k;
            if (Hpp) { Hpp[(size_t)ip * 36 + 6 * i + j] = v; Hpp[(size_t)ip * 36 + 6 * j + i] = v; }
        } else if (bp) bp[(size_t)ip * 6 + tid - 21] = v;
    }
}

__global__ __launch_bounds__(256) void k_ba_reduce_point(int n_points, const int *__restrict__ point_off,
                                                         const double *__restrict__ Cll, double *__restrict__ Hll,
                                                         double *__restrict__ bl)
{
    const int il = blockIdx.x * blockDim.x + threadIdx.x;
    if (il >= n_points) return;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    for (int e = point_off[il]; e < point_off[il + 1]; ++e)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] += Cll[(size_t)e * 9 + k];
    if (Hll) {
        double *h = Hll + (size_t)il * 9;
        h[0] = acc[0]; h[1] = acc[1]; h[2] = acc[2];
        h[3] = acc[1]; h[4] = acc[3]; h[5] = acc[4];
        h[6] = acc[2]; h[7] = acc[4]; h[8] = acc[5];
    }
    if (bl) { bl[(size_t)il * 3] = acc[6]; bl[(size_t)il * 3 + 1] = acc[7]; bl[(size_t)il * 3 + 2] = acc[8]; }
}

namespace {
// The device side of one host-pointer call.  The BA entry points take no handle and run on two of the reference's threads
// (poseOptimize on Tracking, Tracking.cpp:273-358; localBundleAdjustment on LocalMapping, LocalMapping.cpp:45-52), so a call
// leases a workspace for its duration: a NON-BLOCKING stream, one device arena, one page-locked staging block and two events,
// pooled per device.  Concurrent calls never share a stream or scratch, none of them touches stream 0 (include/orbx.h,
// "Streams": a legacy-stream operation is a barrier against every blocking stream of every thread), and a steady-state call
// allocates nothing (hipMalloc / hipFree wait for the whole device).  Inputs go up in ONE copy from the staging block, results
// come back in one, and the LM loop reads one small block per trial.
struct BaWork {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DevBuf d;
    PinBuf h;
    hipError_t init()
    {
        hipError_t e;
        if ((e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)) != hipSuccess || (e = hipEventCreate(&e0)) != hipSuccess ||
            (e = hipEventCreate(&e1)) != hipSuccess) {
            if (e0) (void)hipEventDestroy(e0);
            if (stream) (void)hipStreamDestroy(stream);
        }
        return e;
    }
    hipError_t need(size_t dev_bytes, size_t host_bytes)
    {
        hipError_t e = d.need(dev_bytes, dev_bytes + dev_bytes / 4);
        return e == hipSuccess ? h.need(host_bytes, host_bytes + host_bytes / 4) : e;
    }
};
LeasePool<BaWork> g_work; // per process, keyed by device; never freed: the HIP runtime may be gone when static destructors run
// offsets of a call's arrays in the arena (and, for the staged ones, in the page-locked block), 256-byte aligned
struct Layout {
    size_t n = 0;
    size_t add(size_t bytes) { const size_t o = n; n += (bytes + 255) & ~(size_t)255; return o; }
};
// typed addresses in a block -- the device arena or the page-locked staging block -- by byte offset, and copies between the staging
// block and the caller's host arrays
struct Arena {
    uint8_t *base;
    uint8_t *at(size_t off) const { return base + off; }
    double *D(size_t off) const { return reinterpret_cast<double *>(base + off); }
    int *I(size_t off) const { return reinterpret_cast<int *>(base + off); }
    void put(size_t off, const void *src, size_t bytes) const { if (bytes) memcpy(base + off, src, bytes); }
    void get(void *dst, size_t off, size_t bytes) const { if (dst && bytes) memcpy(dst, base + off, bytes); } // an output may be NULL
};
inline int ba_refuse(const BaVerdict &v) { return orbx_set_error(v.code, v.text); }
} // namespace

extern "C" int orbba_linearize(const orbba_problem *p, orbba_result *r, int device)
{
    if (!p || !r) return orbx_set_error(ORBX_E_ARG, "null argument");
    BaIndex ix;
    if (BaVerdict v = ba_check_problem(p, 0); v.code) return ba_refuse(v);
    if (BaVerdict v = ba_build_index(p, false, &ix); v.code) return ba_refuse(v);
    if (int rc = orb_need_device(&device)) return rc;
    ORB_TRY(hipSetDevice(device));
    const int NP = p->n_poses, NL = p->n_points, NE = p->n_edges;
    // arena: [inputs, one copy up][edge-major scratch][outputs, one copy down: the small blocks first, H_lp last]
    Layout L;
    const size_t oR = L.add(72 * (size_t)NP), ot = L.add(24 * (size_t)NP), ofix = L.add(NP), oP = L.add(24 * (size_t)NL),
                 oep = L.add(4 * (size_t)NE), oel = L.add(4 * (size_t)NE), oz = L.add(16 * (size_t)NE), ow = L.add(8 * (size_t)NE),
                 ope = L.add(4 * (size_t)NE), opo = L.add(4 * (size_t)(NP + 1)), olo = L.add(4 * (size_t)(NL + 1));
    const size_t in_bytes = L.n;
    const size_t oCpp = L.add(216 * (size_t)NE), oCll = L.add(72 * (size_t)NE);
    const size_t out_begin = L.n;
    const size_t oHpp = L.add(288 * (size_t)NP), obp = L.add(48 * (size_t)NP), oHll = L.add(72 * (size_t)NL), obl = L.add(24 * (size_t)NL),
                 ochi = L.add(8 * (size_t)NE), oerr = L.add(16 * (size_t)NE);
    const size_t out_small_end = L.n;
    const size_t oHlp = L.add(144 * (size_t)NE);
    const size_t out_end = (r->H_lp && NE) ? L.n : out_small_end;
    Lease<BaWork> lease(g_work);
    ORB_TRY(lease.acquire(device));
    BaWork *w = lease.w;
    ORB_TRY(w->need(L.n, std::max(in_bytes, out_end - out_begin)));
    hipStream_t s = w->stream;
    const Arena a = {w->d.as<uint8_t>()}, h = {w->h.as<uint8_t>()};
    h.put(oR, p->pose_R, 72 * (size_t)NP); h.put(ot, p->pose_t, 24 * (size_t)NP); h.put(ofix, p->pose_fixed, NP);
    h.put(oP, p->points, 24 * (size_t)NL);
    h.put(oep, p->edge_pose, 4 * (size_t)NE); h.put(oel, p->edge_point, 4 * (size_t)NE); h.put(oz, p->edge_z, 16 * (size_t)NE);
    h.put(ow, p->edge_inv_sigma2, 8 * (size_t)NE); h.put(ope, ix.pose_edges.data(), 4 * (size_t)NE);
    h.put(opo, ix.pose_off.data(), 4 * (size_t)(NP + 1)); h.put(olo, ix.point_off.data(), 4 * (size_t)(NL + 1));
    ORB_TRY(hipMemcpyAsync(a.base, h.base, in_bytes, hipMemcpyHostToDevice, s));
    const BaCam cam = make_cam(p);
    ORB_TRY(hipEventRecord(w->e0, s));
    if (NE)
        hipLaunchKernelGGL(k_ba_edges, dim3((NE + 255) / 256), dim3(256), 0, s, cam, NE, a.D(oR), a.D(ot), a.at(ofix), a.D(oP), a.I(oep),
                           a.I(oel), a.D(oz), a.D(ow), (const uint8_t *)nullptr, a.D(ochi), a.D(oerr), a.D(oHlp), a.D(oCpp), a.D(oCll));
    hipLaunchKernelGGL(k_ba_reduce_pose, dim3(NP), dim3(256), 0, s, a.I(opo), a.I(ope), a.D(oCpp), a.D(oHpp), a.D(obp));
    hipLaunchKernelGGL(k_ba_reduce_point, dim3((NL + 255) / 256), dim3(256), 0, s, NL, a.I(olo), a.D(oCll), a.D(oHll), a.D(obl));
    ORB_TRY(hipEventRecord(w->e1, s));
    ORB_TRY(hipGetLastError());
    ORB_TRY(hipMemcpyAsync(h.base, a.at(out_begin), out_end - out_begin, hipMemcpyDeviceToHost, s));
    ORB_TRY(hipStreamSynchronize(s));
    float ms = 0;
    ORB_TRY(hipEventElapsedTime(&ms, w->e0, w->e1));
    r->kernel_ms = ms;
    // an output's place in the staging block is its place in the arena behind out_begin
    h.get(r->chi2, ochi - out_begin, 8 * (size_t)NE); h.get(r->error, oerr - out_begin, 16 * (size_t)NE);
    h.get(r->H_lp, oHlp - out_begin, 144 * (size_t)NE);
    h.get(r->H_pp, oHpp - out_begin, 288 * (size_t)NP); h.get(r->b_p, obp - out_begin, 48 * (size_t)NP);
    h.get(r->H_ll, oHll - out_begin, 72 * (size_t)NL); h.get(r->b_l, obl - out_begin, 24 * (size_t)NL);
    return ORBX_OK;
}


// =====================================================================================================================
// Levenberg-Marquardt with marginalised points on the device: what g2o's
// OptimizationAlgorithmLevenberg + BlockSolver_6_3 do for the graph of Optimize::localBundleAdjustment
// (modules/Backend/Optimize.cpp:811-911).  All f64, fixed-order reductions, the host only takes the accept/reject
// decision of each trial from three scalars.
//   k_lm_points     thread = point: (H_ll + lambda I)^-1 and its product with b_l
//   k_lm_schur      workgroup = one 6x6 block (i, j >= i) of the reduced system over the free poses:
//                   S_ij = [i == j](H_pp + lambda I) - sum_l H_pl(i,l) H_ll^-1 H_pl(j,l)^T,  rhs_i = b_p - sum_l H_pl H_ll^-1 b_l
//   k_lm_chol_solve single workgroup: in-place Cholesky of S and the two triangular solves
//   k_lm_backsub    thread = point: x_l = H_ll^-1 (b_l - sum_e H_pl^T x_p); partial sums of x (lambda x + b)
//   k_lm_update_*   VertexSE3::oplusImpl (exp(update) * estimate, G2oTypes.h:112-115) and Vertex3D::oplusImpl (:155-158)
//   k_lm_chi2       partial sums of the robustified chi2 over the active edges
// =====================================================================================================================
__global__ __launch_bounds__(256) void k_lm_points(int n_points, double lam, const double *__restrict__ Hll,
                                                   const double *__restrict__ bl, double *__restrict__ inv,
                                                   double *__restrict__ tl)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n_points) return;
    const double *h = Hll + (size_t)l * 9;
    const double a = h[0] + lam, b = h[1], c = h[2], d = h[4] + lam, e = h[5], f = h[8] + lam; // symmetric
    const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
    const double det = a * c00 + b * c01 + c * c02;
    const double id = 1.0 / det;
    double m[9];
    m[0] = c00 * id; m[1] = c01 * id; m[2] = c02 * id;
    m[3] = m[1]; m[4] = (a * f - c * c) * id; m[5] = (b * c - a * e) * id;
    m[6] = m[2]; m[7] = m[5]; m[8] = (a * d - b * b) * id;
#pragma unroll
    for (int k = 0; k < 9; ++k) inv[(size_t)l * 9 + k] = m[k];
    const double b0 = bl[3 * l], b1 = bl[3 * l + 1], b2 = bl[3 * l + 2];
    tl[3 * l] = m[0] * b0 + m[1] * b1 + m[2] * b2;
    tl[3 * l + 1] = m[3] * b0 + m[4] * b1 + m[5] * b2;
    tl[3 * l + 2] = m[6] * b0 + m[7] * b1 + m[8] * b2;
}

__global__ __launch_bounds__(256) void k_lm_schur(int n_free, int n_points, double lam, const int *__restrict__ free_pose,
                                                  const int *__restrict__ edge_of /* [n_free][n_points] */,
                                                  const double *__restrict__ Hpp, const double *__restrict__ bp,
                                                  const double *__restrict__ Hlp, const double *__restrict__ inv,
                                                  const double *__restrict__ tl, double *__restrict__ S,
                                                  double *__restrict__ rhs)
{
    __shared__ double red[4][42];
    // block index -> (i, j >= i)
    int i = 0, rem = blockIdx.x;
    while (rem >= n_free - i) { rem -= n_free - i; ++i; }
    const int j = i + rem, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double acc[42];
#pragma unroll
    for (int k = 0; k < 42; ++k) acc[k] = 0.0;
    const int *ei = edge_of + (size_t)i * n_points, *ej = edge_of + (size_t)j * n_points;
    for (int l = tid; l < n_points; l += 256) {
        const int ea = ei[l], eb = ej[l];
        if (ea < 0 || eb < 0) continue;
        const double *A = Hlp + (size_t)ea * 18, *B = Hlp + (size_t)eb * 18, *m = inv + (size_t)l * 9;
        double Cm[18]; // H_ll^-1 * B (3x6)
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) Cm[6 * r + c] = m[3 * r] * B[c] + m[3 * r + 1] * B[6 + c] + m[3 * r + 2] * B[12 + c];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) acc[6 * r + c] += A[r] * Cm[c] + A[6 + r] * Cm[6 + c] + A[12 + r] * Cm[12 + c];
        if (i == j) {
            const double *t = tl + (size_t)l * 3;
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[36 + r] += A[r] * t[0] + A[6 + r] * t[1] + A[12 + r] * t[2];
        }
    }
#pragma unroll
    for (int k = 0; k < 42; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wv][k] = v;
    }
    __syncthreads();
    const int n = 6 * n_free;
    if (tid < 36) {
        const int r = tid / 6, c = tid % 6;
        const double sum = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        double v = -sum;
        if (i == j) v += Hpp[(size_t)free_pose[i] * 36 + tid] + (r == c ? lam : 0.0);
        S[(size_t)(6 * i + r) * n + 6 * j + c] = v;
        if (i != j) S[(size_t)(6 * j + c) * n + 6 * i + r] = v;
    } else if (tid < 42 && i == j) {
        const int r = tid - 36;
        rhs[6 * i + r] = bp[(size_t)free_pose[i] * 6 + r] - ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]));
    }
}

// S (n x n, row-major, lower triangle used) -> L in place; x = S^-1 rhs.  *ok = 0 if a pivot is not positive.
// The same solve with the system resident in LDS (n <= CH_MAX_N, i.e. up to 23 free key frames: (n + 1)^2 doubles).  The global-
// memory kernel below pays three workgroup barriers and as many memory round trips per column (0.52 ms for n = 114, two thirds
// of a local-BA iteration); here a column costs ONE barrier:
//   * the right-hand side rides along as row n of the matrix, so the forward substitution L y = rhs falls out of the
//     factorisation (row n of L is y^T);
//   * step k reads the unscaled column k of the lower triangle, scales on the fly (every thread computes 1 / sqrt(d_k) itself)
//     and writes the scaled column -- L's column k -- into ROW k of the upper triangle, which no step reads: nothing is read
//     and written in one step (1 / L[k][k] goes to an array of its own: a slow thread may still be reading d_k);
//   * thread (tr, tc) of a (CH_T / 16) x 16 grid owns the elements r = tr mod CH_T / 16, c = tc mod 16: no index division;
//   * L^T x = y is solved by ONE wave without barriers (lane owns x[lane], x[lane + 64], x[lane + 128]; x[k] is broadcast
//     with a lane read; the column of the step after is requested before the current one is used).
// Operation order differs from LAPACK's (the oracle) at rounding level only; the LM tests compare at 1e-6.
// Measured for n = 114 (tools/ba_kernel_stats.sh): 0.52 ms -> 0.13; of that 0.04 are the load, the barriers and the back
// substitution, 0.09 the element updates.  Variants that lost: the next pivot's reciprocal square root on an extra wave
// (0.14: the chain is 0.1 us of a step's 1.2), a step's operands of a row -- or of the whole step -- requested before the first
// store (0.17 / 0.39: nine predicated accesses per row cost more than the two or three real ones they wait for).
#ifndef CH_T
#define CH_T 512
#endif
#define CH_MAX_N 140
__global__ __launch_bounds__(CH_T) void k_lm_chol_solve_lds(int n, const double *__restrict__ S, const double *__restrict__ rhs,
                                                            double *__restrict__ x, int *__restrict__ ok)
{
    extern __shared__ __align__(16) double A[]; // (n + 1) rows x P columns, then 1 / L[k][k] for every k
    const int tid = threadIdx.x, P = n + 1;
    double *dinv = A + (size_t)(n + 1) * P;
    for (int i = tid; i < n * n; i += CH_T) {
        const int r = i / n, c = i - r * n;
        if (c <= r) A[r * P + c] = S[i];
    }
    for (int i = tid; i < n; i += CH_T) A[n * P + i] = rhs[i];
    __syncthreads();
    constexpr int TR = CH_T / 16;
    const int tr = tid >> 4, tc = tid & 15;
    bool bad = false;
    for (int k = 0; k < n; ++k) {
        const double d = A[k * P + k];
        if (!(d > 0.0)) { bad = true; break; } // (every thread reads the same value: a uniform exit)
        const double inv = 1.0 / sqrt(d);
        // first row / column of this thread's residue class beyond k
        const int r0 = k + 1 + ((tr - (k + 1)) & (TR - 1)), c0 = k + 1 + ((tc - (k + 1)) & 15);
        for (int r = r0; r <= n; r += TR) {
            const double lr = A[r * P + k] * inv;
            const int cend = r < n ? r : n - 1;
            for (int c = c0; c <= cend; c += 16) A[r * P + c] -= lr * (A[c * P + k] * inv);
            if (tc == 0) A[k * P + r] = lr; // L[r][k]; r = n: y[k]
        }
        if (tid == 0) dinv[k] = inv;
        __syncthreads();
    }
    if (bad) {
        if (tid == 0) *ok = 0;
        for (int i = tid; i < n; i += CH_T) x[i] = 0.0;
        return;
    }
    if (tid >= 64) return;
    // L^T x = y: L[k][r] (r < k) lies at A[r][k]; y[k] at A[k][n]
    constexpr int SL = (CH_MAX_N + 63) / 64;
    double y[SL], a[SL], an[SL];
#pragma unroll
    for (int q = 0; q < SL; ++q) {
        const int r = min(tid + 64 * q, n - 1);
        y[q] = A[r * P + n];
        an[q] = A[r * P + n - 1];
    }
    double di = dinv[n - 1];
    for (int k = n - 1; k >= 0; --k) {
        const double dk = di;
#pragma unroll
        for (int q = 0; q < SL; ++q) a[q] = an[q];
        if (k > 0) { // the step after's operands: independent of this step's result
            di = dinv[k - 1];
#pragma unroll
            for (int q = 0; q < SL; ++q) an[q] = A[min(tid + 64 * q, n - 1) * P + k - 1];
        }
        const int kq = k >> 6, kl = k & 63; // wave-uniform
        double ysel = y[0];
#pragma unroll
        for (int q = 1; q < SL; ++q) ysel = q == kq ? y[q] : ysel;
        const int lo = __builtin_amdgcn_readlane((int)(__double_as_longlong(ysel) & 0xFFFFFFFFll), kl);
        const int hi = __builtin_amdgcn_readlane((int)(__double_as_longlong(ysel) >> 32), kl);
        const double xk = __longlong_as_double(((long long)hi << 32) | (unsigned int)lo) * dk;
#pragma unroll
        for (int q = 0; q < SL; ++q) {
            const int r = tid + 64 * q;
            if (r < k) y[q] -= a[q] * xk;
            else if (r == k) y[q] = xk;
        }
    }
#pragma unroll
    for (int q = 0; q < SL; ++q)
        if (tid + 64 * q < n) x[tid + 64 * q] = y[q];
    if (tid == 0) *ok = 1;
}

__global__ __launch_bounds__(256) void k_lm_chol_solve(int n, double *__restrict__ S, const double *__restrict__ rhs,
                                                       double *__restrict__ x, int *__restrict__ ok)
{
    __shared__ int bad;
    const int tid = threadIdx.x;
    if (tid == 0) bad = 0;
    for (int i = tid; i < n; i += 256) x[i] = rhs[i];
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        if (tid == 0) {
            const double d = S[(size_t)k * n + k];
            if (!(d > 0.0)) bad = 1;
            else S[(size_t)k * n + k] = sqrt(d);
        }
        __syncthreads();
        if (bad) break;
        const double dk = S[(size_t)k * n + k];
        for (int r = k + 1 + tid; r < n; r += 256) S[(size_t)r * n + k] /= dk;
        __syncthreads();
        const int m = n - k - 1;
        for (int idx = tid; idx < m * m; idx += 256) {
            const int r = k + 1 + idx / m, c = k + 1 + idx % m;
            if (c <= r) S[(size_t)r * n + c] -= S[(size_t)r * n + k] * S[(size_t)c * n + k];
        }
        __syncthreads();
    }
    if (bad) {
        if (tid == 0) *ok = 0;
        for (int i = tid; i < n; i += 256) x[i] = 0.0;
        return;
    }
    for (int k = 0; k < n; ++k) { // L y = rhs
        if (tid == 0) x[k] /= S[(size_t)k * n + k];
        __syncthreads();
        const double yk = x[k];
        for (int r = k + 1 + tid; r < n; r += 256) x[r] -= S[(size_t)r * n + k] * yk;
        __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) { // L^T x = y
        if (tid == 0) x[k] /= S[(size_t)k * n + k];
        __syncthreads();
        const double xk = x[k];
        for (int r = tid; r < k; r += 256) x[r] -= S[(size_t)k * n + r] * xk;
        __syncthreads();
    }
    if (tid == 0) *ok = 1;
}

__device__ __forceinline__ double block_sum_256(double v, double *red4)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

__global__ __launch_bounds__(256) void k_lm_backsub(int n_points, double lam, const int *__restrict__ point_off,
                                                    const int *__restrict__ edge_pose, const int *__restrict__ pose_slot,
                                                    const double *__restrict__ Hlp, const double *__restrict__ xp,
                                                    const double *__restrict__ bl, const double *__restrict__ inv,
                                                    double *__restrict__ xl, double *__restrict__ partial)
{
    __shared__ double red4[4];
    const int l = blockIdx.x * 256 + threadIdx.x;
    double sc = 0.0;
    if (l < n_points) {
        double r0 = bl[3 * l], r1 = bl[3 * l + 1], r2 = bl[3 * l + 2];
        for (int e = point_off[l]; e < point_off[l + 1]; ++e) {
            const int s = pose_slot[edge_pose[e]];
            if (s < 0) continue;
            const double *A = Hlp + (size_t)e * 18, *q = xp + 6 * s;
#pragma unroll
            for (int c = 0; c < 6; ++c) { r0 -= A[c] * q[c]; r1 -= A[6 + c] * q[c]; r2 -= A[12 + c] * q[c]; }
        }
        const double *m = inv + (size_t)l * 9;
        const double x0 = m[0] * r0 + m[1] * r1 + m[2] * r2, x1 = m[3] * r0 + m[4] * r1 + m[5] * r2,
                     x2 = m[6] * r0 + m[7] * r1 + m[8] * r2;
        xl[3 * l] = x0; xl[3 * l + 1] = x1; xl[3 * l + 2] = x2;
        sc = x0 * (lam * x0 + bl[3 * l]) + x1 * (lam * x1 + bl[3 * l + 1]) + x2 * (lam * x2 + bl[3 * l + 2]);
    }
    const double tot = block_sum_256(sc, red4);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// one workgroup: poses <- exp(x_p) * poses for the free poses, and their share of computeScale()
__global__ __launch_bounds__(256) void k_lm_update_poses(int n_free, double lam, const int *__restrict__ free_pose,
                                                         const double *__restrict__ xp, const double *__restrict__ bp,
                                                         double *__restrict__ R, double *__restrict__ t,
                                                         double *__restrict__ scale_out)
{
    __shared__ double red4[4];
    double sc = 0.0;
    for (int i = threadIdx.x; i < n_free; i += 256) {
        const int ip = free_pose[i];
        const double *u = xp + 6 * i;
        const double wx = u[0], wy = u[1], wz = u[2];
#pragma unroll
        for (int k = 0; k < 6; ++k) sc += u[k] * (lam * u[k] + bp[(size_t)ip * 6 + k]);
        // g2o SE3Quat::exp
        const double th = sqrt(wx * wx + wy * wy + wz * wz);
        const double K[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
        double K2[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) K2[3 * r + c] = K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c] + K[3 * r + 2] * K[6 + c];
        double ra, rb, va, vb;
        if (th < 0.00001) { ra = 1.0; rb = 0.5; va = 0.5; vb = 1.0 / 6.0; }
        else {
            ra = sin(th) / th; rb = (1.0 - cos(th)) / (th * th);
            va = rb; vb = (th - sin(th)) / (th * th * th);
        }
        double E[9], V[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double I = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
            E[k] = I + ra * K[k] + rb * K2[k];
            V[k] = I + va * K[k] + vb * K2[k];
        }
        double Rn[9], tn[3];
        const double *Ro = R + (size_t)ip * 9, *to = t + (size_t)ip * 3;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) Rn[3 * r + c] = E[3 * r] * Ro[c] + E[3 * r + 1] * Ro[3 + c] + E[3 * r + 2] * Ro[6 + c];
            tn[r] = (E[3 * r] * to[0] + E[3 * r + 1] * to[1] + E[3 * r + 2] * to[2]) +
                    (V[3 * r] * u[3] + V[3 * r + 1] * u[4] + V[3 * r + 2] * u[5]);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) R[(size_t)ip * 9 + k] = Rn[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[(size_t)ip * 3 + k] = tn[k];
    }
    const double tot = block_sum_256(sc, red4);
    if (threadIdx.x == 0) *scale_out = tot;
}

__global__ __launch_bounds__(256) void k_lm_update_points(int n3, const double *__restrict__ xl, double *__restrict__ P)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n3) P[i] += xl[i];
}

__global__ __launch_bounds__(256) void k_lm_chi2(int n_edges, double delta, const double *__restrict__ chi2,
                                                 const uint8_t *__restrict__ active, double *__restrict__ partial)
{
    __shared__ double red4[4];
    const int e = blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (e < n_edges && (!active || active[e])) {
        v = chi2[e];
        if (delta > 0.0 && v > delta * delta) v = 2.0 * delta * sqrt(v) - delta * delta; // RobustKernelHuber rho[0]
    }
    const double tot = block_sum_256(v, red4);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// computeLambdaInit (g2o OptimizationAlgorithmLevenberg): max |H_jj| over the free poses' and the points' diagonal entries.
// One workgroup; a maximum does not depend on the order it is taken in.
__global__ __launch_bounds__(256) void k_lm_diag_max(int n_free, const int *__restrict__ free_pose, const double *__restrict__ Hpp,
                                                     int n_points, const double *__restrict__ Hll, double *__restrict__ out)
{
    __shared__ double red4[4];
    double mx = 0.0;
    for (int i = threadIdx.x; i < 6 * n_free; i += 256) mx = fmax(mx, fabs(Hpp[(size_t)36 * free_pose[i / 6] + 7 * (i % 6)]));
    for (int i = threadIdx.x; i < 3 * n_points; i += 256) mx = fmax(mx, fabs(Hll[(size_t)9 * (i / 3) + 4 * (i % 3)]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) *out = fmax(fmax(red4[0], red4[1]), fmax(red4[2], red4[3]));
}

namespace {
// One LM problem in the arena: its sizes and the offsets of its arrays.  What a host form brings back leads -- [read-back block]
// [chi2 out][outlier out][estimates R t P], ONE copy down from wherever the caller's first output lies -- and the estimates also open
// what it sends: [oR, in_end) is its ONE copy up.  The device form copies the caller's arrays in and builds the index structures in
// place (below), before it knows the number of free poses: everything up to and including o_edge_of's START does not depend on it.
struct LmPlan {
    int NP, NL, NE, NF, N, EB, LB;
    size_t ochio, oout, orb;                                       // results of the host forms besides the estimates
    size_t oR, ot, oP, est_bytes, est_end;                         // the estimates, in and out
    size_t ofix, oep, oel, oz, ow, oact, opo, ope, olo, oslot, ofree, oix, oeo, in_end;
    size_t oRb, oHlp, oCpp, oCll, oHpp, obp, oHll, obl, oinv, otl, oS, orhs, oxp, oxl, ochi, ochi1, bytes;
    // what the host reads per trial, ONE copy: [chi2 partials at the iteration's estimate: EB][at the trial's: EB]
    // [computeScale partials of the points: LB][of the poses: 1][max |H_jj|: 1][Cholesky flag: int in 8 bytes]
    int RB_CUR, RB_TRY, RB_SCL, RB_POSE, RB_MAX, RB_FLAG, RB_N;
};
LmPlan lm_plan(int NP, int NL, int NE, int NF)
{
    LmPlan q = {};
    q.NP = NP, q.NL = NL, q.NE = NE, q.NF = NF, q.N = 6 * NF, q.EB = (NE + 255) / 256, q.LB = (NL + 255) / 256;
    const int N = q.N;
    q.RB_CUR = 0, q.RB_TRY = q.EB, q.RB_SCL = 2 * q.EB, q.RB_POSE = 2 * q.EB + q.LB, q.RB_MAX = q.RB_POSE + 1, q.RB_FLAG = q.RB_POSE + 2;
    q.RB_N = q.RB_POSE + 3;
    // arena: [chi2 out][outlier out][read-back block][estimates R t P -- in and out][other inputs][scratch]
    Layout L;
    q.ochio = L.add(8 * (size_t)NE), q.oout = L.add(NE), q.orb = L.add(8 * (size_t)q.RB_N);
    q.oR = L.add(72 * (size_t)NP), q.ot = L.add(24 * (size_t)NP), q.oP = L.add(24 * (size_t)NL);
    q.est_bytes = L.n - q.oR, q.est_end = L.n;
    q.ofix = L.add(NP), q.oep = L.add(4 * (size_t)NE), q.oel = L.add(4 * (size_t)NE), q.oz = L.add(16 * (size_t)NE);
    q.ow = L.add(8 * (size_t)NE), q.oact = L.add(NE), q.opo = L.add(4 * (size_t)(NP + 1)), q.ope = L.add(4 * (size_t)NE);
    q.olo = L.add(4 * (size_t)(NL + 1)), q.oslot = L.add(4 * (size_t)NP), q.ofree = L.add(4 * (size_t)NP), q.oix = L.add(64);
    q.oeo = L.add((size_t)4 * NF * NL);
    q.in_end = L.n;
    q.oRb = L.add(q.est_bytes); // push() / pop(): R, t, P kept in the same relative layout
    q.oHlp = L.add(144 * (size_t)NE), q.oCpp = L.add(216 * (size_t)NE), q.oCll = L.add(72 * (size_t)NE);
    q.oHpp = L.add(288 * (size_t)NP), q.obp = L.add(48 * (size_t)NP), q.oHll = L.add(72 * (size_t)NL), q.obl = L.add(24 * (size_t)NL);
    q.oinv = L.add(72 * (size_t)NL), q.otl = L.add(24 * (size_t)NL), q.oS = L.add((size_t)8 * N * N), q.orhs = L.add(8 * (size_t)N);
    q.oxp = L.add(8 * (size_t)N), q.oxl = L.add(24 * (size_t)NL);
    q.ochi = L.add(8 * (size_t)NE), q.ochi1 = L.add(8 * (size_t)NE);
    q.bytes = L.n;
    return q;
}

struct LmKnobs { int max_iterations, max_trials; double tau, lower, upper, user_lambda_init; };
struct LmOutcome { int iterations, trials; double lambda, chi_initial; };
LmKnobs lm_knobs(const orbba_lm_options *o)
{
    return {o->max_iterations, o->max_trials > 0 ? o->max_trials : 10, o->tau > 0 ? o->tau : 1e-5,
            o->good_step_lower > 0 ? o->good_step_lower : 1.0 / 3.0, o->good_step_upper > 0 ? o->good_step_upper : 2.0 / 3.0, o->user_lambda_init};
}
inline double lm_sum(const double *rb, int from, int n) { double v = 0.0; for (int b = 0; b < n; ++b) v += rb[from + b]; return v; }

// optimizer.optimize(max_iterations) on a problem that lies in the arena `a` as `q` describes it, index structures included, enqueued on
// `s`; `rb` is the page-locked read-back block.  THE loop: the host-pointer and the device-pointer entry points both run it.  It waits
// on `s` once per trial and returns behind the last evaluation, whose chi2 partials (q.RB_TRY) the caller reads back with its results.
int lm_loop(const LmPlan &q, const Arena &a, double *rb, hipStream_t s, const BaCam &cam, const uint8_t *d_active, const LmKnobs &o, LmOutcome *out)
{
    // errors at the current estimate (+ the whole linearisation when `full`); activeRobustChi2 as partial sums into the
    // read-back block's slot `slot`
    auto evaluate = [&](bool full, int slot) {
        hipLaunchKernelGGL(k_ba_edges, dim3(q.EB), dim3(256), 0, s, cam, q.NE, a.D(q.oR), a.D(q.ot), a.at(q.ofix), a.D(q.oP), a.I(q.oep),
                           a.I(q.oel), a.D(q.oz), a.D(q.ow), d_active, a.D(q.ochi), (double *)nullptr, full ? a.D(q.oHlp) : nullptr,
                           full ? a.D(q.oCpp) : nullptr, full ? a.D(q.oCll) : nullptr);
        if (full) {
            hipLaunchKernelGGL(k_ba_reduce_pose, dim3(q.NP), dim3(256), 0, s, a.I(q.opo), a.I(q.ope), a.D(q.oCpp), a.D(q.oHpp), a.D(q.obp));
            hipLaunchKernelGGL(k_ba_reduce_point, dim3(q.LB), dim3(256), 0, s, q.NL, a.I(q.olo), a.D(q.oCll), a.D(q.oHll), a.D(q.obl));
        }
        hipLaunchKernelGGL(k_lm_chi2, dim3(q.EB), dim3(256), 0, s, q.NE, cam.delta, a.D(q.ochi), d_active, a.D(q.orb) + slot);
    };
    // the read-back block in host memory: the call's only waits besides the final one
    auto read_back = [&]() -> int {
        ORB_TRY(hipGetLastError());
        ORB_TRY(hipMemcpyAsync(rb, a.at(q.orb), 8 * (size_t)q.RB_N, hipMemcpyDeviceToHost, s));
        ORB_TRY(hipStreamSynchronize(s));
        return ORBX_OK;
    };
    auto sum = [&](int from, int n) { return lm_sum(rb, from, n); };

    LmPolicy p = {0.0, 2.0, 0.0, 0.0, 0, o.lower, o.upper};
    double chi_initial = 0.0;
    int its = 0, trials_total = 0, rc = ORBX_OK;
    for (int it = 0; it < o.max_iterations; ++it) {
        evaluate(true, q.RB_CUR);
        bool have_current = false;
        if (it == 0) {
            if (o.user_lambda_init > 0) p.lam = o.user_lambda_init;
            else { // computeLambdaInit: tau * max |H_jj| over the free vertices
                hipLaunchKernelGGL(k_lm_diag_max, dim3(1), dim3(256), 0, s, q.NF, a.I(q.ofree), a.D(q.oHpp), q.NL, a.D(q.oHll),
                                   a.D(q.orb) + q.RB_MAX);
                if ((rc = read_back())) return rc;
                p.lam = o.tau * rb[q.RB_MAX];
                p.current = sum(q.RB_CUR, q.EB);
                have_current = true;
            }
            p.ni = 2.0;
        }
        lm_policy_iteration(p, p.current); // `current` itself arrives with the first trial's read-back, unless computeLambdaInit has fetched it
        LmTrial t;
        do {
            // push(): keep the estimates
            ORB_TRY(hipMemcpyAsync(a.at(q.oRb), a.at(q.oR), q.est_bytes, hipMemcpyDeviceToDevice, s)); // R, t, P and their copies are laid out alike
            hipLaunchKernelGGL(k_lm_points, dim3(q.LB), dim3(256), 0, s, q.NL, p.lam, a.D(q.oHll), a.D(q.obl), a.D(q.oinv), a.D(q.otl));
            hipLaunchKernelGGL(k_lm_schur, dim3(q.NF * (q.NF + 1) / 2), dim3(256), 0, s, q.NF, q.NL, p.lam, a.I(q.ofree), a.I(q.oeo), a.D(q.oHpp),
                               a.D(q.obp), a.D(q.oHlp), a.D(q.oinv), a.D(q.otl), a.D(q.oS), a.D(q.orhs));
            int *const d_flag = reinterpret_cast<int *>(a.D(q.orb) + q.RB_FLAG);
            // ORBBA_VAR_CHOL = 1: the global-memory kernel, the parity twin (read per call)
            bool in_lds = q.N <= CH_MAX_N && g_ba_chol.load() == 0;
            if (in_lds) {
                const size_t lds = sizeof(double) * ((size_t)(q.N + 1) * (q.N + 1) + q.N);
                // per device; when the opt-in or the launch is refused the global-memory kernel solves the system instead --
                // a launch that did not happen would leave the previous iteration's step in xp / the flag
                in_lds = orbx_lds_opt_in(reinterpret_cast<const void *>(k_lm_chol_solve_lds), lds) == hipSuccess;
                if (in_lds) {
                    hipLaunchKernelGGL(k_lm_chol_solve_lds, dim3(1), dim3(CH_T), lds, s, q.N, a.D(q.oS), a.D(q.orhs), a.D(q.oxp), d_flag);
                    in_lds = hipGetLastError() == hipSuccess;
                }
            }
            if (!in_lds) {
                hipLaunchKernelGGL(k_lm_chol_solve, dim3(1), dim3(256), 0, s, q.N, a.D(q.oS), a.D(q.orhs), a.D(q.oxp), d_flag);
                ORB_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(k_lm_backsub, dim3(q.LB), dim3(256), 0, s, q.NL, p.lam, a.I(q.olo), a.I(q.oep), a.I(q.oslot), a.D(q.oHlp), a.D(q.oxp),
                               a.D(q.obl), a.D(q.oinv), a.D(q.oxl), a.D(q.orb) + q.RB_SCL);
            hipLaunchKernelGGL(k_lm_update_poses, dim3(1), dim3(256), 0, s, q.NF, p.lam, a.I(q.ofree), a.D(q.oxp), a.D(q.obp), a.D(q.oR), a.D(q.ot),
                               a.D(q.orb) + q.RB_POSE);
            hipLaunchKernelGGL(k_lm_update_points, dim3((3 * q.NL + 255) / 256), dim3(256), 0, s, 3 * q.NL, a.D(q.oxl), a.D(q.oP));
            evaluate(false, q.RB_TRY);
            if ((rc = read_back())) return rc;
            if (!have_current) { p.current = sum(q.RB_CUR, q.EB); have_current = true; }
            if (it == 0 && p.qmax == 0) chi_initial = p.current;
            const double temp = sum(q.RB_TRY, q.EB);
            int ok2 = 0;
            memcpy(&ok2, rb + q.RB_FLAG, sizeof(int));
            double scale = rb[q.RB_POSE]; // poses first, then the points block by block
            for (int b = 0; b < q.LB; ++b) scale += rb[q.RB_SCL + b];
            // one total and the whole of computeScale, summed in its order: the policy's + 0.0 on each is exact
            t = lm_policy_trial(p, ok2 != 0, temp, 0.0, scale, 0.0);
            ++trials_total;
            if (!t.accepted) ORB_TRY(hipMemcpyAsync(a.at(q.oR), a.at(q.oRb), q.est_bytes, hipMemcpyDeviceToDevice, s)); // pop(): restore
        } while (lm_policy_again(p, t, o.max_trials));
        ++its;
        if (lm_policy_terminate(p, o.max_trials)) break;
    }
    evaluate(false, q.RB_TRY);
    ORB_TRY(hipGetLastError());
    out->iterations = its, out->trials = trials_total, out->lambda = p.lam, out->chi_initial = chi_initial;
    return ORBX_OK;
}

// ---- what the two host-pointer LM entry points share around their loops.  The staging block mirrors the arena up to q.in_end.
// The ONE copy up: the estimates, the problem, the mask if there is one, and the index structures
int lm_upload(const LmPlan &q, const Arena &a, const Arena &h, const orbba_problem *p, const uint8_t *edge_active, const BaIndex &ix, hipStream_t s)
{
    const size_t NP = q.NP, NL = q.NL, NE = q.NE, NF = q.NF;
    h.put(q.oR, p->pose_R, 72 * NP); h.put(q.ot, p->pose_t, 24 * NP); h.put(q.oP, p->points, 24 * NL);
    h.put(q.ofix, p->pose_fixed, NP); h.put(q.oep, p->edge_pose, 4 * NE); h.put(q.oel, p->edge_point, 4 * NE);
    h.put(q.oz, p->edge_z, 16 * NE); h.put(q.ow, p->edge_inv_sigma2, 8 * NE);
    if (edge_active) h.put(q.oact, edge_active, NE);
    h.put(q.opo, ix.pose_off.data(), 4 * (NP + 1)); h.put(q.ope, ix.pose_edges.data(), 4 * NE);
    h.put(q.olo, ix.point_off.data(), 4 * (NL + 1)); h.put(q.ofree, ix.free_pose.data(), 4 * NF);
    h.put(q.oslot, ix.pose_slot.data(), 4 * NP); h.put(q.oeo, ix.edge_of.data(), 4 * NF * NL);
    ORB_TRY(hipMemcpyAsync(a.at(q.oR), h.at(q.oR), q.in_end - q.oR, hipMemcpyHostToDevice, s));
    return ORBX_OK;
}
// behind a call's last wait: the scalars the loops left in `out`, chi2_final from the last evaluation's partial sums in the read-back
// block, the time between the workspace's two events
int lm_report(const LmPlan &q, const double *rb, const BaWork *w, const LmOutcome &out, orbba_lm_result *r)
{
    float ms = 0;
    ORB_TRY(hipEventElapsedTime(&ms, w->e0, w->e1));
    r->iterations = out.iterations;
    r->trials = out.trials;
    r->lambda = out.lambda;
    r->chi2_initial = out.chi_initial;
    r->chi2_final = lm_sum(rb, q.RB_TRY, q.EB);
    r->device_ms = ms;
    return ORBX_OK;
}
// The ONE copy down, from `from` (q.ochio, q.oout or q.orb: the first block the caller wants) to the end of the estimates, the wait,
// and the copy-out: the scalars, and the estimates and chi2 into whichever of r's arrays are not NULL
int lm_download(const LmPlan &q, const Arena &a, const Arena &h, size_t from, hipStream_t s, const BaWork *w, const LmOutcome &out, orbba_lm_result *r)
{
    const size_t NP = q.NP, NL = q.NL, NE = q.NE;
    ORB_TRY(hipMemcpyAsync(h.at(from), a.at(from), q.est_end - from, hipMemcpyDeviceToHost, s));
    ORB_TRY(hipStreamSynchronize(s));
    h.get(r->pose_R, q.oR, 72 * NP); h.get(r->pose_t, q.ot, 24 * NP); h.get(r->points, q.oP, 24 * NL); h.get(r->chi2, q.ochio, 8 * NE);
    return lm_report(q, h.D(q.orb), w, out, r);
}

} // namespace

extern "C" int orbba_optimize(const orbba_problem *p, const orbba_lm_options *o, orbba_lm_result *r, int device)
{
    if (!p || !o || !r) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (BaVerdict v = ba_check_problem(p, 1); v.code) return ba_refuse(v);
    if (o->max_iterations < 0) return orbx_set_error(ORBX_E_ARG, "negative iteration count");
    BaIndex ix;                          // (the device form builds the same structures with k_lmi_*, below)
    if (BaVerdict v = ba_build_index(p, true, &ix); v.code) return ba_refuse(v);
    if (int rc = orb_need_device(&device)) return rc;
    ORB_TRY(hipSetDevice(device));
    const LmPlan q = lm_plan(p->n_poses, p->n_points, p->n_edges, (int)ix.free_pose.size());
    Lease<BaWork> lease(g_work);
    ORB_TRY(lease.acquire(device));
    BaWork *w = lease.w;
    ORB_TRY(w->need(q.bytes, q.in_end));
    hipStream_t s = w->stream;
    const Arena a = {w->d.as<uint8_t>()}, h = {w->h.as<uint8_t>()};
    if (int rc = lm_upload(q, a, h, p, o->edge_active, ix, s)) return rc;
    const BaCam cam = make_cam(p);
    ORB_TRY(hipEventRecord(w->e0, s));
    LmOutcome out = {};
    if (int rc = lm_loop(q, a, h.D(q.orb), s, cam, o->edge_active ? a.at(q.oact) : nullptr, lm_knobs(o), &out)) return rc;
    ORB_TRY(hipEventRecord(w->e1, s));
    if (r->chi2) ORB_TRY(hipMemcpyAsync(a.at(q.ochio), a.at(q.ochi), 8 * (size_t)q.NE, hipMemcpyDeviceToDevice, s)); // chi2 at the final estimate
    if (int rc = lm_download(q, a, h, r->chi2 ? q.ochio : q.orb, s, w, out, r)) return rc;
    if (o->max_iterations == 0) r->chi2_initial = r->chi2_final; // no trial has set it
    return ORBX_OK;
}

// =====================================================================================================================
// The same on a problem that lies in DEVICE memory (include/orbba.h: orbba_local_bundle_adjustment_device), as
// orbm_local_ba_problem_device leaves it.  The index structures the host forms build on the host (orbba_problem.h) are built here by
// the k_lmi_* kernels, with their checks; both rounds then run lm_loop on them, and the demotion between the rounds and the outlier
// rule behind them are two small kernels (lba_rounds: the host form runs the same function).  Every structure is a function of the edge arrays alone -- counts are sums, a cell of edge_of has one
// writer in a problem that passes the checks, pose_edges is placed in edge order by a block scan -- so the bytes equal the host's.
//   k_lmi_count   thread = edge: index ranges, edges grouped by point; edges per pose into pose_off[pose + 1]
//   k_lmi_poses   one workgroup: pose_off scanned in place; free_pose / pose_slot / the number of free poses by a scan of the flags
//   k_lmi_place   workgroup = pose: its edges in edge order -> pose_edges (reads every edge once per pose: n_poses * n_edges reads)
//   k_lmi_fill    edge_of = -1, free poses x points (the number of free poses is read from device memory)
//   k_lmi_cells   thread = edge: edge_of[slot of its pose][point] = edge; a cell taken twice = a point observed twice by a key frame
//   k_lmi_points  thread = point: point_off = the first edge whose point is not below it (the edges are sorted by point)
// =====================================================================================================================
enum { LMI_FLAG = 0, LMI_NF = 1 };                                  // the index block (q.oix): error bits, free poses
enum { LMI_E_RANGE = 1, LMI_E_ORDER = 2, LMI_E_TWICE = 4, LMI_E_ALL_FIXED = 8 };

__global__ __launch_bounds__(256) void k_lmi_count(int NP, int NL, int NE, const int *__restrict__ ep, const int *__restrict__ el,
                                                   int *__restrict__ pose_off, int *__restrict__ ix)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const int ip = ep[e], il = el[e];
    int err = 0;
    if (ip < 0 || ip >= NP || il < 0 || il >= NL) err |= LMI_E_RANGE;
    else atomicAdd(&pose_off[ip + 1], 1);
    if (e && il < el[e - 1]) err |= LMI_E_ORDER;
    if (err) atomicOr(&ix[LMI_FLAG], err);
}

__global__ __launch_bounds__(1024) void k_lmi_poses(int NP, const uint8_t *__restrict__ fixed, int *__restrict__ pose_off,
                                                    int *__restrict__ free_pose, int *__restrict__ pose_slot, int *__restrict__ ix)
{
    __shared__ int s_wave[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = (NP + 1023) / 1024;
    const int j0 = min(tid * chunk, NP), j1 = min(j0 + chunk, NP);
    int edges = 0, n_free = 0;
    for (int j = j0; j < j1; ++j) edges += pose_off[j + 1], n_free += !fixed[j];
    const int ie = wave_scan(edges), in = wave_scan(n_free);
    if (lane == 63) s_wave[0][wave] = ie, s_wave[1][wave] = in;
    __syncthreads();
    int before_e = ie - edges, before_f = in - n_free, total_f = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wave) before_e += s_wave[0][w], before_f += s_wave[1][w];
        total_f += s_wave[1][w];
    }
    for (int j = j0; j < j1; ++j) {
        before_e += pose_off[j + 1];
        pose_off[j + 1] = before_e;
        if (fixed[j]) pose_slot[j] = -1;
        else pose_slot[j] = before_f, free_pose[before_f++] = j;
    }
    if (tid == 0) {
        pose_off[0] = 0;
        ix[LMI_NF] = total_f;
        if (total_f < 1) atomicOr(&ix[LMI_FLAG], LMI_E_ALL_FIXED);
    }
}

__global__ __launch_bounds__(256) void k_lmi_place(int NE, const int *__restrict__ ep, const int *__restrict__ pose_off,
                                                   int *__restrict__ pose_edges)
{
    __shared__ int s_wave[4];
    const int ip = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int at = pose_off[ip];
    const int end = pose_off[ip + 1];
    for (int e0 = 0; e0 < NE && at < end; e0 += 256) {
        const int e = e0 + tid;
        const int is_mine = e < NE && ep[e] == ip;
        const int incl = wave_scan(is_mine);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = incl - is_mine, total = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        if (is_mine && at + before < min(end, NE)) pose_edges[at + before] = e;
        at += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_lmi_fill(int NL, const int *__restrict__ ix, int cap, int *__restrict__ edge_of)
{
    const long long all = (long long)ix[LMI_NF] * NL, n = all < cap ? all : cap;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) edge_of[i] = -1;
}

__global__ __launch_bounds__(256) void k_lmi_cells(int NP, int NL, int NE, const int *__restrict__ ep, const int *__restrict__ el,
                                                   const int *__restrict__ pose_slot, int *__restrict__ edge_of, int *__restrict__ ix)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const int ip = ep[e], il = el[e];
    if (ip < 0 || ip >= NP || il < 0 || il >= NL) return;
    const int slot = pose_slot[ip];
    if (slot < 0) return;
    if (atomicCAS(&edge_of[(size_t)slot * NL + il], -1, e) != -1) atomicOr(&ix[LMI_FLAG], LMI_E_TWICE);
}

__global__ __launch_bounds__(256) void k_lmi_points(int NL, int NE, const int *__restrict__ el, int *__restrict__ point_off)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l > NL) return;
    int lo = 0, hi = NE;                                           // the first edge whose point is >= l
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (el[mid] < l) lo = mid + 1;
        else hi = mid;
    }
    point_off[l] = lo;
}

// Optimize.cpp:899-902 between the rounds: the demotion mask, and the first round's chi2 kept for the demoted edges
__global__ __launch_bounds__(256) void k_lba_demote(int NE, const double *__restrict__ chi, uint8_t *__restrict__ active, double *__restrict__ chi1)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const double c = chi[e];
    active[e] = !(c > 5.991);
    chi1[e] = c;
}

// :917-921 behind the second round: a demoted edge keeps its stale first-round chi2 (see orbba_local_bundle_adjustment), the outliers
__global__ __launch_bounds__(256) void k_lba_outliers(int NE, const double *__restrict__ chi, const uint8_t *__restrict__ active,
                                                      const double *__restrict__ chi1, double *__restrict__ chi_out, uint8_t *__restrict__ outlier)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= NE) return;
    const double c = active[e] ? chi[e] : chi1[e];
    chi_out[e] = c;
    outlier[e] = !active[e] || c > 5.991;
}

namespace {
// Optimize.cpp:892-922 on a problem that lies in the arena, index structures included: optimize(5), the demotion of the chi2 > 5.991
// edges, optimize(10) without the robust kernel, the outlier rule.  Both local-BA entry points run it; d_chi2 and d_outlier are device
// addresses, the caller's arrays or slots of the arena.  *out: iterations and trials of both rounds, lambda of the second,
// chi_initial of the first.
int lba_rounds(const LmPlan &q, const Arena &a, double *rb, hipStream_t s, BaCam cam, double *d_chi2, uint8_t *d_outlier, LmOutcome *out)
{
    orbba_lm_options o1 = {}, o2 = {};
    o1.max_iterations = 5;               // optimizer.optimize(5), :893
    o2.max_iterations = 10;              // :909
    LmOutcome out1 = {};
    if (int rc = lm_loop(q, a, rb, s, cam, nullptr, lm_knobs(&o1), &out1)) return rc;
    hipLaunchKernelGGL(k_lba_demote, dim3(q.EB), dim3(256), 0, s, q.NE, a.D(q.ochi), a.at(q.oact), a.D(q.ochi1));   // :899-902
    cam.delta = 0.0;                     // setRobustKernel(nullptr), :904
    if (int rc = lm_loop(q, a, rb, s, cam, a.at(q.oact), lm_knobs(&o2), out)) return rc;
    // An edge demoted to level 1 at :899-902 is not part of optimize(10)'s active set: g2o never calls computeError()
    // on it again, so e->chi2() at :919 still evaluates the error vector of the first round -- above 5.991 by
    // construction -- and the observation is always erased, whatever its residual at the final estimate would be
    // (poseOptimize has an explicit computeError() for exactly that reason, Optimize.cpp:510; this loop has none).
    hipLaunchKernelGGL(k_lba_outliers, dim3(q.EB), dim3(256), 0, s, q.NE, a.D(q.ochi), a.at(q.oact), a.D(q.ochi1), d_chi2, d_outlier); // :917-921
    ORB_TRY(hipGetLastError());
    out->iterations += out1.iterations;
    out->trials += out1.trials;
    out->chi_initial = out1.chi_initial;
    return ORBX_OK;
}
} // namespace

// The optimisation part of Optimize::localBundleAdjustment (Optimize.cpp:892-922): checks, host index, one copy up, both rounds, one down
extern "C" int orbba_local_bundle_adjustment(const orbba_problem *p, orbba_lm_result *r, uint8_t *outlier, int device)
{
    if (!p || !r) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (BaVerdict v = ba_check_problem(p, 1); v.code) return ba_refuse(v);
    BaIndex ix;
    if (BaVerdict v = ba_build_index(p, true, &ix); v.code) return ba_refuse(v);
    if (int rc = orb_need_device(&device)) return rc;
    ORB_TRY(hipSetDevice(device));
    const LmPlan q = lm_plan(p->n_poses, p->n_points, p->n_edges, (int)ix.free_pose.size());
    Lease<BaWork> lease(g_work);
    ORB_TRY(lease.acquire(device));
    BaWork *w = lease.w;
    ORB_TRY(w->need(q.bytes, q.in_end));
    hipStream_t s = w->stream;
    const Arena a = {w->d.as<uint8_t>()}, h = {w->h.as<uint8_t>()};
    if (int rc = lm_upload(q, a, h, p, nullptr, ix, s)) return rc;
    ORB_TRY(hipEventRecord(w->e0, s));
    LmOutcome out = {};
    if (int rc = lba_rounds(q, a, h.D(q.orb), s, make_cam(p), a.D(q.ochio), a.at(q.oout), &out)) return rc;
    ORB_TRY(hipEventRecord(w->e1, s));
    if (int rc = lm_download(q, a, h, r->chi2 ? q.ochio : outlier ? q.oout : q.orb, s, w, out, r)) return rc;
    h.get(outlier, q.oout, (size_t)q.NE);
    return ORBX_OK;
}

extern "C" int orbba_local_bundle_adjustment_device(const orbba_problem *p, orbba_lm_result *r, uint8_t *d_outlier, void *stream)
{
    if (!p || !r) return orbx_set_error(ORBX_E_ARG, "null argument");
    const int NP = p->n_poses, NL = p->n_points, NE = p->n_edges;
    if (!ba_sizes_ok(p, 1)) return orbx_set_error(ORBX_E_ARG, "bad sizes");
    if (!ba_arrays_ok(p) || !r->pose_R || !r->pose_t || !r->points || !r->chi2 || !d_outlier)
        return orbx_set_error(ORBX_E_ARG, "null array (every pointer is device memory here, chi2 and outlier included)");
    // the number of free poses is not known yet: the arena is sized for every pose free
    if ((size_t)NP * NL > (size_t)1 << 28) return orbx_set_error(ORBX_E_UNSUPPORTED, "poses x points table too large");
    int device = -1;
    if (int rc = orb_need_device(&device)) return rc;
    hipStream_t s = (hipStream_t)stream; // NULL is stream 0 itself (include/orbx.h, "Streams")
    const LmPlan q0 = lm_plan(NP, NL, NE, NP);
    Lease<BaWork> lease(g_work);
    ORB_TRY(lease.acquire(device));
    lease.stream = s;                    // the call runs on the caller's stream: that one is waited on before the arena goes back
    BaWork *w = lease.w;                 // its arena, staging block and events
    ORB_TRY(w->need(q0.bytes, 8 * (size_t)q0.RB_N + 256));
    const Arena a = {w->d.as<uint8_t>()};
    double *const rb = w->h.as<double>();
    auto copy = [&](size_t off, const void *src, size_t bytes) { return hipMemcpyAsync(a.at(off), src, bytes, hipMemcpyDeviceToDevice, s); };
    ORB_TRY(copy(q0.oR, p->pose_R, 72 * (size_t)NP)); ORB_TRY(copy(q0.ot, p->pose_t, 24 * (size_t)NP)); ORB_TRY(copy(q0.oP, p->points, 24 * (size_t)NL));
    ORB_TRY(copy(q0.ofix, p->pose_fixed, NP)); ORB_TRY(copy(q0.oep, p->edge_pose, 4 * (size_t)NE)); ORB_TRY(copy(q0.oel, p->edge_point, 4 * (size_t)NE));
    ORB_TRY(copy(q0.oz, p->edge_z, 16 * (size_t)NE)); ORB_TRY(copy(q0.ow, p->edge_inv_sigma2, 8 * (size_t)NE));
    // ---- index structures and the host form's checks, on the device
    ORB_TRY(hipMemsetAsync(a.at(q0.opo), 0, 4 * (size_t)(NP + 1), s));
    ORB_TRY(hipMemsetAsync(a.at(q0.oix), 0, 64, s));
    const int EB = q0.EB;
    const int fill_cap = (int)std::min<size_t>((size_t)NP * NL, (size_t)1 << 28);
    hipLaunchKernelGGL(k_lmi_count, dim3(EB), dim3(256), 0, s, NP, NL, NE, a.I(q0.oep), a.I(q0.oel), a.I(q0.opo), a.I(q0.oix));
    hipLaunchKernelGGL(k_lmi_poses, dim3(1), dim3(1024), 0, s, NP, a.at(q0.ofix), a.I(q0.opo), a.I(q0.ofree), a.I(q0.oslot), a.I(q0.oix));
    hipLaunchKernelGGL(k_lmi_place, dim3(NP), dim3(256), 0, s, NE, a.I(q0.oep), a.I(q0.opo), a.I(q0.ope));
    hipLaunchKernelGGL(k_lmi_fill, dim3(std::min((fill_cap + 255) / 256, 1024)), dim3(256), 0, s, NL, a.I(q0.oix), fill_cap, a.I(q0.oeo));
    hipLaunchKernelGGL(k_lmi_cells, dim3(EB), dim3(256), 0, s, NP, NL, NE, a.I(q0.oep), a.I(q0.oel), a.I(q0.oslot), a.I(q0.oeo), a.I(q0.oix));
    hipLaunchKernelGGL(k_lmi_points, dim3((NL + 256) / 256), dim3(256), 0, s, NL, NE, a.I(q0.oel), a.I(q0.olo));
    ORB_TRY(hipGetLastError());
    // the first read-back: the checks' verdict and the number of free poses, which sizes the reduced system
    int *const ix = reinterpret_cast<int *>(rb);
    ORB_TRY(hipMemcpyAsync(ix, a.at(q0.oix), 64, hipMemcpyDeviceToHost, s));
    ORB_TRY(hipStreamSynchronize(s));
    const int flag = ix[LMI_FLAG], NF = ix[LMI_NF];
    if (flag & LMI_E_RANGE) return orbx_set_error(ORBX_E_ARG, "edge index out of range");
    if (flag & LMI_E_ORDER) return orbx_set_error(ORBX_E_ARG, "edges must be grouped by point");
    if (flag & LMI_E_ALL_FIXED || NF < 1 || NF > NP) return orbx_set_error(ORBX_E_ARG, "every pose is fixed: nothing to optimise");
    if (flag & LMI_E_TWICE) return orbx_set_error(ORBX_E_ARG, "a point is observed twice by the same key frame");
    const LmPlan q = lm_plan(NP, NL, NE, NF);                      // the same offsets up to edge_of; the scratch behind it is smaller
    ORB_TRY(hipEventRecord(w->e0, s));
    LmOutcome out = {};
    if (int rc = lba_rounds(q, a, rb, s, make_cam(p), r->chi2, d_outlier, &out)) return rc;
    ORB_TRY(hipMemcpyAsync(r->pose_R, a.at(q.oR), 72 * (size_t)NP, hipMemcpyDeviceToDevice, s));
    ORB_TRY(hipMemcpyAsync(r->pose_t, a.at(q.ot), 24 * (size_t)NP, hipMemcpyDeviceToDevice, s));
    ORB_TRY(hipMemcpyAsync(r->points, a.at(q.oP), 24 * (size_t)NL, hipMemcpyDeviceToDevice, s));
    ORB_TRY(hipEventRecord(w->e1, s));
    ORB_TRY(hipMemcpyAsync(rb, a.at(q.orb), 8 * (size_t)q.RB_N, hipMemcpyDeviceToHost, s));
    ORB_TRY(hipStreamSynchronize(s));    // the arena goes back to the pool: nothing of this call may still be running
    return lm_report(q, rb, w, out, r);
}

// =====================================================================================================================
// Optimize::poseOptimize (modules/Backend/Optimize.cpp:444-545) for a batch of frames: one workgroup runs one frame's
// whole procedure -- four rounds of (restart from the initial pose, up to ten Levenberg-Marquardt iterations on the
// inlier edges with the Huber kernel, re-classification of every edge at chi2 <= 5.991) -- without leaving the kernel.
// The 6x6 system is reduced over the edges in a fixed order (strided per thread, wave shuffles, four partials) and then
// solved redundantly by every lane, so all control flow is uniform across the workgroup.
// =====================================================================================================================
__device__ __forceinline__ void se3_exp_apply(const double *u, double *R, double *t)
{
    const double wx = u[0], wy = u[1], wz = u[2];
    const double th = sqrt(wx * wx + wy * wy + wz * wz);
    const double K[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double K2[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) K2[3 * r + c] = K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c] + K[3 * r + 2] * K[6 + c];
    double ra, rb, va, vb;
    if (th < 0.00001) { ra = 1.0; rb = 0.5; va = 0.5; vb = 1.0 / 6.0; }
    else {
        ra = sin(th) / th; rb = (1.0 - cos(th)) / (th * th);
        va = rb; vb = (th - sin(th)) / (th * th * th);
    }
    double E[9], V[9], Rn[9], tn[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double I = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        E[k] = I + ra * K[k] + rb * K2[k];
        V[k] = I + va * K[k] + vb * K2[k];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Rn[3 * r + c] = E[3 * r] * R[c] + E[3 * r + 1] * R[3 + c] + E[3 * r + 2] * R[6 + c];
        tn[r] = (E[3 * r] * t[0] + E[3 * r + 1] * t[1] + E[3 * r + 2] * t[2]) + (V[3 * r] * u[3] + V[3 * r + 1] * u[4] + V[3 * r + 2] * u[5]);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = tn[k];
}

// all 256 threads get the sum of v[0..K) over the workgroup, summed in a fixed order
template <int K> __device__ __forceinline__ void block_sum_vals(double *v, double (*red)[28])
{
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double x = v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
        v[k] = x;
    }
    __syncthreads(); // the previous round's readers are done
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

// solves (H + lam I) x = b for the symmetric 6x6 H given by its 21 upper-triangular entries; false if not positive definite
__device__ __forceinline__ bool solve6(const double *h21, double lam, const double *b, double *x)
{
    double L[36];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { L[6 * j + i] = h21[k] + (i == j ? lam : 0.0); ++k; } // lower triangle
    for (int c = 0; c < 6; ++c) {
        double d = L[6 * c + c];
        for (int m = 0; m < c; ++m) d -= L[6 * c + m] * L[6 * c + m];
        if (!(d > 0.0)) return false;
        d = sqrt(d);
        L[6 * c + c] = d;
        for (int r = c + 1; r < 6; ++r) {
            double v = L[6 * r + c];
            for (int m = 0; m < c; ++m) v -= L[6 * r + m] * L[6 * c + m];
            L[6 * r + c] = v / d;
        }
    }
    double y[6];
    for (int r = 0; r < 6; ++r) {
        double v = b[r];
        for (int m = 0; m < r; ++m) v -= L[6 * r + m] * y[m];
        y[r] = v / L[6 * r + r];
    }
    for (int r = 5; r >= 0; --r) {
        double v = y[r];
        for (int m = r + 1; m < 6; ++m) v -= L[6 * m + r] * x[m];
        x[r] = v / L[6 * r + r];
    }
    return true;
}

__global__ __launch_bounds__(256) void k_pose_optimize(BaCam cam, int rounds, int iterations, int cap, const int *__restrict__ edge_off,
                                                       const double *__restrict__ R0, const double *__restrict__ t0,
                                                       const double *__restrict__ Pw, const double *__restrict__ z,
                                                       const double *__restrict__ w, double *__restrict__ R_out,
                                                       double *__restrict__ t_out, uint8_t *__restrict__ inlier,
                                                       int *__restrict__ n_inliers, double *__restrict__ chi2_out)
{
    __shared__ double red[4][28];
    // A frame's edges (map point, measurement, weight, inlier flag: 49 bytes each) are read in every one of up to 4 x 10 x 2 passes:
    // up to `cap` of them are staged in LDS once (structure of arrays), so a pass costs LDS latency instead of an L2 round trip per
    // operand.  Same operations in the same order as from global memory (a frame with more edges keeps reading it from there).
    extern __shared__ __align__(16) double sm[];
    const int f = blockIdx.x, tid = threadIdx.x, e0 = edge_off[f], n = edge_off[f + 1] - e0;
    const bool staged = n <= cap;
    double *const sPx = sm, *const sPy = sPx + cap, *const sPz = sPy + cap, *const szu = sPz + cap, *const szv = szu + cap, *const sww = szv + cap;
    uint8_t *const sin_ = reinterpret_cast<uint8_t *>(sww + cap);
    double Ri[9], ti[3], R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Ri[k] = R0[(size_t)f * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = ti[k] = t0[(size_t)f * 3 + k];
    for (int e = tid; e < n; e += 256) {
        inlier[e0 + e] = 1;
        if (staged) {
            sPx[e] = Pw[(size_t)(e0 + e) * 3]; sPy[e] = Pw[(size_t)(e0 + e) * 3 + 1]; sPz[e] = Pw[(size_t)(e0 + e) * 3 + 2];
            szu[e] = z[(size_t)(e0 + e) * 2]; szv[e] = z[(size_t)(e0 + e) * 2 + 1]; sww[e] = w[e0 + e];
            sin_[e] = 1;
        }
    }
    __syncthreads();
    auto is_in = [&](int e) -> bool { return staged ? sin_[e] != 0 : inlier[e0 + e] != 0; };
    auto weight = [&](int e) -> double { return staged ? sww[e] : w[e0 + e]; };
    const double d2 = cam.delta * cam.delta;

    // residual of edge e at pose (R, t); returns chi2, optionally the pieces needed for the Jacobian
    auto edge_chi = [&](int e, const double *Rc, const double *tc, double *ex, double *ey, double *Pc) -> double {
        double P[3], zu, zv;
        if (staged) { P[0] = sPx[e]; P[1] = sPy[e]; P[2] = sPz[e]; zu = szu[e]; zv = szv[e]; }
        else {
            const double *Pg = Pw + (size_t)(e0 + e) * 3;
            P[0] = Pg[0]; P[1] = Pg[1]; P[2] = Pg[2]; zu = z[(size_t)(e0 + e) * 2]; zv = z[(size_t)(e0 + e) * 2 + 1];
        }
        const double X = Rc[0] * P[0] + Rc[1] * P[1] + Rc[2] * P[2] + tc[0];
        const double Y = Rc[3] * P[0] + Rc[4] * P[1] + Rc[5] * P[2] + tc[1];
        const double Z = Rc[6] * P[0] + Rc[7] * P[1] + Rc[8] * P[2] + tc[2];
        double u, v;
        ba_project(cam, X, Y, Z, &u, &v);
        *ex = zu - u;
        *ey = zv - v;
        Pc[0] = X; Pc[1] = Y; Pc[2] = Z;
        return weight(e) * (*ex * *ex + *ey * *ey);
    };
    auto robust_sum = [&](const double *Rc, const double *tc) -> double { // activeRobustChi2
        double s[1] = {0.0};
        for (int e = tid; e < n; e += 256) {
            if (!is_in(e)) continue;
            double ex, ey, Pc[3];
            double c = edge_chi(e, Rc, tc, &ex, &ey, Pc);
            if (cam.delta > 0.0 && c > d2) c = 2.0 * cam.delta * sqrt(c) - d2;
            s[0] += c;
        }
        block_sum_vals<1>(s, red);
        return s[0];
    };

    if (n >= 3) { // fewer than three correspondences: nothing is done (:491)
        for (int round = 0; round < rounds; ++round) {
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = Ri[k]; // vPose->setEstimate(Tcw) (:497)
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = ti[k];
            double cnt[1] = {0.0};
            for (int e = tid; e < n; e += 256) cnt[0] += is_in(e) ? 1.0 : 0.0;
            block_sum_vals<1>(cnt, red);
            double lam = 0.0, ni = 2.0;
            if (cnt[0] > 0.0) {
                for (int it = 0; it < iterations; ++it) {
                    // computeActiveErrors + buildSystem
                    double acc[28];
#pragma unroll
                    for (int k = 0; k < 28; ++k) acc[k] = 0.0;
                    for (int e = tid; e < n; e += 256) {
                        if (!is_in(e)) continue;
                        double ex, ey, Pc[3];
                        const double c = edge_chi(e, R, t, &ex, &ey, Pc);
                        double rw = 1.0, rc = c;
                        if (cam.delta > 0.0 && c > d2) { rw = cam.delta / sqrt(c); rc = 2.0 * cam.delta * sqrt(c) - d2; }
                        const double W = rw * weight(e), X = Pc[0], Y = Pc[1], Z = Pc[2];
                        double Jp[6];
                        ba_proj_jacobian(cam, X, Y, Z, Jp);
                        double Jq[12];
#pragma unroll
                        for (int r = 0; r < 2; ++r) {
                            const double a = Jp[3 * r], b = Jp[3 * r + 1], cc = Jp[3 * r + 2];
                            Jq[6 * r + 0] = b * Z - cc * Y;
                            Jq[6 * r + 1] = -a * Z + cc * X;
                            Jq[6 * r + 2] = a * Y - b * X;
                            Jq[6 * r + 3] = -a; Jq[6 * r + 4] = -b; Jq[6 * r + 5] = -cc;
                        }
                        int k = 0;
#pragma unroll
                        for (int i = 0; i < 6; ++i)
#pragma unroll
                            for (int j = i; j < 6; ++j) acc[k++] += W * (Jq[i] * Jq[j] + Jq[6 + i] * Jq[6 + j]);
#pragma unroll
                        for (int i = 0; i < 6; ++i) acc[21 + i] += -W * (Jq[i] * ex + Jq[6 + i] * ey);
                        acc[27] += rc;
                    }
                    block_sum_vals<28>(acc, red);
                    double current = acc[27];
                    const double *h21 = acc, *b = acc + 21;
                    if (it == 0) { // computeLambdaInit
                        double mx = 0.0;
                        int k = 0;
                        for (int i = 0; i < 6; ++i) { mx = fmax(mx, fabs(h21[k])); k += 6 - i; }
                        lam = 1e-5 * mx;
                        ni = 2.0;
                    }
                    // g2o's trial policy, by every lane: THE ONE COPY that is not orb_lm_policy.h's.  With the header's calls the kernel
                    // kept its registers and every byte of its results and took 1.5 to 3.5 % longer ("The policy, written once")
                    double rho = 0.0;
                    int qmax = 0;
                    do {
                        double Rb[9], tb[3], x[6];
#pragma unroll
                        for (int k = 0; k < 9; ++k) Rb[k] = R[k];
#pragma unroll
                        for (int k = 0; k < 3; ++k) tb[k] = t[k];
                        const bool ok2 = solve6(h21, lam, b, x);
                        if (!ok2)
#pragma unroll
                            for (int k = 0; k < 6; ++k) x[k] = 0.0;
                        se3_exp_apply(x, R, t);
                        double temp = robust_sum(R, t);
                        if (!ok2) temp = 1.7976931348623157e308;
                        double scale = 0.0;
#pragma unroll
                        for (int k = 0; k < 6; ++k) scale += x[k] * (lam * x[k] + b[k]);
                        scale += 1e-3;
                        rho = (current - temp) / scale;
                        if (rho > 0 && isfinite(temp)) {
                            double alpha = 1.0 - (2 * rho - 1) * (2 * rho - 1) * (2 * rho - 1);
                            alpha = fmin(alpha, 2.0 / 3.0);
                            lam *= fmax(1.0 / 3.0, alpha);
                            ni = 2.0;
                            current = temp;
                        } else {
                            lam *= ni;
                            ni *= 2;
#pragma unroll
                            for (int k = 0; k < 9; ++k) R[k] = Rb[k];
#pragma unroll
                            for (int k = 0; k < 3; ++k) t[k] = tb[k];
                            if (!isfinite(lam)) break;
                        }
                        ++qmax;
                    } while (rho < 0 && qmax < 10);
                    if (qmax == 10 || rho == 0 || !isfinite(lam)) break;
                }
            }
            // :503-516 -- every edge is re-evaluated at the round's pose
            __syncthreads();
            for (int e = tid; e < n; e += 256) {
                double ex, ey, Pc[3];
                const double c = edge_chi(e, R, t, &ex, &ey, Pc);
                inlier[e0 + e] = !(c > 5.991);
                if (staged) sin_[e] = !(c > 5.991);
            }
            __syncthreads();
        }
    }
    double cnt[1] = {0.0};
    for (int e = tid; e < n; e += 256) {
        double ex, ey, Pc[3];
        const double c = edge_chi(e, R, t, &ex, &ey, Pc);
        if (chi2_out) chi2_out[e0 + e] = c;
        cnt[0] += (n >= 3 && is_in(e)) ? 1.0 : 0.0;
    }
    block_sum_vals<1>(cnt, red);
    if (tid == 0) {
        n_inliers[f] = (int)cnt[0];
#pragma unroll
        for (int k = 0; k < 9; ++k) R_out[(size_t)f * 9 + k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t_out[(size_t)f * 3 + k] = t[k];
    }
}

// edges of a frame staged in LDS by k_pose_optimize (49 bytes each; ORBBA_VAR_POSE_LDS = 0: never, the parity twin)
static int pose_lds_cap() { return g_ba_pose_lds.load(); }
static size_t pose_lds_bytes(int cap) { return ((size_t)cap * 49 + 15) / 16 * 16; }
static hipError_t pose_lds_configure(int cap)
{
    return orbx_lds_opt_in(reinterpret_cast<const void *>(k_pose_optimize), pose_lds_bytes(cap)); // per device, largest size wins
}
extern "C" int orbba_pose_optimize_batch(const orbba_pose_problem *p, orbba_pose_result *r, int device)
{
    if (!p || !r) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (p->n_frames < 1 || !p->edge_off || !p->pose_R || !p->pose_t) return orbx_set_error(ORBX_E_ARG, "bad sizes / null arrays");
    const int B = p->n_frames, NE = p->edge_off[B];
    for (int f = 0; f < B; ++f)
        if (p->edge_off[f + 1] < p->edge_off[f] || p->edge_off[0] != 0)
            return orbx_set_error(ORBX_E_ARG, "edge offsets must start at 0 and be non-decreasing");
    if (NE > 0 && (!p->points || !p->edge_z || !p->edge_inv_sigma2)) return orbx_set_error(ORBX_E_ARG, "null edge array");
    if (!r->pose_R || !r->pose_t || !r->n_inliers || (NE > 0 && !r->inlier)) return orbx_set_error(ORBX_E_ARG, "null output array");
    if (int rc = orb_need_device(&device)) return rc;
    ORB_TRY(hipSetDevice(device));
    // arena: [inputs, one copy up][results, one copy down]
    Layout L;
    const size_t ooff = L.add(4 * (size_t)(B + 1)), oR0 = L.add(72 * (size_t)B), ot0 = L.add(24 * (size_t)B), oP = L.add(24 * (size_t)NE),
                 oz = L.add(16 * (size_t)NE), ow = L.add(8 * (size_t)NE);
    const size_t in_bytes = L.n;
    const size_t oR = L.add(72 * (size_t)B), ot = L.add(24 * (size_t)B), oni = L.add(4 * (size_t)B), oin = L.add(NE);
    const size_t out_small_end = L.n;
    const size_t ochi = L.add(8 * (size_t)NE);
    const size_t out_end = (NE && r->chi2) ? L.n : out_small_end;
    Lease<BaWork> lease(g_work);
    ORB_TRY(lease.acquire(device));
    BaWork *w = lease.w;
    ORB_TRY(w->need(L.n, std::max(in_bytes, out_end - in_bytes)));
    hipStream_t s = w->stream;
    const Arena a = {w->d.as<uint8_t>()}, h = {w->h.as<uint8_t>()};
    h.put(ooff, p->edge_off, 4 * (size_t)(B + 1)); h.put(oR0, p->pose_R, 72 * (size_t)B); h.put(ot0, p->pose_t, 24 * (size_t)B);
    h.put(oP, p->points, 24 * (size_t)NE); h.put(oz, p->edge_z, 16 * (size_t)NE); h.put(ow, p->edge_inv_sigma2, 8 * (size_t)NE);
    ORB_TRY(hipMemcpyAsync(a.base, h.base, in_bytes, hipMemcpyHostToDevice, s));
    const BaCam cam = make_cam(p);
    ORB_TRY(hipEventRecord(w->e0, s));
    int max_n = 0;
    for (int f = 0; f < B; ++f) max_n = std::max(max_n, p->edge_off[f + 1] - p->edge_off[f]);
    const int cap = std::min(pose_lds_cap(), max_n); // (no more LDS than the largest frame needs: more workgroups per CU for a big batch)
    ORB_TRY(pose_lds_configure(cap));
    hipLaunchKernelGGL(k_pose_optimize, dim3(B), dim3(256), pose_lds_bytes(cap), s, cam, p->rounds > 0 ? p->rounds : 4,
                       p->iterations > 0 ? p->iterations : 10, cap, a.I(ooff), a.D(oR0), a.D(ot0), a.D(oP), a.D(oz), a.D(ow), a.D(oR), a.D(ot),
                       a.at(oin), a.I(oni), a.D(ochi));
    ORB_TRY(hipEventRecord(w->e1, s));
    ORB_TRY(hipGetLastError());
    ORB_TRY(hipMemcpyAsync(h.base, a.at(in_bytes), out_end - in_bytes, hipMemcpyDeviceToHost, s));
    ORB_TRY(hipStreamSynchronize(s));
    float ms = 0;
    ORB_TRY(hipEventElapsedTime(&ms, w->e0, w->e1));
    r->kernel_ms = ms;
    // a result's place in the staging block is its place in the arena behind the inputs
    h.get(r->pose_R, oR - in_bytes, 72 * (size_t)B); h.get(r->pose_t, ot - in_bytes, 24 * (size_t)B); h.get(r->n_inliers, oni - in_bytes, 4 * (size_t)B);
    h.get(r->inlier, oin - in_bytes, NE); h.get(r->chi2, ochi - in_bytes, 8 * (size_t)NE);
    return ORBX_OK;
}

// ---------------------------------------------------------------------------------------------
// The tracking chain without a host hop (Tracking.cpp:289-336): the matched map points of a device-resident frame record
// (orbm_search_by_projection_*_device wrote frame_mp) become the edges of poseOptimize (Optimize.cpp:468-490) on the
// device, and orbba_pose_optimize_batch_device runs k_pose_optimize on device arrays.
// ---------------------------------------------------------------------------------------------
// edges in key-point order (:470): for key point i with frame_mp[i] in [0, nq): the map point's position, kp.pt, 1 / size^2
__global__ __launch_bounds__(1024) void k_pose_edges(int n2, int nq, const int32_t *__restrict__ frame_mp,
                                                     const orbx_kp *__restrict__ kps, const float *__restrict__ q_points,
                                                     int32_t *__restrict__ edge_off, double *__restrict__ points,
                                                     double *__restrict__ z, double *__restrict__ w, int32_t *__restrict__ edge_kp)
{
    __shared__ int s_wave[16], s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n2; i0 += 1024) {
        const int i = i0 + tid;
        const int q = i < n2 ? frame_mp[i] : -1;
        const bool on = q >= 0 && q < nq;
        const unsigned long long mk = __ballot(on);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
        if (lane == 0) s_wave[wv] = (int)__popcll(mk);
        __syncthreads();
        int before = s_base;
        for (int k = 0; k < wv; ++k) before += s_wave[k];
        if (on) {
            const int e = before + rank;
            const orbx_kp kp = kps[i];
            points[3 * e] = (double)q_points[3 * q]; points[3 * e + 1] = (double)q_points[3 * q + 1]; points[3 * e + 2] = (double)q_points[3 * q + 2];
            z[2 * e] = (double)kp.x; z[2 * e + 1] = (double)kp.y;           // setMeasurement({kp.pt.x, kp.pt.y}) (:478)
            w[e] = (double)__fdiv_rn(__fdiv_rn(1.f, kp.size), kp.size);     // invSigma2 = 1.f / kp.size / kp.size (:479)
            if (edge_kp) edge_kp[e] = i;
        }
        __syncthreads();
        if (tid == 0) { int t = 0; for (int k = 0; k < 16; ++k) t += s_wave[k]; s_base += t; }
        __syncthreads();
    }
    if (tid == 0) { edge_off[0] = 0; edge_off[1] = s_base; }
}
extern "C" int orbba_pose_edges_device(int n2, int nq, const int32_t *d_frame_mp, const void *d_kps, const float *d_q_points,
                                       int32_t *d_edge_off, double *d_points, double *d_edge_z, double *d_edge_inv_sigma2,
                                       int32_t *d_edge_kp, void *stream)
{
    if (n2 < 0 || nq < 0 || !d_frame_mp || !d_kps || !d_q_points || !d_edge_off || !d_points || !d_edge_z || !d_edge_inv_sigma2)
        return orbx_set_error(ORBX_E_ARG, "bad argument");
    if (int rc = orb_need_device()) return rc;
    hipLaunchKernelGGL(k_pose_edges, dim3(1), dim3(1024), 0, (hipStream_t)stream, n2, nq, d_frame_mp, (const orbx_kp *)d_kps,
                       d_q_points, d_edge_off, d_points, d_edge_z, d_edge_inv_sigma2, d_edge_kp);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
// the outliers of poseOptimize leave the frame (Optimize.cpp:531-538): frame_mp[vecIndices[e]] = nullptr
__global__ __launch_bounds__(256) void k_pose_drop_outliers(int n2, const int32_t *__restrict__ edge_off, const int32_t *__restrict__ edge_kp,
                                                            const uint8_t *__restrict__ inlier, int32_t *__restrict__ frame_mp)
{
    const int ne = min(edge_off[1], n2); // (one edge per key point at most: the arrays hold n2 entries)
    for (int e = blockIdx.x * 256 + threadIdx.x; e < ne; e += gridDim.x * 256) {
        const int i = edge_kp[e];
        if (!inlier[e] && i >= 0 && i < n2) frame_mp[i] = -1;
    }
}
extern "C" int orbba_pose_drop_outliers_device(int n2, const int32_t *d_edge_off, const int32_t *d_edge_kp, const uint8_t *d_inlier,
                                               int32_t *d_frame_mp, void *stream)
{
    if (n2 < 0 || !d_edge_off || !d_edge_kp || !d_inlier || !d_frame_mp) return orbx_set_error(ORBX_E_ARG, "bad argument");
    if (int rc = orb_need_device()) return rc;
    if (n2 == 0) return ORBX_OK;
    // the edge count is on the device: a grid for n2 edges, at most 16 workgroups (the stride loop serves the rest)
    hipLaunchKernelGGL(k_pose_drop_outliers, dim3(std::min((n2 + 255) / 256, 16)), dim3(256), 0, (hipStream_t)stream, n2, d_edge_off,
                       d_edge_kp, d_inlier, d_frame_mp);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
extern "C" int orbba_pose_optimize_batch_device(const orbba_pose_problem *p, orbba_pose_result *r, void *stream)
{
    if (!p || !r) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (p->n_frames < 1 || !p->edge_off || !p->pose_R || !p->pose_t || !p->points || !p->edge_z || !p->edge_inv_sigma2 ||
        !r->pose_R || !r->pose_t || !r->n_inliers || !r->inlier || !r->chi2)
        return orbx_set_error(ORBX_E_ARG, "null array (every pointer is device memory here, chi2 included)");
    if (int rc = orb_need_device()) return rc;
    const BaCam cam = make_cam(p);
    const int cap = pose_lds_cap(); // (the edge counts are on the device: the full capacity, one workgroup per CU)
    ORB_TRY(pose_lds_configure(cap));
    hipLaunchKernelGGL(k_pose_optimize, dim3(p->n_frames), dim3(256), pose_lds_bytes(cap), (hipStream_t)stream, cam, p->rounds > 0 ? p->rounds : 4,
                       p->iterations > 0 ? p->iterations : 10, cap, p->edge_off, p->pose_R, p->pose_t, p->points, p->edge_z,
                       p->edge_inv_sigma2, r->pose_R, r->pose_t, r->inlier, r->n_inliers, r->chi2);
    ORB_TRY(hipGetLastError());
    r->kernel_ms = 0.f;
    return ORBX_OK;
}
