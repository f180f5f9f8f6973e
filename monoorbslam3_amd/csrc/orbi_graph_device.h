// The layer the kernels on the inertial graph share (the inertial factors, the visual edges, the marginalised window): the ordered three-term
// sum, the fixed-dof rule, the validity of an orbi_edge, the duplicate scan over a job list, EdgeMono's pose path on a VertexPose -- the pose derived from (R_wb, t_wb) and
// orbi_calib, the pose Jacobian, the Huber kernel, the quadratic form and its scatter into a state's blocks -- and what the host side of
// the two *_linearize_device entry points has in common.  Every operation order here is one the public headers fix and the numpy models
// of tests/ hold to the bit: a correction is made here, once.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/orbvi.h"
#include "../../include/orbx.h"
#include "orb_host.h"
#include "orb_math.h"
#include "orbba_camera.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ double dsum3(double p0, double p1, double p2) { return (p0 + p1) + p2; }
// dof 0..5 of a state is its pose (ORBI_FIX_POSE), then three each of velocity, gyro bias and accelerometer bias
__device__ __forceinline__ bool dof_fixed(int fixed, int dof) { return (fixed >> (dof < 6 ? 0 : dof / 3 - 1)) & 1; }
// an inertial edge that takes part: two different states of the n and a record of the bank
__device__ __forceinline__ bool edge_valid(int i, int j, int rec, int n, int cap)
{
    return !(i < 0 || i >= n || j < 0 || j >= n || i == j || rec < 0 || rec >= cap);
}
// whether one of the jobs [0, job) of a list of `stride` ints names `value` in `field` (or `value2` in `field2`, where that is given),
// dropped or not: the later job is the duplicate
__device__ __forceinline__ bool job_named_before(const int32_t *jobs, int stride, int job, int field, int value, int field2 = -1, int value2 = 0)
{
    bool hit = false;
    for (int k = 0; k < job; ++k)
        if (jobs[stride * k + field] == value || (field2 >= 0 && jobs[stride * k + field2] == value2)) hit = true;
    return hit;
}

// ---- the pose an EdgeMono hangs on, entry by entry: a caller spreads the entries over threads or unrolls them ---------------------------
// entry k of R_cw = R_cb*R_wb^T, the calibration widened
__device__ __forceinline__ double pose_rcw(const orbi_calib &cal, const double *Rwb, int k)
{
    const int i = k / 3, j = k - 3 * i;
    return dsum3((double)cal.Rcb[3 * i] * Rwb[3 * j], (double)cal.Rcb[3 * i + 1] * Rwb[3 * j + 1], (double)cal.Rcb[3 * i + 2] * Rwb[3 * j + 2]);
}
// entry i of t_cw = t_cb - R_cw*t_wb
__device__ __forceinline__ double pose_tcw(const orbi_calib &cal, const double *Rcw, const double *twb, int i)
{
    return (double)cal.tcb[i] - dsum3(Rcw[3 * i] * twb[0], Rcw[3 * i + 1] * twb[1], Rcw[3 * i + 2] * twb[2]);
}
// entry i of t_bc: the float Pose::inverse of T_cb
__device__ __forceinline__ double pose_tbc(const orbi_calib &cal, int i)
{
    const float p0 = ORB_FMUL(-cal.Rcb[i], cal.tcb[0]), p1 = ORB_FMUL(-cal.Rcb[3 + i], cal.tcb[1]), p2 = ORB_FMUL(-cal.Rcb[6 + i], cal.tcb[2]);
    return (double)ORB_FADD(ORB_FADD(p0, p1), p2);
}
// linearizeOplus on the pose: J (2 x 6, row-major) = [(-Jp)*(R_cb*Hat(R_bc*Pc + t_bc)), (-Jp)*(-R_cb)]; C = R_cb widened, Pc = (X, Y, Z).
// J may be the workspace row Pc was read from
__device__ __forceinline__ void pose_jacobian(const double *C, const double *tbc, const double *Jp, double X, double Y, double Z, double *J)
{
    const double bx = dsum3(C[0] * X, C[3] * Y, C[6] * Z) + tbc[0];
    const double by = dsum3(C[1] * X, C[4] * Y, C[7] * Z) + tbc[1];
    const double bz = dsum3(C[2] * X, C[5] * Y, C[8] * Z) + tbc[2];
    const double Hb[9] = {0.0, -bz, by, bz, 0.0, -bx, -by, bx, 0.0};
    double M[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = dsum3(C[3 * (k / 3)] * Hb[k % 3], C[3 * (k / 3) + 1] * Hb[3 + k % 3], C[3 * (k / 3) + 2] * Hb[6 + k % 3]);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            J[6 * r + c] = dsum3(-Jp[3 * r] * M[c], -Jp[3 * r + 1] * M[3 + c], -Jp[3 * r + 2] * M[6 + c]);
            J[6 * r + 3 + c] = dsum3(-Jp[3 * r] * -C[c], -Jp[3 * r + 1] * -C[3 + c], -Jp[3 * r + 2] * -C[6 + c]);
        }
}
// RobustKernelHuber of a chi2: rho and the weight rho'; delta <= 0 is no kernel
__device__ __forceinline__ void huber(double chi, double delta, double &rho, double &rw)
{
    const double dsqr = delta * delta;
    rho = chi, rw = 1.0;
    if (delta > 0.0 && chi > dsqr) {
        const double sq = sqrt(chi);
        rho = (2.0 * sq) * delta - dsqr, rw = delta / sq;
    }
}
// constructQuadraticForm of one edge on the pose: J^T (w*Omega) J into acc[0..20] (the upper triangle row by row) and J^T (w*Omega) e
// into acc[21..26]; J is 2 x 6 in a workspace row
__device__ __forceinline__ void quad_accumulate(const double *Jrow, double W, double wex, double wey, double *acc)
{
    double J[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) J[k] = Jrow[k];
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c, ++k) acc[k] = acc[k] + (J[r] * (W * J[c]) + J[6 + r] * (W * J[6 + c]));
#pragma unroll
    for (int r = 0; r < 6; ++r) acc[21 + r] = acc[21 + r] + (J[r] * wex + J[6 + r] * wey);
}
// sum t of those 27 into a state's blocks: t < 21 is ADDED to H (15 x 15) at entry t of the upper triangle and at its mirror, t >= 21 is
// SUBTRACTED from b
__device__ __forceinline__ void quad_scatter(int t, double s, double *H, double *b)
{
    if (t >= 21) {
        b[t - 21] = b[t - 21] - s;
        return;
    }
    int r = 0, c = t;                              // entry t of the upper triangle, row by row
    while (c >= 6 - r) c -= 6 - r, ++r;
    c += r;
    H[15 * r + c] = H[15 * r + c] + s;
    if (r != c) H[15 * c + r] = H[15 * c + r] + s;
}

// ---- the host side the *_linearize_device entry points share -----------------------------------------------------------------------------
inline BaCam graph_camera(const orbvi_camera &camera, double huber_delta)       // delta: huber_delta
{
    return {camera.fx, camera.fy, camera.cx, camera.cy, huber_delta, camera.camera_model,
            {camera.fisheye_k[0], camera.fisheye_k[1], camera.fisheye_k[2], camera.fisheye_k[3]}};
}
// The checks in the order both entry points make them: the graph, then the caller's own arrays and counts (`own`: what is wrong with
// them, or null), then mode, kernel and camera.  The limits come behind the caller's mode-dependent checks and stay with it.
inline int graph_check_linearize(const orbi_graph &graph, const int32_t *d_result, const char *own, int mode, double huber_delta, double chi2_threshold,
                                 const orbvi_camera &camera)
{
    if (!graph.Rwb || !graph.twb || !graph.v || !graph.bg || !graph.ba || !graph.fixed || graph.n_states < 0 || !d_result)
        return orbx_set_error(ORBX_E_ARG, "null graph array or result, or a negative state count");
    if (own) return orbx_set_error(ORBX_E_ARG, own);
    if (mode < 0 || mode > 2) return orbx_set_error(ORBX_E_ARG, "mode is 0 (linearise), 1 (errors only) or 2 (classify)");
    if (!(huber_delta == huber_delta) || !(chi2_threshold == chi2_threshold)) return orbx_set_error(ORBX_E_ARG, "huber_delta or chi2_threshold is not a number");
    if (camera.camera_model != 0 && camera.camera_model != 1) return orbx_set_error(ORBX_E_ARG, "camera_model is 0 (Pinhole) or 1 (Kannala-Brandt)");
    return ORBX_OK;
}

} // namespace
