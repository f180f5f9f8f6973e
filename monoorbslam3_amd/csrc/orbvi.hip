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
#include "orbvi_stages.h"

#pragma clang fp contract(off)

static_assert(sizeof(orbvi_camera) == 72, "orbvi.h fixes this layout");

namespace {

// The bodies of both kernels are orbvi_stages.h's, which k_vi_pose_loop (orbvi_loop.hip) runs as well: a kernel here owns its LDS, its
// launch shape and the flush of its counters.  vi_linearize_group is, in the order k_vi_linearize had them: pose_rcw(), pose_tbc(),
// pose_tcw(), dsum3(), ba_project(), huber(), ba_proj_jacobian(), pose_jacobian(), quad_accumulate(), block_sums_put(), block_add(),
// block_sums_get(), quad_scatter(); vi_solve_assemble is dof_fixed() and edge_valid() around the blocks' copies.
__global__ __launch_bounds__(VI_T) void k_vi_linearize(const ViArgs a)
{
    __shared__ double s_part[VI_WAVES][VI_SUMS];
    __shared__ double s_pose[P_WORDS];
    __shared__ int s_cnt[8];
    __shared__ int s_i[I_WORDS];
    vi_linearize_group<1>(a, a.mode, blockIdx.x, threadIdx.x, s_part, s_pose, s_cnt, s_i);
    flush_counts(s_cnt, a.result);
}

constexpr int SV_T = 256;

__global__ __launch_bounds__(SV_T) void k_vi_solve(int n, const uint8_t *__restrict__ fixed, const orbi_edge *__restrict__ edges, int n_edges, int cap,
                                                   const double *__restrict__ H_diag, const double *__restrict__ H_off, const double *__restrict__ b,
                                                   const double *__restrict__ lambda, double *__restrict__ dx, double *__restrict__ out,
                                                   int32_t *__restrict__ result)
{
    __shared__ double s_A[SV_N * SV_LD];
    __shared__ double s_v[SV_N];
    __shared__ int s_fix[SV_N];
    __shared__ int s_cnt[8];
    vi_solve_assemble<SV_T>(threadIdx.x, n, fixed, edges, n_edges, cap, H_diag, H_off, s_A, s_fix, s_cnt);
    if (threadIdx.x >= 64) return;                // one wave from here on, a lane per row: no workgroup barrier below
    const int i = threadIdx.x, N = 15 * n;
    const double h_max = vi_solve_largest(N, s_A, s_fix, i);
    const bool refused = vi_solve_wave(N, b, *lambda, dx, out, s_A, s_v, s_fix, i);
    if (i == 0) out[1] = h_max;
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
