// Projection-search queries built on the device (include/orbm.h, "Projection-search queries built on the device"): a map-point
// table and a pose in device memory become the q_xy / q_radius / q_level / q_angle / q_ok arrays of the three projection searches.
//   orbm_project_frame_device     ORBMatcher.cpp:212-229, :276-348   frame / key frame -> frame
//   orbm_project_frustum_device   Tracking.cpp:403-412, Frame.cpp:129-166, ORBMatcher.cpp:360-365   local map -> frame
//   orbm_project_fuse_device      ORBMatcher.cpp:534-553             map points -> key frame (the fuse)
//
// Evaluation orders (float; no fused multiply-add: the build passes -ffp-contract=off and the pragma below repeats it here):
//   Pc_k  = ((R_k0 * x + R_k1 * y) + R_k2 * z) + t_k
//   O_w_k = -((R_0k * t_0 + R_1k * t_1) + R_2k * t_2)                 Pose.cpp:12-14
//   dist  = sqrtf((ox * ox + oy * oy) + oz * oz),  OP . Pn = (ox * nx + oy * ny) + oz * nz
//   Pinhole u = fx * (X / Z) + cx                                      Pinhole.cpp:34-38
//   Fisheye u = ((fx * theta_d) * a) / r + cx, theta_d = (((theta + k0 theta3) + k1 theta5) + k2 theta7) + k3 theta9   Fisheye.cpp:52-66
// `/` and sqrtf are the correctly rounded ones (hipcc's default for float; never __fsqrt_rn / __frcp_rn / fast-math forms here);
// logf (predictScaleLevel, MapPoint.cpp:165) and atanf (Fisheye.cpp:55) are the device library's and not correctly rounded.
//
// Shape: a call is a few thousand points, so it is bound by latency, not by throughput: ONE launch of ONE 1024-thread workgroup
// per call, a point per thread and pass.  One workgroup needs no zeroed counters in memory and no second launch: the gate counts
// are summed in LDS and d_result is WRITTEN at the end, and the frustum form's "already in the frame" mask (one bit per point) is
// built in LDS ahead of the gates behind a workgroup barrier.  The camera and the level tables are kernel arguments; the pose is
// read through uniform addresses (scalar loads), rounded to float once per thread ahead of the loop.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_host.h"
#include "orbm_internal.h"
#include "orbm_camera.h"

#pragma clang fp contract(off)

namespace {

constexpr int PJ_T = 1024;              // threads of the one workgroup

struct ProjArgs {                       // by value in the launch's arguments
    orbm_proj_camera cam;
    float scale_factors[ORBX_MAX_LEVELS];
    int n_levels;
    float log_scale_factor, th, view_cos_limit;
};

enum { FORM_FRAME = 0, FORM_FRUSTUM = 1, FORM_FUSE = 2 };

template <int FORM>
__global__ __launch_bounds__(PJ_T) void k_project(const ProjArgs a, const double *__restrict__ pose_R, const double *__restrict__ pose_t,
                                                  const float *__restrict__ points, const uint8_t *__restrict__ valid,
                                                  const float *__restrict__ normals, const float *__restrict__ min_dist,
                                                  const float *__restrict__ max_dist, const orbx_kp *__restrict__ kps1,
                                                  const int32_t *__restrict__ frame_mp, int n2, int nq, float *__restrict__ q_xy,
                                                  float *__restrict__ q_radius, int32_t *__restrict__ q_level,
                                                  float *__restrict__ q_angle, uint8_t *__restrict__ q_ok,
                                                  float *__restrict__ view_cos, int32_t *__restrict__ result)
{
    extern __shared__ uint32_t s_in_frame[]; // frustum: bit q <=> q occurs in frame_mp (Tracking.cpp:404)
    __shared__ float s_scale[ORBX_MAX_LEVELS];
    __shared__ int s_count[8];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 8) s_count[tid] = 0;
    if (FORM != FORM_FRAME) {
#pragma unroll
        for (int k = 0; k < ORBX_MAX_LEVELS; ++k)   // constant indices: the table stays in the kernel arguments' scalar loads
            if (tid == k) s_scale[k] = a.scale_factors[k];
    }
    if (FORM == FORM_FRUSTUM) {
        const int words = (nq + 31) >> 5;
        for (int w = tid; w < words; w += PJ_T) s_in_frame[w] = 0u;
        __syncthreads();
        for (int j = tid; j < n2; j += PJ_T) {
            const int q = frame_mp[j];
            if (q >= 0 && q < nq) atomicOr(&s_in_frame[q >> 5], 1u << (q & 31));
        }
    }
    __syncthreads();
    // the pose as the reference holds it: Matrix3f / Vector3f (Optimize.cpp:528-529)
    float R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (float)pose_R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = (float)pose_t[k];
    // O_w = -(R^T t) (Pose.cpp:12-14)
    const float owx = -((R[0] * t[0] + R[3] * t[1]) + R[6] * t[2]);
    const float owy = -((R[1] * t[0] + R[4] * t[1]) + R[7] * t[2]);
    const float owz = -((R[2] * t[0] + R[5] * t[1]) + R[8] * t[2]);
    const int max_level = a.n_levels - 1;
    // gate codes in the order of d_result: 0 = on, then the reference's tests in their order
    constexpr int G_INVALID = 1, G_IN_FRAME = 2, G_DEPTH = FORM == FORM_FRUSTUM ? 3 : 2, G_IMAGE = G_DEPTH + 1, G_DIST = G_DEPTH + 2,
                  G_ANGLE = G_DEPTH + 3, N_CODES = FORM == FORM_FRAME ? 4 : G_ANGLE + 1;
    for (int i0 = 0; i0 < nq; i0 += PJ_T) {   // uniform trip count: the ballots below see whole waves
        const int i = i0 + tid;
        int code = -1;
        float u = 0.f, v = 0.f, radius = 0.f, angle = 0.f, vcos = 0.f;
        int level = 0;
        if (i < nq) {
            code = 0;
            if (!valid[i]) code = G_INVALID;
            else if (FORM == FORM_FRUSTUM && ((s_in_frame[i >> 5] >> (i & 31)) & 1u)) code = G_IN_FRAME;
            else {
                const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
                const float pcx = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
                const float pcy = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
                const float pcz = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
                if (pcz < 0.f) code = G_DEPTH;
                else {
                    project(a.cam, pcx, pcy, pcz, u, v);
                    if (u < a.cam.min_x || u >= a.cam.max_x || v < a.cam.min_y || v >= a.cam.max_y) code = G_IMAGE;
                    else if (FORM == FORM_FRAME) {
                        const orbx_kp kp = kps1[i];
                        radius = a.th * kp.size;   // th * lastFrame->key_points[i].size (ORBMatcher.cpp:228)
                        level = kp.octave;
                        angle = kp.angle;
                    } else {
                        const float ox = x - owx, oy = y - owy, oz = z - owz;
                        const float dist = sqrtf((ox * ox + oy * oy) + oz * oz);
                        const float maxd = max_dist[i];
                        const float dot = (ox * normals[3 * i] + oy * normals[3 * i + 1]) + oz * normals[3 * i + 2];
                        if (dist < min_dist[i] || dist > maxd) code = G_DIST;
                        else {
                            float th_c = a.th;
                            if (FORM == FORM_FRUSTUM) {
                                vcos = dot / dist;                                   // Frame.cpp:152
                                if (vcos < a.view_cos_limit) code = G_ANGLE;
                                th_c = a.th * ((double)vcos > 0.998 ? 2.5f : 4.f);   // ORBMatcher.cpp:362-364 (float against a double literal)
                            } else if (dot < 0.5f * dist) code = G_ANGLE;            // ORBMatcher.cpp:550 (0.5 * dist is exact in float too)
                            if (code == 0) {
                                // MapPoint::predictScaleLevel (MapPoint.cpp:159-170)
                                const float c = ceilf(logf(maxd / dist) / a.log_scale_factor);
                                level = c < 0.f ? 0 : (c > (float)max_level ? max_level : (int)c);
                                radius = th_c * s_scale[level];
                            }
                        }
                    }
                }
            }
            const bool on = code == 0;
            q_ok[i] = on ? 1 : 0;
            q_xy[2 * i] = on ? u : 0.f;
            q_xy[2 * i + 1] = on ? v : 0.f;
            q_radius[i] = on ? radius : 0.f;
            q_level[i] = on ? level : 0;
            if (FORM == FORM_FRAME) q_angle[i] = on ? angle : 0.f;
            if (FORM == FORM_FRUSTUM && view_cos) view_cos[i] = on ? vcos : 0.f;
        }
#pragma unroll
        for (int c = 0; c < N_CODES; ++c) {
            const unsigned long long mk = __ballot(code == c);
            if (lane == 0 && mk) atomicAdd(&s_count[c], (int)__popcll(mk));
        }
    }
    __syncthreads();
    if (tid < 8) {
        int n = s_count[tid];
        if (FORM == FORM_FRUSTUM && tid == 7) n = s_count[G_DEPTH] + s_count[G_IMAGE] + s_count[G_DIST] + s_count[G_ANGLE]; // outView
        result[tid] = n;
    }
}

int check_common(orbm_t *h, const orbm_proj_camera *cam, const void *R, const void *t, const void *points, const void *valid, int nq,
                 const void *xy, const void *radius, const void *level, const void *ok, const void *result, void *stream, hipStream_t *s)
{
    if (!cam || !R || !t || !points || !valid || !xy || !radius || !level || !ok || !result)
        return orbx_set_error(ORBX_E_ARG, "null argument");
    if (nq < 0) return orbx_set_error(ORBX_E_ARG, "nq is negative");
    if (int rc = orbm_check_camera(cam)) return rc;
    return orbm_begin_device(h, stream, s, nq);
}

int check_levels(const float *scale_factors, int n_levels)
{
    if (!scale_factors) return orbx_set_error(ORBX_E_ARG, "null level table");
    if (n_levels < 1 || n_levels > ORBX_MAX_LEVELS) return orbx_set_error(ORBX_E_ARG, "n_levels must be 1 .. 16");
    return ORBX_OK;
}

ProjArgs make_args(const orbm_proj_camera *cam, const float *scale_factors, int n_levels, float log_scale_factor, float th, float limit)
{
    ProjArgs a = {};
    a.cam = *cam;
    for (int k = 0; k < ORBX_MAX_LEVELS; ++k) a.scale_factors[k] = scale_factors && k < n_levels ? scale_factors[k] : 1.f;
    a.n_levels = n_levels;
    a.log_scale_factor = log_scale_factor;
    a.th = th;
    a.view_cos_limit = limit;
    return a;
}

} // namespace

extern "C" int orbm_project_frame_device(orbm_t *h, const orbm_proj_camera *cam, const double *d_pose_R, const double *d_pose_t,
                                         const float *d_points, const uint8_t *d_valid, const void *d_kps1, int nq, float th,
                                         float *d_q_xy, float *d_q_radius, int32_t *d_q_octave, float *d_q_angle, uint8_t *d_q_ok,
                                         int32_t *d_result, void *stream)
{
    if (!d_kps1 || !d_q_angle) return orbx_set_error(ORBX_E_ARG, "null argument");
    hipStream_t s;
    if (int rc = check_common(h, cam, d_pose_R, d_pose_t, d_points, d_valid, nq, d_q_xy, d_q_radius, d_q_octave, d_q_ok, d_result, stream, &s)) return rc;
    hipLaunchKernelGGL(k_project<FORM_FRAME>, dim3(1), dim3(PJ_T), 0, s, make_args(cam, nullptr, 1, 1.f, th, 0.f), d_pose_R, d_pose_t,
                       d_points, d_valid, nullptr, nullptr, nullptr, (const orbx_kp *)d_kps1, nullptr, 0, nq, d_q_xy, d_q_radius,
                       d_q_octave, d_q_angle, d_q_ok, nullptr, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_project_frustum_device(orbm_t *h, const orbm_proj_camera *cam, const double *d_pose_R, const double *d_pose_t,
                                           const float *d_points, const uint8_t *d_valid, const float *d_normals,
                                           const float *d_min_dist, const float *d_max_dist, int nq, const int32_t *d_frame_mp, int n2,
                                           const float *scale_factors, int n_levels, float log_scale_factor, float th,
                                           float view_cos_limit, float *d_q_xy, float *d_q_radius, int32_t *d_q_level, uint8_t *d_q_ok,
                                           float *d_view_cos, int32_t *d_result, void *stream)
{
    if (!d_normals || !d_min_dist || !d_max_dist || n2 < 0 || (n2 > 0 && !d_frame_mp)) return orbx_set_error(ORBX_E_ARG, "bad argument");
    if (int rc = check_levels(scale_factors, n_levels)) return rc;
    hipStream_t s;
    if (int rc = check_common(h, cam, d_pose_R, d_pose_t, d_points, d_valid, nq, d_q_xy, d_q_radius, d_q_level, d_q_ok, d_result, stream, &s)) return rc;
    const size_t mask_bytes = (size_t)((nq + 31) >> 5) * 4; // <= 64 KB: no opt-in needed
    hipLaunchKernelGGL(k_project<FORM_FRUSTUM>, dim3(1), dim3(PJ_T), mask_bytes, s,
                       make_args(cam, scale_factors, n_levels, log_scale_factor, th, view_cos_limit), d_pose_R, d_pose_t, d_points, d_valid,
                       d_normals, d_min_dist, d_max_dist, nullptr, d_frame_mp, n2, nq, d_q_xy, d_q_radius, d_q_level, nullptr, d_q_ok,
                       d_view_cos, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_project_fuse_device(orbm_t *h, const orbm_proj_camera *cam, const double *d_pose_R, const double *d_pose_t,
                                        const float *d_points, const uint8_t *d_valid, const float *d_normals, const float *d_min_dist,
                                        const float *d_max_dist, int nq, const float *scale_factors, int n_levels,
                                        float log_scale_factor, float th, float *d_q_xy, float *d_q_radius, int32_t *d_q_level,
                                        uint8_t *d_q_ok, int32_t *d_result, void *stream)
{
    if (!d_normals || !d_min_dist || !d_max_dist) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (int rc = check_levels(scale_factors, n_levels)) return rc;
    hipStream_t s;
    if (int rc = check_common(h, cam, d_pose_R, d_pose_t, d_points, d_valid, nq, d_q_xy, d_q_radius, d_q_level, d_q_ok, d_result, stream, &s)) return rc;
    hipLaunchKernelGGL(k_project<FORM_FUSE>, dim3(1), dim3(PJ_T), 0, s, make_args(cam, scale_factors, n_levels, log_scale_factor, th, 0.f),
                       d_pose_R, d_pose_t, d_points, d_valid, d_normals, d_min_dist, d_max_dist, nullptr, nullptr, 0, nq, d_q_xy,
                       d_q_radius, d_q_level, nullptr, d_q_ok, nullptr, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
