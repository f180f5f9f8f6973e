// New map points from the matches of one key-frame pair, on the device (include/orbm.h, "New map points triangulated on the
// device"): what LocalMapping::createNewMapPoints does between SearchForTriangulation and the fuse.
//   orbm_triangulate_matches_device   LocalMapping.cpp:171-253, TwoViewReconstruction.cpp:689-705, MapPoint.cpp:16-30, :43-76
//   orbm_triangulate_matches          the same with host pointers: one pinned copy each way on the handle's stream
//
// Evaluation orders outside the singular-vector solve are the header's (float; no fused multiply-add: the build passes
// -ffp-contract=off and the pragma below repeats it here; `/` and sqrtf are the correctly rounded ones).
//
// The solve: the reference takes the last column of V of a JacobiSVD of the 4x4 matrix A.  Here a one-sided (Hestenes) Jacobi
// rotates pairs of COLUMNS of A until they are orthogonal, applying the same rotations to V = I; the column of least norm then
// belongs to the smallest singular value and its column of V is the answer.  TR_SWEEPS cyclic sweeps over the six pairs, fully in
// registers with constant indices (no scratch); a numpy float32 restatement of this loop settles to its final digits in four
// sweeps on the test clouds, six are run.  A non-finite matrix (a non-finite key point) yields a non-finite vector, as there.
//
// Shape: a call is at most a few thousand matches and is bound by latency: ONE launch of ONE 1024-thread workgroup, a feature of
// key frame 1 per thread and chunk.  A full table has to be found BEFORE anything is written and a thread cannot keep the points
// of an unbounded number of chunks, so the features are walked twice: the first walk decides and counts (and writes d_code), the
// second repeats the same arithmetic on the same inputs -- bit for bit the same decisions -- and appends the accepted ones in
// ascending feature order behind a block-wide prefix sum of wave ballots.  No handle scratch, no allocation, no host wait.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>

#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_host.h"
#include "orbm_internal.h"
#include "orbm_camera.h"
#include "orbm_jacobi.h"

#pragma clang fp contract(off)

namespace {

constexpr int TR_T = 1024;     // threads of the one workgroup
constexpr int TR_WAVES = TR_T / 64;

struct TriArgs {               // by value in the launch's arguments
    orbm_proj_camera cam;
    float sigma2[ORBX_MAX_LEVELS];
    int n_levels;
    float max_scale_factor, ratio_factor;
    double cos_parallax, chi2;
    int scale_w, scale_h;      // the Fisheye scale table's size; scale_w = 0: one entry per key point, key frame 1 then key frame 2
    int table_base;            // row r of the table is written at r - table_base (the host entry point stages the new rows only)
};

struct TriPoint {
    float p[3], nrm[3], min_dist, max_dist;
};

// gate codes = index of the counter in d_result (1 is the overflow flag, no gate)
enum { T_ACCEPTED = 0, T_FAIL = 2, T_ILLEGAL = 3, T_PARALLAX = 4, T_NEGATIVE = 5, T_REPROJ = 6, T_SCALE = 7 };

// dot4, rotate (one Hestenes rotation of two columns) and TR_SWEEPS: orbm_jacobi.h, shared with orbm_two_view_pose.hip

// camera->backProject(kp.pt): Pinhole.cpp:40-42 / Fisheye.cpp:68-73
__device__ __forceinline__ void back_project(const TriArgs &a, float inv_fx, float inv_fy, const float *__restrict__ scale, int per_kp_index,
                                             float x, float y, float &xn, float &yn)
{
    xn = (x - a.cam.cx) * inv_fx;
    yn = (y - a.cam.cy) * inv_fy;
    if (a.cam.model != 0) {
        int at = per_kp_index;
        if (a.scale_w > 0) {   // scale_mat.at<float>(p.y, p.x), the index kept inside the table
            const int xi = min(max((int)x, 0), a.scale_w - 1), yi = min(max((int)y, 0), a.scale_h - 1);
            at = yi * a.scale_w + xi;
        }
        const float s = scale[at];
        xn = xn * s;
        yn = yn * s;
    }
}

// LocalMapping.cpp:181-241 for one match; returns the gate code
__device__ __forceinline__ int triangulate_one(const TriArgs &a, const float *s_sigma2, const float (&R1)[9], const float (&t1)[3],
                                               const float (&R2)[9], const float (&t2)[3], const float (&O1)[3], const float (&O2)[3],
                                               float inv_fx, float inv_fy, const float *__restrict__ scale, int i, int m, int n1,
                                               const orbx_kp &kp1, const orbx_kp &kp2, TriPoint &out)
{
    float xn1, yn1, xn2, yn2;
    back_project(a, inv_fx, inv_fy, scale, i, kp1.x, kp1.y, xn1, yn1);
    back_project(a, inv_fx, inv_fy, scale, n1 + m, kp2.x, kp2.y, xn2, yn2);
    // A (TwoViewReconstruction.cpp:692-696) by column: col[k][row]; P = [R | t]
    float A[4][4], V[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float p1_0 = k < 3 ? R1[k] : t1[0], p1_1 = k < 3 ? R1[3 + k] : t1[1], p1_2 = k < 3 ? R1[6 + k] : t1[2];
        const float p2_0 = k < 3 ? R2[k] : t2[0], p2_1 = k < 3 ? R2[3 + k] : t2[1], p2_2 = k < 3 ? R2[6 + k] : t2[2];
        A[k][0] = xn1 * p1_2 - p1_0;
        A[k][1] = yn1 * p1_2 - p1_1;
        A[k][2] = xn2 * p2_2 - p2_0;
        A[k][3] = yn2 * p2_2 - p2_1;
#pragma unroll
        for (int r = 0; r < 4; ++r) V[k][r] = r == k ? 1.f : 0.f;
    }
    for (int sweep = 0; sweep < TR_SWEEPS; ++sweep) {
        rotate(A[0], A[1], V[0], V[1]);
        rotate(A[0], A[2], V[0], V[2]);
        rotate(A[0], A[3], V[0], V[3]);
        rotate(A[1], A[2], V[1], V[2]);
        rotate(A[1], A[3], V[1], V[3]);
        rotate(A[2], A[3], V[2], V[3]);
    }
    // the column of least norm: strict '<' in ascending order
    float best = dot4(A[0], A[0]);
    float ph[4] = {V[0][0], V[0][1], V[0][2], V[0][3]};
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const float nk = dot4(A[k], A[k]);
        const bool take = nk < best;
        best = take ? nk : best;
#pragma unroll
        for (int r = 0; r < 4; ++r) ph[r] = take ? V[k][r] : ph[r];
    }
    if (ph[3] == 0.f) return T_FAIL;                                                      // TwoViewReconstruction.cpp:700
    const float x = ph[0] / ph[3], y = ph[1] / ph[3], z = ph[2] / ph[3];                   // :703
    if (!isfinite(x) || !isfinite(y) || !isfinite(z)) return T_ILLEGAL;                   // LocalMapping.cpp:187
    // parallax (:193-204)
    float n1x = x - O1[0], n1y = y - O1[1], n1z = z - O1[2];
    const float dist1 = sqrtf((n1x * n1x + n1y * n1y) + n1z * n1z);
    n1x = n1x / dist1, n1y = n1y / dist1, n1z = n1z / dist1;
    float n2x = x - O2[0], n2y = y - O2[1], n2z = z - O2[2];
    const float dist2 = sqrtf((n2x * n2x + n2y * n2y) + n2z * n2z);
    n2x = n2x / dist2, n2y = n2y / dist2, n2z = n2z / dist2;
    const float cos_parallax = (n1x * n2x + n1y * n2y) + n1z * n2z;
    if ((double)cos_parallax > a.cos_parallax) return T_PARALLAX;                         // float against a double literal
    const int l1 = min(max(kp1.octave, 0), a.n_levels - 1), l2 = min(max(kp2.octave, 0), a.n_levels - 1);
    const float s1 = s_sigma2[l1], s2 = s_sigma2[l2];
    // key frame 1 (:207-219)
    float u, v;
    const float z1 = ((R1[6] * x + R1[7] * y) + R1[8] * z) + t1[2];
    if (z1 <= 0.f) return T_NEGATIVE;
    project(a.cam, ((R1[0] * x + R1[1] * y) + R1[2] * z) + t1[0], ((R1[3] * x + R1[4] * y) + R1[5] * z) + t1[1], z1, u, v);
    const float e1 = (u - kp1.x) * (u - kp1.x) + (v - kp1.y) * (v - kp1.y);
    if ((double)e1 > (double)s1 * a.chi2) return T_REPROJ;                                // float * double literal
    // key frame 2 (:222-234)
    const float z2 = ((R2[6] * x + R2[7] * y) + R2[8] * z) + t2[2];
    if (z2 <= 0.f) return T_NEGATIVE;
    project(a.cam, ((R2[0] * x + R2[1] * y) + R2[2] * z) + t2[0], ((R2[3] * x + R2[4] * y) + R2[5] * z) + t2[1], z2, u, v);
    const float e2 = (u - kp2.x) * (u - kp2.x) + (v - kp2.y) * (v - kp2.y);
    if ((double)e2 > (double)s2 * a.chi2) return T_REPROJ;
    // scale consistency (:236-241)
    const float dist_ratio = dist1 / dist2;
    const float level_ratio = sqrtf(s2) / sqrtf(s1);
    if (dist_ratio * a.ratio_factor < level_ratio || dist_ratio > level_ratio * a.ratio_factor) return T_SCALE;
    // MapPoint::MapPoint + update() (MapPoint.cpp:16-30, :43-76), the ...Invariance getters (:83-91)
    out.p[0] = x, out.p[1] = y, out.p[2] = z;
    out.nrm[0] = (n1x + n2x) / 2.f, out.nrm[1] = (n1y + n2y) / 2.f, out.nrm[2] = (n1z + n2z) / 2.f;
    const float span = dist2 * kp2.size;
    out.max_dist = 1.2f * span;
    out.min_dist = 0.8f * (span / a.max_scale_factor);
    return T_ACCEPTED;
}

__global__ __launch_bounds__(TR_T) void k_triangulate(const TriArgs a, const double *__restrict__ pose_R1, const double *__restrict__ pose_t1,
                                                      const double *__restrict__ pose_R2, const double *__restrict__ pose_t2,
                                                      const orbx_kp *__restrict__ kps1, int n1, const orbx_kp *__restrict__ kps2,
                                                      const uint32_t *__restrict__ desc2, int n2, const int32_t *__restrict__ matches12,
                                                      const float *__restrict__ scale, int32_t *n_points, int cap_points,
                                                      float *__restrict__ points, uint8_t *__restrict__ valid, float *__restrict__ normals,
                                                      float *__restrict__ min_dist, float *__restrict__ max_dist, uint32_t *__restrict__ desc,
                                                      int32_t *__restrict__ obs, int32_t *__restrict__ mp1, int32_t *__restrict__ mp2,
                                                      uint8_t *__restrict__ has_mp1, uint8_t *__restrict__ has_mp2,
                                                      int32_t *__restrict__ code_out, int32_t *__restrict__ result)
{
    __shared__ float s_sigma2[ORBX_MAX_LEVELS];
    __shared__ int s_count[8];
    __shared__ int s_wave[TR_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 8) s_count[tid] = 0;
#pragma unroll
    for (int k = 0; k < ORBX_MAX_LEVELS; ++k)   // constant indices: the table stays in the kernel arguments' scalar loads
        if (tid == k) s_sigma2[k] = a.sigma2[k];
    __syncthreads();
    // both poses as the reference holds them: Matrix3f / Vector3f
    float R1[9], t1[3], R2[9], t2[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R1[k] = (float)pose_R1[k], R2[k] = (float)pose_R2[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t1[k] = (float)pose_t1[k], t2[k] = (float)pose_t2[k];
    // O_w = -(R^T t) (Pose.cpp:12-14)
    float O1[3], O2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        O1[k] = -((R1[k] * t1[0] + R1[3 + k] * t1[1]) + R1[6 + k] * t1[2]);
        O2[k] = -((R2[k] * t2[0] + R2[3 + k] * t2[1]) + R2[6 + k] * t2[2]);
    }
    const float inv_fx = 1.f / a.cam.fx, inv_fy = 1.f / a.cam.fy;   // Camera: float inv_fx = 1.f / fx
    int old_n = 0, row0 = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int i0 = 0; i0 < n1; i0 += TR_T) {   // uniform trip count: the ballots and barriers below see whole waves
            const int i = i0 + tid;
            int code = -1, m = -1;
            TriPoint pt;
            if (i < n1) {
                m = matches12[i];
                if (m >= 0 && m < n2) code = triangulate_one(a, s_sigma2, R1, t1, R2, t2, O1, O2, inv_fx, inv_fy, scale, i, m, n1, kps1[i], kps2[m], pt);
                if (pass == 0 && code_out) code_out[i] = code;
            }
            if (pass == 0) {
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    if (c == 1) continue;
                    const unsigned long long mk = __ballot(code == c);
                    if (lane == 0 && mk) atomicAdd(&s_count[c], (int)__popcll(mk));
                }
            } else {
                // rows in ascending feature order: waves before this one, then lanes before this one
                const unsigned long long mk = __ballot(code == T_ACCEPTED);
                if (lane == 0) s_wave[wave] = (int)__popcll(mk);
                __syncthreads();
                int before = 0, total = 0;
#pragma unroll
                for (int w = 0; w < TR_WAVES; ++w) {
                    const int c = s_wave[w];
                    before += w < wave ? c : 0;
                    total += c;
                }
                if (code == T_ACCEPTED) {
                    const int row = row0 + before + (int)__popcll(mk & ((1ull << lane) - 1ull));   // < cap_points: checked after pass 0
                    const int at = row - a.table_base;
                    points[3 * at] = pt.p[0], points[3 * at + 1] = pt.p[1], points[3 * at + 2] = pt.p[2];
                    normals[3 * at] = pt.nrm[0], normals[3 * at + 1] = pt.nrm[1], normals[3 * at + 2] = pt.nrm[2];
                    min_dist[at] = pt.min_dist;
                    max_dist[at] = pt.max_dist;
                    valid[at] = 1;
#pragma unroll
                    for (int k = 0; k < 8; ++k) desc[8 * at + k] = desc2[8 * m + k];   // curKF->descriptors.row(match.second) (MapPoint.cpp:28)
                    obs[2 * at] = i, obs[2 * at + 1] = m;
                    mp1[i] = row, mp2[m] = row;                                         // LocalMapping.cpp:245-246
                    has_mp1[i] = 1, has_mp2[m] = 1;
                }
                row0 += total;
                __syncthreads();   // s_wave is rewritten by the next chunk
            }
        }
        if (pass == 0) {
            __syncthreads();
            const int accepted = s_count[0];
            old_n = *n_points;   // read by every thread ahead of the one store below, which follows a barrier
            const bool overflow = accepted > 0 && (old_n < 0 || old_n > cap_points || accepted > cap_points - old_n);
            if (tid < 8) result[tid] = tid == 0 ? (overflow ? 0 : accepted) : tid == 1 ? (overflow ? 1 : 0) : s_count[tid];
            if (overflow || accepted == 0) return;   // uniform: the table, the slots, the flags and the counter stay as they were
            row0 = old_n;
        }
    }
    __syncthreads();
    if (tid == 0) *n_points = row0;
}

struct TriCall {   // the arguments both entry points share, checked by check()
    const orbm_proj_camera *cam;
    const float *sigma2;
    int n_levels;
    float max_scale_factor;
    double cos_parallax, chi2;
    float ratio_factor;
};

int check(const TriCall &c, const void *scale, int scale_w, int scale_h, const void *R1, const void *t1, const void *R2,
          const void *t2, const void *kps1, int n1, const void *kps2, const void *desc2, int n2, const void *matches12, const void *n_points,
          int cap_points, const void *points, const void *valid, const void *normals, const void *min_dist, const void *max_dist,
          const void *desc, const void *obs, const void *mp1, const void *mp2, const void *has1, const void *has2, const void *result)
{
    if (!c.cam || !c.sigma2 || !R1 || !t1 || !R2 || !t2 || !n_points || !result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (n1 < 0 || n2 < 0 || cap_points < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (n1 > 0 && (!kps1 || !matches12 || !mp1 || !has1)) return orbx_set_error(ORBX_E_ARG, "null key-frame 1 array");
    if (n2 > 0 && (!kps2 || !desc2 || !mp2 || !has2)) return orbx_set_error(ORBX_E_ARG, "null key-frame 2 array");
    if (cap_points > 0 && (!points || !valid || !normals || !min_dist || !max_dist || !desc || !obs))
        return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if (int rc = orbm_check_camera(c.cam)) return rc;
    if (c.cam->model == 1 && (!scale || scale_w < 1 || scale_h < 1)) return orbx_set_error(ORBX_E_ARG, "Fisheye needs its scale table");
    if (c.n_levels < 1 || c.n_levels > ORBX_MAX_LEVELS) return orbx_set_error(ORBX_E_ARG, "n_levels must be 1 .. 16");
    if ((((uintptr_t)desc2) | ((uintptr_t)desc)) & 3) return orbx_set_error(ORBX_E_ARG, "descriptor arrays must be 4-byte aligned");
    return ORBX_OK;
}

TriArgs make_args(const TriCall &c, int scale_w, int scale_h, int table_base)
{
    TriArgs a = {};
    a.cam = *c.cam;
    for (int k = 0; k < ORBX_MAX_LEVELS; ++k) a.sigma2[k] = k < c.n_levels ? c.sigma2[k] : 1.f;
    a.n_levels = c.n_levels;
    a.max_scale_factor = c.max_scale_factor;
    a.ratio_factor = c.ratio_factor;
    a.cos_parallax = c.cos_parallax;
    a.chi2 = c.chi2;
    a.scale_w = scale_w;
    a.scale_h = scale_h;
    a.table_base = table_base;
    return a;
}

// The host entry point's staging block, [inputs | in / out | outputs] in 16-byte aligned pieces; the device block and the pinned
// block share the layout, so one copy goes up (inputs, in / out) and one comes down (in / out, outputs).
struct TriStage {
    double *poses;
    orbx_kp *kps1, *kps2;
    uint8_t *desc2;
    int32_t *matches12;
    float *scale;
    int32_t *mp1, *mp2;
    uint8_t *has1, *has2;
    int32_t *n_points;
    float *points, *normals, *min_dist, *max_dist;
    uint8_t *desc;
    int32_t *obs;
    uint8_t *valid;
    int32_t *code, *result;
    size_t in_end, inout_end, total;
    char *base;
    template <typename T> T *take(size_t n)
    {
        T *p = (T *)(base + total);
        total += (n * sizeof(T) + 15) & ~(size_t)15;
        return p;
    }
    void lay(void *block, size_t n1, size_t n2, size_t n_scale, size_t rows)
    {
        base = (char *)block;
        total = 0;
        poses = take<double>(24), kps1 = take<orbx_kp>(n1), kps2 = take<orbx_kp>(n2), desc2 = take<uint8_t>(n2 * 32);
        matches12 = take<int32_t>(n1), scale = take<float>(n_scale);
        in_end = total;
        mp1 = take<int32_t>(n1), mp2 = take<int32_t>(n2), has1 = take<uint8_t>(n1), has2 = take<uint8_t>(n2), n_points = take<int32_t>(1);
        inout_end = total;
        points = take<float>(rows * 3), normals = take<float>(rows * 3), min_dist = take<float>(rows), max_dist = take<float>(rows);
        desc = take<uint8_t>(rows * 32), obs = take<int32_t>(rows * 2), valid = take<uint8_t>(rows);
        code = take<int32_t>(n1), result = take<int32_t>(8);
    }
};

} // namespace

extern "C" int orbm_triangulate_matches_device(orbm_t *h, const orbm_proj_camera *cam, const float *d_fisheye_scale, int scale_w, int scale_h,
                                               const double *d_pose_R1, const double *d_pose_t1, const double *d_pose_R2,
                                               const double *d_pose_t2, const void *d_kps1, int n1, const void *d_kps2,
                                               const uint8_t *d_desc2, int n2, const int32_t *d_matches12, const float *sigma2, int n_levels,
                                               float max_scale_factor, double cos_parallax, double chi2, float ratio_factor,
                                               int32_t *d_n_points, int cap_points, float *d_points, uint8_t *d_valid, float *d_normals,
                                               float *d_min_dist, float *d_max_dist, uint8_t *d_desc, int32_t *d_obs, int32_t *d_mp1,
                                               int32_t *d_mp2, uint8_t *d_has_mp1, uint8_t *d_has_mp2, int32_t *d_code, int32_t *d_result,
                                               void *stream)
{
    const TriCall c = {cam, sigma2, n_levels, max_scale_factor, cos_parallax, chi2, ratio_factor};
    if (int rc = check(c, d_fisheye_scale, scale_w, scale_h, d_pose_R1, d_pose_t1, d_pose_R2, d_pose_t2, d_kps1, n1, d_kps2, d_desc2, n2,
                       d_matches12, d_n_points, cap_points, d_points, d_valid, d_normals, d_min_dist, d_max_dist, d_desc, d_obs, d_mp1, d_mp2,
                       d_has_mp1, d_has_mp2, d_result))
        return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    hipLaunchKernelGGL(k_triangulate, dim3(1), dim3(TR_T), 0, s, make_args(c, cam->model == 1 ? scale_w : 0, scale_h, 0), d_pose_R1, d_pose_t1,
                       d_pose_R2, d_pose_t2, (const orbx_kp *)d_kps1, n1, (const orbx_kp *)d_kps2, (const uint32_t *)d_desc2, n2, d_matches12,
                       d_fisheye_scale, d_n_points, cap_points, d_points, d_valid, d_normals, d_min_dist, d_max_dist, (uint32_t *)d_desc, d_obs,
                       d_mp1, d_mp2, d_has_mp1, d_has_mp2, d_code, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_triangulate_matches(orbm_t *h, const orbm_proj_camera *cam, const float *fisheye_scale, int scale_w, int scale_h,
                                        const double *pose_R1, const double *pose_t1, const double *pose_R2, const double *pose_t2,
                                        const void *kps1, int n1, const void *kps2, const uint8_t *desc2, int n2, const int32_t *matches12,
                                        const float *sigma2, int n_levels, float max_scale_factor, double cos_parallax, double chi2,
                                        float ratio_factor, int32_t *n_points, int cap_points, float *points, uint8_t *valid, float *normals,
                                        float *min_dist, float *max_dist, uint8_t *desc, int32_t *obs, int32_t *mp1, int32_t *mp2,
                                        uint8_t *has_mp1, uint8_t *has_mp2, int32_t *code, int32_t *result)
{
    const TriCall c = {cam, sigma2, n_levels, max_scale_factor, cos_parallax, chi2, ratio_factor};
    if (int rc = check(c, fisheye_scale, scale_w, scale_h, pose_R1, pose_t1, pose_R2, pose_t2, kps1, n1, kps2, desc2, n2, matches12, n_points,
                       cap_points, points, valid, normals, min_dist, max_dist, desc, obs, mp1, mp2, has_mp1, has_mp2, result))
        return rc;
    if (int rc = orb_need_device()) return rc;
    if (!h) return orbx_set_error(ORBX_E_ARG, "null handle");
    const bool fisheye = cam->model == 1;
    const int old_n = *n_points;
    // the rows this call can append: one per match, and no more than the table has left
    int n_match = 0;
    for (int i = 0; i < n1; ++i) n_match += matches12[i] >= 0 && matches12[i] < n2;
    const int room = old_n >= 0 && old_n <= cap_points ? cap_points - old_n : 0;
    const size_t rows = (size_t)std::min(n_match, room);
    const size_t n_scale = fisheye ? (size_t)n1 + n2 : 0;
    TriStage hp, dp;
    hp.lay(nullptr, n1, n2, n_scale, rows);   // measures
    void *dev = nullptr, *pin = nullptr;
    hipStream_t s = nullptr;
    ORB_TRY(orbm_host_stage(h, hp.total, &dev, &pin, &s));
    hp.lay(pin, n1, n2, n_scale, rows);
    dp.lay(dev, n1, n2, n_scale, rows);
    memcpy(hp.poses, pose_R1, 72), memcpy(hp.poses + 9, pose_t1, 24), memcpy(hp.poses + 12, pose_R2, 72), memcpy(hp.poses + 21, pose_t2, 24);
    if (n1) memcpy(hp.kps1, kps1, (size_t)n1 * sizeof(orbx_kp)), memcpy(hp.matches12, matches12, (size_t)n1 * 4), memcpy(hp.mp1, mp1, (size_t)n1 * 4), memcpy(hp.has1, has_mp1, (size_t)n1);
    if (n2) memcpy(hp.kps2, kps2, (size_t)n2 * sizeof(orbx_kp)), memcpy(hp.desc2, desc2, (size_t)n2 * 32), memcpy(hp.mp2, mp2, (size_t)n2 * 4), memcpy(hp.has2, has_mp2, (size_t)n2);
    *hp.n_points = old_n;
    if (fisheye) {   // scale_mat.at<float>(p.y, p.x) per key point, key frame 1 then key frame 2; the index kept inside the table as the kernel does
        const orbx_kp *kk[2] = {(const orbx_kp *)kps1, (const orbx_kp *)kps2};
        const int nn[2] = {n1, n2};
        for (int v = 0; v < 2; ++v)
            for (int i = 0; i < nn[v]; ++i) {
                const float x = kk[v][i].x, y = kk[v][i].y;
                const int xi = x >= (float)(scale_w - 1) ? scale_w - 1 : x > 0.f ? (int)x : 0;   // NaN -> 0
                const int yi = y >= (float)(scale_h - 1) ? scale_h - 1 : y > 0.f ? (int)y : 0;
                hp.scale[(size_t)v * n1 + i] = fisheye_scale[(size_t)yi * scale_w + xi];
            }
    }
    ORB_TRY(hipMemcpyAsync(dev, pin, hp.inout_end, hipMemcpyHostToDevice, s));
    // the table's rows from old_n on are the staged ones: table_base = old_n, capacity = old_n + rows
    hipLaunchKernelGGL(k_triangulate, dim3(1), dim3(TR_T), 0, s, make_args(c, 0, 0, old_n), dp.poses, dp.poses + 9, dp.poses + 12, dp.poses + 21,
                       dp.kps1, n1, dp.kps2, (const uint32_t *)dp.desc2, n2, dp.matches12, dp.scale, dp.n_points, old_n + (int)rows, dp.points,
                       dp.valid, dp.normals, dp.min_dist, dp.max_dist, (uint32_t *)dp.desc, dp.obs, dp.mp1, dp.mp2, dp.has1, dp.has2, dp.code,
                       dp.result);
    ORB_TRY(hipGetLastError());
    ORB_TRY(hipMemcpyAsync((char *)pin + hp.in_end, (char *)dev + hp.in_end, hp.total - hp.in_end, hipMemcpyDeviceToHost, s));
    ORB_TRY(hipStreamSynchronize(s));
    memcpy(result, hp.result, 32);
    if (code && n1) memcpy(code, hp.code, (size_t)n1 * 4);
    const size_t added = (size_t)hp.result[0];
    if (added) {   // no overflow: rows old_n .. old_n + added - 1, the slots, the flags, the counter
        memcpy(points + 3 * (size_t)old_n, hp.points, added * 12), memcpy(normals + 3 * (size_t)old_n, hp.normals, added * 12);
        memcpy(min_dist + old_n, hp.min_dist, added * 4), memcpy(max_dist + old_n, hp.max_dist, added * 4);
        memcpy(desc + 32 * (size_t)old_n, hp.desc, added * 32), memcpy(obs + 2 * (size_t)old_n, hp.obs, added * 8), memcpy(valid + old_n, hp.valid, added);
        memcpy(mp1, hp.mp1, (size_t)n1 * 4), memcpy(mp2, hp.mp2, (size_t)n2 * 4), memcpy(has_mp1, hp.has1, (size_t)n1), memcpy(has_mp2, hp.has2, (size_t)n2);
        *n_points = *hp.n_points;
    }
    return ORBX_OK;
}
