// Map::applyScaleRotation on the device-resident map (include/orbm.h, "The map rescaled and rotated on the device"; Map.cpp:96-124 with
// KeyFrame::setPose and setVelocity behind it, KeyFrame.cpp:27-34, :65-69):
//   orbm_apply_scale_rotation_device   every key frame's T_cw, its state row (Rwb, twb, v) and velo_priori, every map point's position
// The rotation and the scale are READ FROM DEVICE MEMORY (the d_summary the IMU initialisation's recovery leaves), and so is the decision
// of LocalMapping.cpp:435-439: with be_first and a scale below min_scale every kernel returns before its first store, so the chain needs
// no host wait to honour it.
//
// Shape: a key frame is ONE WAVE, four per workgroup -- T_wb = T_cw.inverse() * T_cb is orbi_imu_pose_device's code from the shared
// orbi_so3.h, which spreads a pose over the first lanes of a wave through LDS; a map point is a thread.  Float, the header's orders, no
// fused multiply-add.  Integer atomics only (the counts): the same input gives the same bytes.
#include <hip/hip_runtime.h>

#include "../../include/orbi.h"
#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_host.h"
#include "orb_math.h"
#include "orbi_so3.h"
#include "orbm_internal.h"

#pragma clang fp contract(off)

static_assert(sizeof(orbi_prior) == 36 * sizeof(float) && offsetof(orbi_prior, velo_priori) == 0, "orbi_prior as the rescale writes it");

namespace {

constexpr int RS_WAVES = 4, RS_T = 64 * RS_WAVES;
enum { RS_KF = 0, RS_RANGE = 1, RS_DUPLICATE = 2, RS_REFUSED = 3, RS_POINTS = 4 };   // d_result; the first four are ORBI_R_*

struct RescaleArgs {
    orbi_calib cal;
    int n_kf;
    double *pose_R, *pose_t;
    const uint8_t *bad;
    const int32_t *kf_imu;
    float *state;
    int n_src;
    orbi_prior *priors;
    int n_priors;
    float *points;
    const uint8_t *valid;
    const int32_t *n_points;
    int cap_points;
    const float *summary;
    int be_first;
    float min_scale;
    int32_t *result;
};

__device__ __forceinline__ bool refused(const RescaleArgs &a) { return a.be_first && a.summary[9] < a.min_scale; }

__global__ void k_rescale_begin(const RescaleArgs a)
{
    if (threadIdx.x < 8) a.result[threadIdx.x] = threadIdx.x == RS_REFUSED ? refused(a) : 0;
}

// LDS words of a wave: Rwy[9], the old T_cw (R[9], t[3]), the new one (R[9], t[3]), (Rcb, tcb)[12], twc[3]
enum { L_RWY = 0, L_R = 9, L_T = 18, L_R2 = 21, L_T2 = 30, L_CB = 33, L_TWC = 45, L_WORDS = 48 };

__global__ __launch_bounds__(RS_T) void k_rescale_kf(const RescaleArgs a)
{
    __shared__ float s_f[RS_WAVES][L_WORDS];
    if (refused(a)) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = blockIdx.x * RS_WAVES + wave;
    if (k >= a.n_kf || a.bad[k]) return;             // no workgroup barrier in this kernel
    float *S = s_f[wave];
    const float s = a.summary[9];
    const int row = __builtin_amdgcn_readfirstlane(a.kf_imu[3 * (size_t)k]), slot = __builtin_amdgcn_readfirstlane(a.kf_imu[3 * (size_t)k + 2]);
    int code = RS_KF;
    if (row < 0 || row >= a.n_src || slot < 0 || slot >= a.n_priors) code = RS_RANGE;
    else {                                           // a row or slot that an earlier live key frame names
        bool dup = false;
        for (int m = lane; m < k; m += 64)
            if (!a.bad[m] && (a.kf_imu[3 * (size_t)m] == row || a.kf_imu[3 * (size_t)m + 2] == slot)) dup = true;
        if (__ballot(dup)) code = RS_DUPLICATE;
    }
    if (lane < 9) S[L_RWY + lane] = a.summary[lane], S[L_R + lane] = (float)a.pose_R[9 * (size_t)k + lane], S[L_CB + lane] = a.cal.Rcb[lane];
    if (lane < 3) S[L_T + lane] = (float)a.pose_t[3 * (size_t)k + lane], S[L_CB + 9 + lane] = a.cal.tcb[lane];
    WSYNC();
    // setPose(Tcw.R * Rwy, Tcw.t * s)
    if (lane < 9) {
        const float r = m3(S + L_R, S + L_RWY, lane / 3, lane % 3);
        S[L_R2 + lane] = r;
        a.pose_R[9 * (size_t)k + lane] = (double)r;
    } else if (lane < 12) {
        const float t = a.be_first ? mul(S[L_T + lane - 9], s) : S[L_T + lane - 9];
        S[L_T2 + lane - 9] = t;
        a.pose_t[3 * (size_t)k + lane - 9] = (double)t;
    }
    WSYNC();
    if (code == RS_KF) {
        float *dst = a.state + 15 * (size_t)row;
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        if (lane >= 12 && lane < 15) v0 = dst[12], v1 = dst[13], v2 = dst[14];
        imu_pose_from_camera(S + L_R2, S + L_T2, S + L_CB, S + L_TWC, dst, lane);   // its fence stands between the reads above and the stores below
        if (lane >= 12 && lane < 15) {               // setVelocity((Ryw * Vw) * s), which also sets velo_priori
            const int e = lane - 12;
            const float rv = sum3(mul(S[L_RWY + e], v0), mul(S[L_RWY + 3 + e], v1), mul(S[L_RWY + 6 + e], v2));
            const float v = a.be_first ? mul(rv, s) : rv;
            dst[lane] = v;
            a.priors[slot].velo_priori[e] = v;
        }
    }
    if (lane == 0) atomicAdd(&a.result[code], 1);
}

__global__ __launch_bounds__(RS_T) void k_rescale_points(const RescaleArgs a)
{
    __shared__ int s_cnt;
    if (refused(a)) return;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int n = min(max(a.n_points[0], 0), a.cap_points);
    const int p = blockIdx.x * RS_T + threadIdx.x;
    if (p < n && a.valid[p]) {                       // setPos((Ryw * pos) * s)
        const float s = a.summary[9];
        float *P = a.points + 3 * (size_t)p;
        const float x = P[0], y = P[1], z = P[2];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const float r = sum3(mul(a.summary[e], x), mul(a.summary[3 + e], y), mul(a.summary[6 + e], z));
            P[e] = a.be_first ? mul(r, s) : r;
        }
        atomicAdd(&s_cnt, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&a.result[RS_POINTS], s_cnt);
}

} // namespace

extern "C" int orbm_apply_scale_rotation_device(orbm_t *h, const struct orbi_calib *calib, int n_kf, double *d_pose_R, double *d_pose_t,
                                                const uint8_t *d_bad, const int32_t *d_kf_imu, float *d_state, int n_src,
                                                struct orbi_prior *d_priors, int n_priors, float *d_points, const uint8_t *d_valid,
                                                const int32_t *d_n_points, int cap_points, const float *d_summary, int be_first, float min_scale,
                                                int32_t *d_result, void *stream)
{
    if (!calib || !d_summary || !d_n_points || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (n_kf < 0 || n_src < 0 || n_priors < 0 || cap_points < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (n_kf > 0 && (!d_pose_R || !d_pose_t || !d_bad || !d_kf_imu || !d_state || !d_priors)) return orbx_set_error(ORBX_E_ARG, "null key-frame array");
    if (cap_points > 0 && (!d_points || !d_valid)) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    RescaleArgs a = {};
    a.cal = *calib, a.n_kf = n_kf, a.pose_R = d_pose_R, a.pose_t = d_pose_t, a.bad = d_bad, a.kf_imu = d_kf_imu, a.state = d_state, a.n_src = n_src;
    a.priors = d_priors, a.n_priors = n_priors, a.points = d_points, a.valid = d_valid, a.n_points = d_n_points, a.cap_points = cap_points;
    a.summary = d_summary, a.be_first = be_first != 0, a.min_scale = min_scale, a.result = d_result;
    hipLaunchKernelGGL(k_rescale_begin, dim3(1), dim3(64), 0, s, a);
    if (n_kf > 0) hipLaunchKernelGGL(k_rescale_kf, dim3((n_kf + RS_WAVES - 1) / RS_WAVES), dim3(RS_T), 0, s, a);
    if (cap_points > 0) hipLaunchKernelGGL(k_rescale_points, dim3((cap_points + RS_T - 1) / RS_T), dim3(RS_T), 0, s, a);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
