// The writer of the device-resident map-point table (include/orbm.h, "Map points refreshed on the device") and the two small
// reductions that sit beside it in the reference:
//   orbm_refresh_points_device       MapPoint::computeDescriptor + MapPoint::update (MapPoint.cpp:43-76, :103-152) for a list of
//                                    table rows, and the counting loop of KeyFrame::updateConnections (KeyFrame.cpp:233-242)
//   orbm_scene_median_depth_device   KeyFrame::computeSceneMedianDepth (KeyFrame.cpp:159-179) for many key frames, with the
//                                    baseline of LocalMapping.cpp:163
//
// Evaluation orders are the header's (float; no fused multiply-add: the build passes -ffp-contract=off and the pragma below
// repeats it here; `/` and sqrtf are the correctly rounded ones).
//
// Shape of the refresh.  A point has 2-15 observations as a rule, and everything about one is a chain of dependent gathers (the
// observation, its key frame's feature count, pose, bad flag, descriptor pointer, descriptor), so the kernel lives on waves in
// flight: workgroups of four waves, ONE SELECTED ROW PER WAVE, a 2 KB slice of LDS per wave (8 KB per workgroup: LDS never caps
// the CU below its 32 waves).  An observation per lane and chunk of 64:
//   walk 1   validates, counts, adds to d_covis, computes the unit direction per lane and sums the directions in CSR order by
//            reading lane after lane (the order is the header's, so no tree);
//   walk 2   the medoid of the good descriptors.  The slice holds a TILE of 64 observations' descriptors; a lane owns a row and
//            finds the median of its distances by the value bisection of k_medoid (9 counting steps over 0 .. 256).  A list of at
//            most 64 observations -- the common case -- fills the tile once; a longer one walks its tiles again in every step
//            and re-gathers them, which costs 9 * (n / 64)^2 tile loads and is the price of not holding 32 KB per point.
// Counting does not depend on the order inside a tile and the winner is the least (median, position in the list), so both forms
// -- and the shortcut for one or two good rows, whose medians are all 0 -- give the same bytes.
// No scratch memory, no handle scratch, no allocation, no host wait: a clearing launch (d_covis, d_result) and the kernel.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orbm_internal.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int RF_WAVES = 4;           // waves (= selected rows in flight) per workgroup
constexpr int RF_T = RF_WAVES * 64;
constexpr int RF_MAX_GRID = 2048;     // workgroups; the waves stride over the selection beyond that
constexpr int MD_T = 512;             // threads of a key frame's workgroup
constexpr int MD_MAX = ORBM_MEDIAN_MAX_STRIDE;

// result slots of the refresh
enum { R_DONE = 0, R_INVALID = 1, R_NONE = 2, R_LONG = 3, R_DROPPED = 4, R_ALL_BAD = 5, R_REF_UNSEEN = 6, R_REF_MISSING = 7 };

__device__ __forceinline__ int lowest(u64 m) { return __ffsll((long long)m) - 1; }
__device__ __forceinline__ float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// O_w = -(R^T t) of key frame k, pose rounded to float first (Pose.cpp:12-14)
__device__ __forceinline__ void camera_centre(const double *__restrict__ pose_R, const double *__restrict__ pose_t, int k, float (&O)[3])
{
    float R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (float)pose_R[9 * (size_t)k + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = (float)pose_t[3 * (size_t)k + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) O[i] = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
}

// observation j of a list that ends at `end`: usable (both indices in range) and of a key frame that is not bad?
// Its own, not map_usable of orbm_map.h: the refresh reads descriptors, not slots, so the bound is kf.d_n[k] with no stride.
__device__ __forceinline__ bool good_observation(const orbm_kf_table &kf, const int32_t *__restrict__ obs_kf, const int32_t *__restrict__ obs_kp,
                                                 int j, int end, int &k, int &f)
{
    if (j >= end) return false;
    k = obs_kf[j], f = obs_kp[j];
    if (k < 0 || k >= kf.n_kf || f < 0 || f >= kf.d_n[k]) return false;
    return kf.d_bad[k] == 0;
}

// the tile: descriptors of the observations t0 .. t0 + 63 of the list, one per lane; returns the mask of the good ones
__device__ __forceinline__ u64 load_tile(const orbm_kf_table &kf, const int32_t *__restrict__ obs_kf, const int32_t *__restrict__ obs_kp, int t0,
                                         int end, int lane, uint32_t (*tile)[8])
{
    int k = 0, f = 0;
    const bool good = good_observation(kf, obs_kf, obs_kp, t0 + lane, end, k, f);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the reads of the tile before this one are done
    __builtin_amdgcn_wave_barrier();
    if (good) {
        const uint32_t *src = (const uint32_t *)(kf.d_desc[k] + (size_t)f * 32);
#pragma unroll
        for (int w = 0; w < 8; ++w) tile[lane][w] = src[w];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return __ballot(good);
}

__global__ void k_refresh_clear(int32_t *__restrict__ covis, int n_kf, int32_t *__restrict__ result)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (covis && i < n_kf) covis[i] = 0;
    if (i < 8) result[i] = 0;
}

__global__ __launch_bounds__(RF_T) void k_refresh(const orbm_kf_table kf, const int32_t *__restrict__ sel, int n_sel,
                                                  const float *__restrict__ points, const uint8_t *__restrict__ valid, int cap_points,
                                                  float *__restrict__ normals, float *__restrict__ min_dist, float *__restrict__ max_dist,
                                                  uint32_t *__restrict__ desc, const int32_t *__restrict__ obs_off,
                                                  const int32_t *__restrict__ obs_kf, const int32_t *__restrict__ obs_kp, int n_obs,
                                                  const int32_t *__restrict__ ref_kf, float max_scale_factor, int kf_self,
                                                  int32_t *__restrict__ covis, int32_t *__restrict__ result)
{
    __shared__ uint32_t s_tile[RF_WAVES][64][8];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t(*tile)[8] = s_tile[wave];
    int count[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // constant indices only: registers
    const int n_waves = gridDim.x * RF_WAVES;
    for (int e = blockIdx.x * RF_WAVES + wave; e < n_sel; e += n_waves) {
        const int p = __builtin_amdgcn_readfirstlane(sel[e]);
        if (p < 0 || p >= cap_points) continue;
        if (!valid[p]) { ++count[R_INVALID]; continue; }          // MapPoint.cpp:50, :108
        int b = __builtin_amdgcn_readfirstlane(obs_off[p]), end = __builtin_amdgcn_readfirstlane(obs_off[p + 1]);
        if (b < 0 || end < b || end > n_obs) b = end = 0;         // offsets that do not describe a list: an empty one
        const float px = points[3 * (size_t)p], py = points[3 * (size_t)p + 1], pz = points[3 * (size_t)p + 2];
        const int rk = __builtin_amdgcn_readfirstlane(ref_kf[p]);
        // ---- walk 1: counts, covisibility, the sum of the unit directions in CSR order, the reference key frame's feature
        float sx = 0.f, sy = 0.f, sz = 0.f;
        int n = 0, n_good = 0, first_good = -1, ref_kp = -1;
        for (int c0 = b; c0 < end; c0 += 64) {
            const int j = c0 + lane;
            bool ok = false, good = false;
            int k = -1, f = -1;
            float dx = 0.f, dy = 0.f, dz = 0.f;
            if (j < end) {
                k = obs_kf[j], f = obs_kp[j];
                if (k >= 0 && k < kf.n_kf && f >= 0 && f < kf.d_n[k]) {
                    ok = true;
                    good = kf.d_bad[k] == 0;
                    float O[3];
                    camera_centre(kf.d_pose_R, kf.d_pose_t, k, O);
                    const float vx = px - O[0], vy = py - O[1], vz = pz - O[2];
                    const float len = sqrtf((vx * vx + vy * vy) + vz * vz);
                    const bool unit = len > 0.f;                  // Eigen's normalized()
                    dx = unit ? vx / len : vx, dy = unit ? vy / len : vy, dz = unit ? vz / len : vz;
                    if (covis && k != kf_self) atomicAdd(&covis[k], 1);   // KeyFrame.cpp:237-240
                }
            }
            const u64 m_ok = __ballot(ok), m_good = __ballot(good), m_ref = __ballot(ok && k == rk);
            count[R_DROPPED] += min(end - c0, 64) - (int)__popcll(m_ok);
            n += (int)__popcll(m_ok);
            n_good += (int)__popcll(m_good);
            if (first_good < 0 && m_good) first_good = c0 + lowest(m_good);
            if (ref_kp < 0 && m_ref) ref_kp = __builtin_amdgcn_readlane(f, lowest(m_ref));
            for (u64 m = m_ok; m; m &= m - 1) {                    // sumDirection += ... in list order (MapPoint.cpp:57-63)
                const int l = lowest(m);
                sx = sx + lane_value(dx, l), sy = sy + lane_value(dy, l), sz = sz + lane_value(dz, l);
            }
        }
        // ---- what the reference cannot do is found before anything is written
        if (n == 0) { ++count[R_NONE]; continue; }
        if (n > ORBM_MAX_LIST) { ++count[R_LONG]; continue; }
        if (rk < 0 || rk >= kf.n_kf) { ++count[R_REF_MISSING]; continue; }
        if (ref_kp < 0) {                                          // obs[refKeyFrame] through map::operator[]: feature 0
            if (kf.d_n[rk] < 1) { ++count[R_REF_MISSING]; continue; }
            ref_kp = 0;
            ++count[R_REF_UNSEEN];
        }
        ++count[R_DONE];
        if (lane == 0) {
            float O[3];
            camera_centre(kf.d_pose_R, kf.d_pose_t, rk, O);
            const float vx = px - O[0], vy = py - O[1], vz = pz - O[2];
            const float dist = sqrtf((vx * vx + vy * vy) + vz * vz);
            const float size = *(const float *)((const char *)kf.d_kps[rk] + (size_t)ref_kp * sizeof(orbx_kp) + offsetof(orbx_kp, size));
            const float span = dist * size, fn = (float)n;
            normals[3 * (size_t)p] = sx / fn, normals[3 * (size_t)p + 1] = sy / fn, normals[3 * (size_t)p + 2] = sz / fn;
            max_dist[p] = 1.2f * span;
            min_dist[p] = 0.8f * (span / max_scale_factor);
        }
        if (n_good == 0) { ++count[R_ALL_BAD]; continue; }         // MapPoint.cpp:122
        // ---- walk 2: the good row of least median distance, first in the list on ties (MapPoint.cpp:124-146)
        int best = first_good;                                     // one or two good rows: every median is the self distance 0
        if (n_good > 2) {
            const bool one_tile = end - b <= 64;
            const int kth = (n_good - 1) / 2;
            u64 m_tile = 0;
            if (one_tile) m_tile = load_tile(kf, obs_kf, obs_kp, b, end, lane, tile);
            int my_median = 256, my_row = 0x7fffffff;
            for (int r0 = b; r0 < end; r0 += 64) {
                int k = 0, f = 0;
                const bool row = good_observation(kf, obs_kf, obs_kp, r0 + lane, end, k, f);
                if (!__ballot(row)) continue;
                uint32_t di[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                if (row) {
                    const uint32_t *src = (const uint32_t *)(kf.d_desc[k] + (size_t)f * 32);
#pragma unroll
                    for (int w = 0; w < 8; ++w) di[w] = src[w];
                }
                int lo = 0, hi = 256;                              // the least v with #{j : d_ij <= v} > kth
                for (int step = 0; step < 9; ++step) {             // 257 values
                    const int mid = (lo + hi) >> 1;
                    int cnt = 0;
                    for (int t0 = b; t0 < end; t0 += 64) {
                        if (!one_tile) m_tile = load_tile(kf, obs_kf, obs_kp, t0, end, lane, tile);
                        for (u64 m = m_tile; m; m &= m - 1) {
                            const int j = lowest(m);
                            int d = 0;
#pragma unroll
                            for (int w = 0; w < 8; ++w) d += __popc(di[w] ^ tile[j][w]);
                            cnt += d <= mid;
                        }
                    }
                    if (lo < hi) {
                        if (cnt > kth) hi = mid; else lo = mid + 1;
                    }
                }
                if (row && lo < my_median) my_median = lo, my_row = r0 + lane;   // rows ascend per lane: strict '<' keeps the first
            }
            const int median = wave_min(my_median);
            const int at = wave_min(my_median == median ? my_row : 0x7fffffff);
            if (median < 256) best = __builtin_amdgcn_readfirstlane(at);   // bestMedian starts at 256 with a strict '<' (:138-146)
        }
        if (lane < 8) {
            const int k = obs_kf[best], f = obs_kp[best];
            desc[8 * (size_t)p + lane] = ((const uint32_t *)(kf.d_desc[k] + (size_t)f * 32))[lane];
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (count[c]) atomicAdd(&result[c], count[c]);
    }
}

// KeyFrame::computeSceneMedianDepth: a workgroup per key frame; the depths become order-preserving keys in LDS and the element
// count / 2 of the ascending order is found by a radix select, most significant byte first (the value a sort would return).
__global__ __launch_bounds__(MD_T) void k_median_depth(const double *__restrict__ pose_R, const double *__restrict__ pose_t,
                                                       const int32_t *__restrict__ slots, const int32_t *__restrict__ n_slots, int stride,
                                                       const float *__restrict__ points, int cap_points, int cur,
                                                       float *__restrict__ median, int32_t *__restrict__ count, float *__restrict__ baseline)
{
    __shared__ uint32_t s_key[MD_MAX];
    __shared__ int s_hist[256];
    __shared__ int s_wave[4];
    __shared__ int s_n, s_digit, s_rank;
    const int k = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const float r0 = (float)pose_R[9 * (size_t)k + 6], r1 = (float)pose_R[9 * (size_t)k + 7], r2 = (float)pose_R[9 * (size_t)k + 8];
    const float t2 = (float)pose_t[3 * (size_t)k + 2];
    const int n = min(max(n_slots[k], 0), stride);               // <= MD_MAX: the host checked stride
    for (int i = tid; i < n; i += MD_T) {
        const int s = slots[(size_t)k * stride + i];
        if (s < 0 || s >= cap_points) continue;                  // mapPoints[i] != nullptr (KeyFrame.cpp:168)
        const float z = ((r0 * points[3 * (size_t)s] + r1 * points[3 * (size_t)s + 1]) + r2 * points[3 * (size_t)s + 2]) + t2;
        const uint32_t u = __float_as_uint(z);
        s_key[atomicAdd(&s_n, 1)] = (u >> 31) ? ~u : (u | 0x80000000u);
    }
    __syncthreads();
    const int cnt = s_n;
    if (tid == 0) {
        count[k] = cnt;
        if (baseline && cur >= 0) {                               // LocalMapping.cpp:163
            float Oc[3], Ok[3];
            camera_centre(pose_R, pose_t, cur, Oc);
            camera_centre(pose_R, pose_t, k, Ok);
            const float vx = Oc[0] - Ok[0], vy = Oc[1] - Ok[1], vz = Oc[2] - Ok[2];
            baseline[k] = sqrtf((vx * vx + vy * vy) + vz * vz);
        }
        if (cnt == 0) median[k] = __uint_as_float(0x7fc00000u);  // the reference reads past an empty vector
    }
    if (cnt == 0) return;
    uint32_t prefix = 0, known = 0;
    int rank = cnt / 2;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < cnt; i += MD_T) {
            const uint32_t key = s_key[i];
            if ((key & known) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        const int h = tid < 256 ? s_hist[tid] : 0;
        int incl = h;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if ((tid & 63) >= o) incl += t;
        }
        if (tid < 256 && (tid & 63) == 63) s_wave[tid >> 6] = incl;
        __syncthreads();
        if (tid < 256) {
            for (int w = 0; w < (tid >> 6); ++w) incl += s_wave[w];
            if (incl - h <= rank && rank < incl) s_digit = tid, s_rank = rank - (incl - h);   // one bin: it is not empty
        }
        __syncthreads();
        prefix |= (uint32_t)s_digit << shift;
        known |= 255u << shift;
        rank = s_rank;
        __syncthreads();                                          // s_digit, s_rank and s_hist are rewritten by the next byte
    }
    if (tid == 0) median[k] = __uint_as_float((prefix >> 31) ? (prefix & 0x7fffffffu) : ~prefix);
}

} // namespace

extern "C" int orbm_refresh_points_device(orbm_t *h, const orbm_kf_table *kf, const int32_t *d_sel, int n_sel, const float *d_points,
                                          const uint8_t *d_valid, int cap_points, float *d_normals, float *d_min_dist, float *d_max_dist,
                                          uint8_t *d_desc, const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp,
                                          int n_obs, const int32_t *d_ref_kf, float max_scale_factor, int kf_self, int32_t *d_covis,
                                          int32_t *d_result, void *stream)
{
    if (!kf || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (kf->n_kf < 0 || n_sel < 0 || cap_points < 0 || n_obs < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (kf->n_kf > 0 && (!kf->d_pose_R || !kf->d_pose_t || !kf->d_bad || !kf->d_kps || !kf->d_desc || !kf->d_n))
        return orbx_set_error(ORBX_E_ARG, "null key-frame table array");
    if (n_sel > 0 && !d_sel) return orbx_set_error(ORBX_E_ARG, "null selection");
    if (cap_points > 0 && (!d_points || !d_valid || !d_normals || !d_min_dist || !d_max_dist || !d_desc || !d_obs_off || !d_ref_kf))
        return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if (n_obs > 0 && (!d_obs_kf || !d_obs_kp)) return orbx_set_error(ORBX_E_ARG, "null observation array");
    if (((uintptr_t)d_desc) & 3) return orbx_set_error(ORBX_E_ARG, "descriptor arrays must be 4-byte aligned");
    if (int rc = orbm_check_kf_rows(kf->d_kps, kf->d_desc)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    const int n_clear = std::max(d_covis ? kf->n_kf : 0, 8);
    hipLaunchKernelGGL(k_refresh_clear, dim3((n_clear + 255) / 256), dim3(256), 0, s, d_covis, kf->n_kf, d_result);
    ORB_TRY(hipGetLastError());
    if (n_sel == 0 || cap_points == 0) return ORBX_OK;
    const int grid = std::min((n_sel + RF_WAVES - 1) / RF_WAVES, RF_MAX_GRID);
    hipLaunchKernelGGL(k_refresh, dim3(grid), dim3(RF_T), 0, s, *kf, d_sel, n_sel, d_points, d_valid, cap_points, d_normals, d_min_dist,
                       d_max_dist, (uint32_t *)d_desc, d_obs_off, d_obs_kf, d_obs_kp, n_obs, d_ref_kf, max_scale_factor, kf_self, d_covis,
                       d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_scene_median_depth_device(orbm_t *h, int n_kf, const double *d_pose_R, const double *d_pose_t, const int32_t *d_slots,
                                              const int32_t *d_n, int stride, const float *d_points, int cap_points, int cur,
                                              float *d_median, int32_t *d_count, float *d_baseline, void *stream)
{
    if (n_kf < 0 || stride < 0 || cap_points < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (n_kf > 0 && (!d_pose_R || !d_pose_t || !d_n || !d_median || !d_count)) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (n_kf > 0 && stride > 0 && !d_slots) return orbx_set_error(ORBX_E_ARG, "null slot array");
    if (cap_points > 0 && !d_points) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if (cur >= n_kf && d_baseline) return orbx_set_error(ORBX_E_ARG, "cur is not a key frame of the call");
    if (int rc = orbm_check_stride(stride)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    if (n_kf == 0) return ORBX_OK;
    hipLaunchKernelGGL(k_median_depth, dim3(n_kf), dim3(MD_T), 0, s, d_pose_R, d_pose_t, d_slots, d_n, stride, d_points, cap_points, cur,
                       d_median, d_count, d_baseline);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
