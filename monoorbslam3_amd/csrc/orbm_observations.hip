// The observation index of the device-resident map-point table and the one step of LocalMapping::Run that reads it and had no
// device form (include/orbm.h, "Observations built and key frames culled on the device"):
//   orbm_build_observations_device   the CSR the refresh reads (d_obs_off / d_obs_kf / d_obs_kp), rebuilt from the key frames' slot
//                                    arrays: what MapPoint::addObservation / eraseObservation / setBad and KeyFrame::setBad leave
//                                    in every point's `observations` (MapPoint.cpp:182-226, KeyFrame.cpp:402-412)
//   orbm_cull_keyframes_device       LocalMapping::KeyFrameCulling (LocalMapping.cpp:318-372) with the cascade of KeyFrame::setBad
//
// The build.  THE SLOT ARRAYS ARE THE TRUTH, the CSR is their inverse: count -> scan -> scatter -> sort, five small launches.
//   k_obs_clear     d_obs_off and d_result to zero
//   k_obs_slots<0>  a thread per slot: d_obs_off[p + 1] += 1 for an observation of row p; the two skip counters
//   k_obs_scan      ONE workgroup: the exclusive scan of d_obs_off in place, which leaves the START of row p in d_obs_off[p + 1];
//                   n_obs, the longest list, the lists over 1024; the overflow test.  On overflow every offset becomes 0, the
//                   flag is set and the two kernels below return at once
//   k_obs_slots<1>  a thread per slot again: pos = atomicAdd(&d_obs_off[p + 1], 1) -- the cursor of row p IS its slot of the offset
//                   array, which ends as the END of row p = the start of row p + 1 = the final value: no scratch -- and the key
//                   k * ORBM_MEDIAN_MAX_STRIDE + i goes to d_obs_kp[pos], in whichever order the atomics came
//   k_obs_sort      a wave per row, four to a workgroup (the refresh's shape): every entry's rank = the number of smaller keys of
//                   its list (the keys are distinct), read lane by lane from tiles of 64; the key goes to d_obs_kf[start + rank]
//                   while d_obs_kp is only read, then the wave splits the sorted keys into (k, i) in place and looks for equal
//                   neighbours k (a key frame twice).  A list of n entries costs n * ceil(n / 64) lane reads.
// The order an atomic won never reaches the output: the bytes are those of a sort on distinct keys.
//
// The culling.  ONE launch of ONE workgroup of 1024 threads that walks the candidates in order, a thread per slot of the candidate
// and workgroup barriers between the phases -- the candidates are sequential by definition (each sees the slots, d_valid and d_bad
// the ones before it left), the slots of one candidate are independent, and at <= 23 candidates x <= 8192 slots x short lists the
// work is latency, not throughput (the shape of k_project / k_triangulate).  A point named by two slots of the culled key frame
// (which the reference cannot have) is cascaded ONCE: the first thread to set the point's bit in a claim mask of one bit per table
// row (dynamic LDS, <= 64 KB at 524288 rows) owns it; whichever wins, the owner does the same work, so the bytes do not depend on it.
// No scratch memory, no handle scratch, no allocation, no host wait.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <algorithm>
#include <string>

#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orbm_internal.h"
#include "orbm_map.h"

namespace {

typedef unsigned long long u64;

constexpr int OB_T = 256;               // threads of the per-slot kernels
constexpr int OB_MAX_GRID = 2048;       // workgroups; the threads stride beyond that
constexpr int OB_SCAN_T = 1024;         // the scan's one workgroup
constexpr int OB_WAVES = 4;             // rows in flight per workgroup of the sort
constexpr int OB_MAX_KF = 262143;       // the sort key k << MAP_KEY_SHIFT | i fits in int32
constexpr int CL_T = 1024;              // the culling's one workgroup
constexpr int CL_MAX_RECENT = 32;

// result slots of the build and of the culling
enum { B_NOBS = 0, B_OVERFLOW = 1, B_INVALID = 2, B_BAD_KF = 3, B_LONGEST = 4, B_TWICE = 5, B_LONG = 6 };
enum { C_CULLED = 0, C_KEPT = 1, C_SKIPPED = 2, C_POINTS_BAD = 3, C_CLEARED = 4, C_REASSIGNED = 5, C_DROPPED = 6 };

__global__ void k_obs_clear(int32_t *__restrict__ off, int n, int32_t *__restrict__ result)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    for (int i = t; i < n; i += gridDim.x * blockDim.x) off[i] = 0;
    if (t < 8) result[t] = 0;
}

// SCATTER = false: count the observations of every row into off[p + 1]; true: place their keys behind the rows' cursors
template <bool SCATTER>
__global__ __launch_bounds__(OB_T) void k_obs_slots(int n_kf, const int32_t *__restrict__ n_slots, const uint8_t *__restrict__ bad,
                                                    const int32_t *__restrict__ slots, int stride, const uint8_t *__restrict__ valid,
                                                    int cap_points, int cap_obs, int32_t *__restrict__ off, int32_t *__restrict__ keys,
                                                    int32_t *__restrict__ result)
{
    if (SCATTER && result[B_OVERFLOW]) return;
    const long long total = (long long)n_kf * stride;
    int invalid = 0, bad_kf = 0;
    for (long long t = (long long)blockIdx.x * OB_T + threadIdx.x; t < total; t += (long long)gridDim.x * OB_T) {
        const int k = (int)(t / stride), i = (int)(t - (long long)k * stride);
        if (i >= n_slots[k]) continue;
        const int p = slots[t];
        if (p < 0 || p >= cap_points) continue;                    // no map point
        if (!valid[p]) { ++invalid; continue; }                    // a bad point has no observations (MapPoint.cpp:217)
        if (bad[k]) { ++bad_kf; continue; }                        // KeyFrame::setBad erased them (KeyFrame.cpp:410)
        if (SCATTER) {
            const int pos = atomicAdd(&off[p + 1], 1);
            if ((unsigned)pos < (unsigned)cap_obs) keys[pos] = (k << MAP_KEY_SHIFT) | i;   // the count said so; never past the array
        } else {
            atomicAdd(&off[p + 1], 1);
        }
    }
    if (SCATTER) return;
    block_add(result, {B_INVALID, B_BAD_KF}, {invalid, bad_kf});
}

// off[0] = 0, off[p + 1] = the count of row p  ->  off[j] = the sum of the entries below j: row p starts at off[p + 1]
__global__ __launch_bounds__(OB_SCAN_T) void k_obs_scan(int32_t *__restrict__ off, int cap_points, int cap_obs, int32_t *__restrict__ result)
{
    __shared__ int s_wave[OB_SCAN_T / 64];
    __shared__ int s_longest, s_long;
    const int tid = threadIdx.x, n = cap_points + 1;
    const int chunk = (n + OB_SCAN_T - 1) / OB_SCAN_T;
    const int j0 = min(tid * chunk, n), j1 = min(j0 + chunk, n);
    if (tid == 0) s_longest = 0, s_long = 0;
    __syncthreads();
    int sum = 0, longest = 0, n_long = 0;
    for (int j = j0; j < j1; ++j) {
        const int c = off[j];
        sum += c;
        longest = max(longest, c);
        n_long += c > ORBM_MAX_LIST;
    }
    const int incl = wave_scan(sum);
    if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
    block_add(&s_long, 0, n_long);
    longest = wave_max(longest);
    if ((tid & 63) == 0) atomicMax(&s_longest, longest);
    __syncthreads();
    int before = incl - sum, total = 0;
    for (int w = 0; w < OB_SCAN_T / 64; ++w) {
        if (w < (tid >> 6)) before += s_wave[w];
        total += s_wave[w];
    }
    const bool overflow = total > cap_obs;
    if (tid == 0) {
        result[B_NOBS] = total;
        result[B_OVERFLOW] = overflow;
        result[B_LONGEST] = s_longest;
        result[B_LONG] = s_long;
    }
    for (int j = j0; j < j1; ++j) {
        const int c = off[j];
        off[j] = overflow ? 0 : before;
        before += c;
    }
}

__global__ __launch_bounds__(OB_WAVES * 64) void k_obs_sort(const int32_t *__restrict__ off, int cap_points, int32_t *obs_kf, int32_t *obs_kp,
                                                            int cap_obs, int32_t *__restrict__ result)
{
    if (result[B_OVERFLOW]) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_waves = gridDim.x * OB_WAVES;
    int twice = 0;
    for (int p = blockIdx.x * OB_WAVES + wave; p < cap_points; p += n_waves) {
        const int b = __builtin_amdgcn_readfirstlane(off[p]), end = __builtin_amdgcn_readfirstlane(off[p + 1]);
        if (b < 0 || end <= b || end > cap_obs) continue;
        const int n = end - b;
        // ---- every key's rank among the keys of its list; the sorted keys go to obs_kf, obs_kp is only read
        for (int t0 = b; t0 < end; t0 += 64) {
            const int j = t0 + lane;
            const int mine = j < end ? obs_kp[j] : 0x7fffffff;
            int rank = 0;
            if (n <= 64) {
                for (int l = 0; l < n; ++l) rank += __builtin_amdgcn_readlane(mine, l) < mine;
            } else {
                for (int u0 = b; u0 < end; u0 += 64) {
                    const int other = u0 + lane < end ? obs_kp[u0 + lane] : 0x7fffffff;
                    const int m = min(64, end - u0);
                    for (int l = 0; l < m; ++l) rank += __builtin_amdgcn_readlane(other, l) < mine;
                }
            }
            if (j < end) obs_kf[b + rank] = mine;
        }
        __threadfence_block();                                     // the wave's own stores, before its lanes read each other's
        // ---- (k, i) in place; a key frame twice shows as equal neighbours
        int carry = -1;
        bool dup = false;
        for (int t0 = b; t0 < end; t0 += 64) {
            const int j = t0 + lane;
            const int key = j < end ? obs_kf[j] : 0;
            const int k = key >> MAP_KEY_SHIFT;
            int prev = __shfl_up(k, 1);
            if (lane == 0) prev = carry;
            carry = __builtin_amdgcn_readlane(k, 63);
            if (j < end) {
                obs_kf[j] = k;
                obs_kp[j] = key & (ORBM_MEDIAN_MAX_STRIDE - 1);
                dup |= j > b && prev == k;
            }
        }
        twice += __ballot(dup) != 0;
    }
    if (lane == 0 && twice) atomicAdd(&result[B_TWICE], twice);
}

// ---- the culling -----------------------------------------------------------------------------------------------------------------
struct CullArgs {
    int32_t recent[CL_MAX_RECENT];
    double timestamps[CL_MAX_RECENT];
    int n_recent, first_kf, th_obs;
    double redundant_ratio, max_gap;
};

// the map (orbm_map.h) and the key-frame table's key points, for the octaves
struct CullView : MapView {
    const void *const *kps;
};

__device__ __forceinline__ int cull_octave(const CullView &v, int k, int i)
{
    return *(const int32_t *)((const char *)v.kps[k] + (size_t)i * sizeof(orbx_kp) + offsetof(orbx_kp, octave));
}

__global__ __launch_bounds__(CL_T) void k_cull(const CullArgs a, const CullView v, uint8_t *bad, int32_t *ref_kf, int32_t *code, int32_t *num_mp,
                                               int32_t *num_redundant, int32_t *result)
{
    extern __shared__ uint32_t s_claim[];                          // bit p: row p's cascade has an owner
    __shared__ int s_count[8];
    __shared__ int s_cand[2];                                      // numMP and the redundant slots of the candidate
    const int tid = threadIdx.x;
    bits_zero<CL_T>(s_claim, v.cap_points);
    if (tid < 8) s_count[tid] = 0;
    if (tid < a.n_recent) code[tid] = -1, num_mp[tid] = 0, num_redundant[tid] = 0;
    __syncthreads();
    int dropped = 0, points_bad = 0, cleared = 0, reassigned = 0;   // per thread, summed at the end
    int culled = 0, kept = 0, skipped = 0;                          // the same in every thread
    for (int j = tid; j < v.n_obs; j += CL_T) {
        int k, i;
        dropped += !map_entry(v, j, k, i);
    }
    int last = 0;
    for (int idx = 1; idx < a.n_recent - 1; ++idx) {
        const int c = a.recent[idx];
        int skip = 0;                                              // LocalMapping.cpp:329-331, in the order of the `||`
        if (c == a.first_kf) skip = 1;
        else if (a.timestamps[idx + 1] - a.timestamps[last] > a.max_gap) skip = 2;
        if (skip) {
            if (tid == 0) code[idx] = skip;
            ++skipped;
            continue;
        }
        if (tid == 0) s_cand[0] = 0, s_cand[1] = 0;
        __syncthreads();
        const int n_c = map_slots(v, c);
        int32_t *mine = map_slot(v, c, 0);
        // ---- numMP and the redundant slots (:339-362)
        int mp = 0, red = 0;
        for (int i = tid; i < n_c; i += CL_T) {
            const int p = mine[i];
            if (p < 0 || p >= v.cap_points || !v.valid[p]) continue;
            ++mp;
            int b, e, live = 0, others = 0;
            map_list(v, p, b, e);
            const int level = cull_octave(v, c, i);
            for (int j = b; j < e; ++j) {
                int k2, i2;
                if (!map_entry(v, j, k2, i2) || !map_live(v, k2, i2, p)) continue;
                ++live;                                            // getNumObs()
                others += k2 != c && cull_octave(v, k2, i2) <= level + 1;
            }
            red += live > a.th_obs && others >= a.th_obs;          // the break of :355 only caps the count
        }
        block_add(s_cand, {0, 1}, {mp, red});
        __syncthreads();
        mp = s_cand[0], red = s_cand[1];
        __syncthreads();                                           // read by everyone before the next candidate resets them
        if (tid == 0) num_mp[idx] = mp, num_redundant[idx] = red;
        if (!((double)red > a.redundant_ratio * (double)mp)) {     // :364
            if (tid == 0) code[idx] = 0;
            ++kept;
            last = idx;
            continue;
        }
        // ---- KeyFrame::setBad (KeyFrame.cpp:402-418): eraseObservation for every point, once per point
        if (tid == 0) code[idx] = 3, bad[c] = 1;
        ++culled;
        __syncthreads();
        for (int i = tid; i < n_c; i += CL_T) {
            const int p = mine[i];
            if (p < 0 || p >= v.cap_points || !v.valid[p]) continue;
            if (!bit_set(s_claim, p)) continue;                    // another slot of c names p and owns it
            int b, e, left = 0, first = -1;
            map_list(v, p, b, e);
            for (int j = b; j < e; ++j) {
                int k2, i2;
                if (!map_entry(v, j, k2, i2) || k2 == c || !map_live(v, k2, i2, p)) continue;
                if (left++ == 0) first = k2;
            }
            if (ref_kf[p] == c && left > 0) ref_kf[p] = first, ++reassigned;   // observations.begin() (MapPoint.cpp:198-199)
            if (left > 2) continue;
            v.valid[p] = 0;                                        // MapPoint::setBad (:202, :210-226)
            ++points_bad;
            for (int j = b; j < e; ++j) {
                int k2, i2;
                if (!map_entry(v, j, k2, i2) || k2 == c || !map_live(v, k2, i2, p)) continue;
                *map_slot(v, k2, i2) = -1;                         // KeyFrame::eraseMapPoint
                ++cleared;
            }
        }
        __syncthreads();
        for (int i = tid; i < n_c; i += CL_T) {                    // map_points.clear() (KeyFrame.cpp:418); the claims go with it
            const int p = mine[i];
            if (p >= 0 && p < v.cap_points) atomicAnd(&s_claim[p >> 5], ~(1u << (p & 31)));
            mine[i] = -1;
        }
        __syncthreads();
    }
    block_add(s_count, {C_DROPPED, C_POINTS_BAD, C_CLEARED, C_REASSIGNED}, {dropped, points_bad, cleared, reassigned});
    if (tid == 0) s_count[C_CULLED] = culled, s_count[C_KEPT] = kept, s_count[C_SKIPPED] = skipped;
    __syncthreads();
    if (tid < 8) result[tid] = s_count[tid];
}

} // namespace

extern "C" int orbm_build_observations_device(orbm_t *h, int n_kf, const int32_t *d_n, const uint8_t *d_bad, const int32_t *d_slots,
                                              int stride, const uint8_t *d_valid, int cap_points, int cap_obs, int32_t *d_obs_off,
                                              int32_t *d_obs_kf, int32_t *d_obs_kp, int32_t *d_result, void *stream)
{
    if (!d_obs_off || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (int rc = orbm_check_map(n_kf, d_n, d_bad, d_slots, stride, d_valid, cap_points, d_obs_off, d_obs_kf, d_obs_kp, cap_obs)) return rc;   // the CSR to be
    if (int rc = orbm_check_stride(stride)) return rc;
    if (n_kf > OB_MAX_KF) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than 262143 key frames in one call");
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    const int n_off = cap_points + 1;
    hipLaunchKernelGGL(k_obs_clear, dim3(std::min((n_off + 255) / 256, OB_MAX_GRID)), dim3(256), 0, s, d_obs_off, n_off, d_result);
    ORB_TRY(hipGetLastError());
    const long long total = (long long)n_kf * stride;
    const int grid = (int)std::min<long long>((total + OB_T - 1) / OB_T, OB_MAX_GRID);
    if (total > 0 && cap_points > 0) {
        hipLaunchKernelGGL(k_obs_slots<false>, dim3(grid), dim3(OB_T), 0, s, n_kf, d_n, d_bad, d_slots, stride, d_valid, cap_points, cap_obs,
                           d_obs_off, (int32_t *)nullptr, d_result);
        ORB_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_obs_scan, dim3(1), dim3(OB_SCAN_T), 0, s, d_obs_off, cap_points, cap_obs, d_result);
    ORB_TRY(hipGetLastError());
    if (total == 0 || cap_points == 0 || cap_obs == 0) return ORBX_OK;
    hipLaunchKernelGGL(k_obs_slots<true>, dim3(grid), dim3(OB_T), 0, s, n_kf, d_n, d_bad, d_slots, stride, d_valid, cap_points, cap_obs,
                       d_obs_off, d_obs_kp, d_result);
    ORB_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_obs_sort, dim3(std::min((cap_points + OB_WAVES - 1) / OB_WAVES, OB_MAX_GRID)), dim3(OB_WAVES * 64), 0, s, d_obs_off,
                       cap_points, d_obs_kf, d_obs_kp, cap_obs, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_cull_keyframes_device(orbm_t *h, const orbm_kf_table *kf, uint8_t *d_bad, int32_t *d_slots, int stride, uint8_t *d_valid,
                                          int cap_points, const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp,
                                          int n_obs, int32_t *d_ref_kf, const int32_t *recent, const double *timestamps, int n_recent,
                                          int first_kf, int th_obs, double redundant_ratio, double max_gap, int32_t *d_code,
                                          int32_t *d_num_mp, int32_t *d_num_redundant, int32_t *d_result, void *stream)
{
    if (!kf || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    MapView m;
    if (int rc = orbm_map_view(&m, kf->n_kf, kf->d_n, d_bad, d_slots, stride, d_valid, cap_points, d_obs_off, d_obs_kf, d_obs_kp, n_obs)) return rc;
    if (n_recent < 0 || th_obs < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (kf->n_kf > 0 && !kf->d_kps) return orbx_set_error(ORBX_E_ARG, "null key-frame array");
    if (cap_points > 0 && !d_ref_kf) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if (n_recent > 0 && (!recent || !timestamps || !d_code || !d_num_mp || !d_num_redundant))
        return orbx_set_error(ORBX_E_ARG, "null candidate array");
    if (int rc = orbm_check_kf_rows(kf->d_kps)) return rc;
    if (first_kf < -1 || first_kf >= kf->n_kf) return orbx_set_error(ORBX_E_ARG, "first_kf is neither -1 nor a key frame of the table");
    if (n_recent > CL_MAX_RECENT) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than 32 recent key frames in one call");
    if (int rc = orbm_check_stride(stride)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    for (int i = 0; i < n_recent; ++i)
        if (recent[i] < 0 || recent[i] >= kf->n_kf) return orbx_set_error(ORBX_E_ARG, "an entry of recent is not a key frame of the table");
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    CullArgs a = {};
    for (int i = 0; i < n_recent; ++i) a.recent[i] = recent[i], a.timestamps[i] = timestamps[i];
    a.n_recent = n_recent, a.first_kf = first_kf, a.th_obs = th_obs, a.redundant_ratio = redundant_ratio, a.max_gap = max_gap;
    const size_t claim_bytes = (size_t)((cap_points + 31) >> 5) * 4;   // <= 64 KB
    if (claim_bytes + 1024 > 64 * 1024) ORB_TRY(orbx_lds_opt_in((const void *)k_cull, claim_bytes));   // with the static 48 B: past 64 KB
    hipLaunchKernelGGL(k_cull, dim3(1), dim3(CL_T), claim_bytes, s, a, CullView{m, kf->d_kps}, d_bad, d_ref_kf, d_code, d_num_mp, d_num_redundant, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
