// The start of a mapper step on the device-resident map (include/orbm.h, "Key frames inserted and recent map points culled on the device"):
//   orbm_insert_keyframe_device       Tracking::createNewKeyFrame + the KeyFrame constructor (modules/Frontend/Tracking.cpp:578-588,
//                                     modules/BasicObject/KeyFrame.cpp:15-25) and the loop of LocalMapping::processNewKeyFrame
//                                     (modules/Frontend/LocalMapping.cpp:93-105): eraseMapPoint for a bad point, addObservation otherwise
//   orbm_register_new_points_device   the fields of the MapPoint constructor the triangulation does not write (MapPoint.cpp:18, :24-25)
//                                     and recent_map_points.push_back (LocalMapping.cpp:243-248)
//   orbm_cull_map_points_device       LocalMapping::MapPointCulling (:117-144) with the cascade of MapPoint::setBad (MapPoint.cpp:210-226)
//
// Each is ONE launch of ONE workgroup of 1024 threads that walks its input in tiles of 1024, the shape of k_cull / k_fuse_apply /
// k_local_map: a few hundred to a few thousand entries are latency, not throughput.  THE SLOT ARRAYS ARE THE TRUTH: the slot IS the
// observation, so addObservation is the store of the slot and setBad clears the slots that name the row; the CSR only says where they
// are and is never rewritten.  The insert counts the distinct rows of the new key frame and the culling tests its one premise (no row
// twice in the list) with a mask of one bit per table row in dynamic LDS (<= 64 KB at 524288 rows); a bit's first setter is counted,
// whoever it is, so no stored value depends on the order the atomics arrive in.  The culling compacts the kept entries in place behind
// a block scan: a tile's reads, a barrier, its writes, and a write never lands beyond the entry it came from.
// Integer only (the found ratio is one float division per entry).  No scratch memory, no handle scratch, no allocation, no host wait.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orbm_internal.h"

namespace {

typedef unsigned long long u64;

constexpr int KF_T = 1024;                       // the one workgroup of every kernel here
constexpr int KF_WAVES = KF_T / 64;

// d_result of the three calls, as the header lists them
enum { I_HELD = 0, I_INVALID = 2, I_RANGE = 3, I_TWICE = 4, I_CUT = 5 };
enum { G_ROWS = 0, G_REFUSED = 1, G_FROM = 2, G_TO = 3, G_RECENT = 4 };
enum { P_KEPT = 0, P_REFUSED = 1, P_BAD = 2, P_RATIO = 3, P_FEW = 4, P_AGED = 5, P_CLEARED = 6, P_DROPPED = 7 };

__device__ __forceinline__ int clamp_to(int x, int hi) { return min(max(x, 0), hi); }

// row K of the key-frame table, the arrays of orbm_kf_table as their owner holds them
struct KfRow {
    int K;
    u64 *pose_R, *pose_t;                        // doubles, moved as their 64 bits
    uint8_t *bad;
    const void **kps;
    const uint8_t **desc;
    int32_t *n;
};

__global__ __launch_bounds__(KF_T) void k_kf_insert(KfRow row, int32_t *slots, int stride, const uint8_t *__restrict__ valid, int cap_points,
                                                    const int32_t *__restrict__ frame_mp, int n2, const u64 *__restrict__ frame_R,
                                                    const u64 *__restrict__ frame_t, const void *frame_kps, const uint8_t *frame_desc,
                                                    int32_t *result)
{
    extern __shared__ uint32_t s_mask[];                           // bit p: a slot of K names row p
    __shared__ int s_count[8];
    const int tid = threadIdx.x;
    for (int w = tid; w < (cap_points + 31) >> 5; w += KF_T) s_mask[w] = 0;
    if (tid < 8) s_count[tid] = 0;
    __syncthreads();
    // ---- the KeyFrame constructor: T_cw, key points, descriptors, num_kps (KeyFrame.cpp:15-25)
    if (tid < 9) row.pose_R[(size_t)row.K * 9 + tid] = frame_R[tid];
    else if (tid < 12) row.pose_t[(size_t)row.K * 3 + (tid - 9)] = frame_t[tid - 9];
    else if (tid == 12) row.bad[row.K] = 0, row.n[row.K] = n2, row.kps[row.K] = frame_kps, row.desc[row.K] = frame_desc;
    // ---- map_points(frame->map_points), then LocalMapping.cpp:93-105 on every slot
    int32_t *mine = slots + (size_t)row.K * stride;
    const int m = min(n2, stride);
    int held = 0, distinct = 0, invalid = 0, range = 0;
    for (int i = tid; i < stride; i += KF_T) {
        int slot = -1;
        const int p = i < m ? frame_mp[i] : -1;
        if (p != -1) {
            if (p < 0 || p >= cap_points) ++range;
            else if (!valid[p]) ++invalid;                         // eraseMapPoint (:98)
            else slot = p, ++held, distinct += bit_set(s_mask, p);   // addObservation (:100) refuses a second slot; map_points keeps it
        }
        mine[i] = slot;
    }
    block_add(s_count, I_HELD, held), block_add(s_count, I_TWICE, held - distinct);
    block_add(s_count, I_INVALID, invalid), block_add(s_count, I_RANGE, range);
    if (tid == 0) s_count[I_CUT] = max(n2 - stride, 0);
    __syncthreads();
    if (tid < 8) result[tid] = s_count[tid];
}

__global__ __launch_bounds__(KF_T) void k_kf_register(const int32_t *n_points, int32_t *n_registered, int K, int kf_id, int cap_points,
                                                      int32_t *__restrict__ ref_kf, int32_t *__restrict__ first_kf,
                                                      int32_t *__restrict__ found, int32_t *__restrict__ visible,
                                                      int32_t *__restrict__ recent, int cap_recent, int32_t *n_recent, int32_t *result)
{
    const int tid = threadIdx.x;
    const int a = clamp_to(*n_registered, cap_points), b = clamp_to(*n_points, cap_points), r = clamp_to(*n_recent, cap_recent);
    __syncthreads();                                               // everyone has the three counters before one thread rewrites them
    const int refused = a > b ? 2 : (b - a > cap_recent - r ? 1 : 0);
    if (refused) {
        if (tid < 8) result[tid] = tid == G_REFUSED ? refused : tid == G_FROM ? a : tid == G_TO ? b : tid == G_RECENT ? r : 0;
        return;
    }
    for (int p = a + tid; p < b; p += KF_T) {
        ref_kf[p] = K, first_kf[p] = kf_id;                        // reference_kf(curKF), first_kf_id(curKF->id) (MapPoint.cpp:18)
        found[p] = 1, visible[p] = 1;                              // num_visible = num_found = 1 (:24-25)
        recent[r + (p - a)] = p;                                   // recent_map_points.push_back (LocalMapping.cpp:247)
    }
    if (tid == 0) *n_recent = r + (b - a), *n_registered = b;
    if (tid < 8) result[tid] = tid == G_ROWS ? b - a : tid == G_FROM ? a : tid == G_TO ? b : tid == G_RECENT ? r + (b - a) : 0;
}

// The map as orbm_build_observations_device takes and leaves it; slots and valid are written here.  This file keeps its own view, CSR
// rules and argument checks instead of those of orbm_map.h: with the shared ones the chain insert -> build -> cull -> register measured
// 4 % slower (tools/keyframe_latency.py, profiles/map_view_refactor_latency.txt) although k_kf_cull_points compiled to equivalent code
struct MapView {
    int n_kf, stride, cap_points, n_obs;
    const int32_t *kf_n, *obs_off, *obs_kf, *obs_kp;
    const uint8_t *bad;
    int32_t *slots;
    uint8_t *valid;
};

// CSR entry j: both indices usable?  (the culling's distrust)
__device__ __forceinline__ bool entry_ok(const MapView &m, int j, int &k, int &i)
{
    k = m.obs_kf[j], i = m.obs_kp[j];
    return k >= 0 && k < m.n_kf && i >= 0 && i < min(max(m.kf_n[k], 0), m.stride);
}

// the list of row p: offsets that do not describe a list inside [0, n_obs] give an empty one
__device__ __forceinline__ void row_list(const MapView &m, int p, int &b, int &e)
{
    b = m.obs_off[p], e = m.obs_off[p + 1];
    if (b < 0 || e < b || e > m.n_obs) b = e = 0;
}

// the live entries of row p -- getNumObs() -- counted, or with CLEAR their slots set to -1 (KeyFrame::eraseMapPoint, MapPoint.cpp:222-224)
template <bool CLEAR> __device__ __forceinline__ int live_entries(const MapView &m, int p)
{
    int b, e, n = 0;
    row_list(m, p, b, e);
    for (int j = b; j < e; ++j) {
        int k, i;
        if (!entry_ok(m, j, k, i)) continue;
        int32_t *slot = m.slots + (size_t)k * m.stride + i;
        if (*slot != p || m.bad[k]) continue;
        if (CLEAR) *slot = -1;
        ++n;
    }
    return n;
}

__global__ __launch_bounds__(KF_T) void k_kf_cull_points(MapView m, int32_t *recent, int32_t *n_recent, int cap_recent, int cur_kf_id,
                                                         const int32_t *__restrict__ first_kf, const int32_t *__restrict__ found,
                                                         const int32_t *__restrict__ visible, int32_t *__restrict__ code, int32_t *result)
{
    extern __shared__ uint32_t s_mask[];                           // bit p: an entry of the list names row p
    __shared__ int s_wave[KF_WAVES];
    __shared__ int s_count[8];
    const int tid = threadIdx.x;
    const int n = clamp_to(*n_recent, cap_recent);
    for (int w = tid; w < (m.cap_points + 31) >> 5; w += KF_T) s_mask[w] = 0;
    if (tid < 8) s_count[tid] = 0;
    __syncthreads();
    // ---- the premise: no row twice in the list, over all tiles, before anything is written
    int twice = 0;
    for (int j = tid; j < n; j += KF_T) {
        const int p = recent[j];
        if (p >= 0 && p < m.cap_points) twice |= !bit_set(s_mask, p);
    }
    if (__syncthreads_or(twice)) {
        if (tid < 8) result[tid] = tid == P_REFUSED;
        return;
    }
    int dropped = 0, cleared = 0, was_bad = 0, ratio = 0, few = 0, aged = 0;
    for (int j = tid; j < m.n_obs; j += KF_T) {
        int k, i;
        dropped += !entry_ok(m, j, k, i);
    }
    // ---- LocalMapping.cpp:123-139, a thread per entry: a setBad touches only slots that name its own row
    int kept = 0;                                                  // the same in every thread
    for (int j0 = 0; j0 < n; j0 += KF_T) {
        const int j = j0 + tid;
        int p = -1, c = -2;                                        // -2: no entry
        if (j < n) {
            p = recent[j];
            if (p < 0 || p >= m.cap_points) c = -1, ++dropped;
            else if (!m.valid[p]) c = 1, ++was_bad;                // :126
            else if ((float)found[p] / (float)visible[p] < 0.25f) c = 2, ++ratio;   // :129, MapPoint.cpp:278
            else {
                const uint32_t age = (uint32_t)cur_kf_id - (uint32_t)first_kf[p];
                if (age >= 2 && live_entries<false>(m, p) <= 2) c = 3, ++few;       // :133
                else if (age > 2) c = 4, ++aged;                   // :136
                else c = 0;
            }
            if (c == 2 || c == 3) m.valid[p] = 0, cleared += live_entries<true>(m, p);   // MapPoint::setBad (MapPoint.cpp:210-226)
            code[j] = c;
        }
        int tile;
        const int at = kept + block_scan<KF_WAVES>(c == 0, s_wave, tile);   // its first barrier stands between the tile's reads and its writes
        if (c == 0) recent[at] = p;
        kept += tile;
    }
    block_add(s_count, P_BAD, was_bad), block_add(s_count, P_RATIO, ratio), block_add(s_count, P_FEW, few), block_add(s_count, P_AGED, aged);
    block_add(s_count, P_CLEARED, cleared), block_add(s_count, P_DROPPED, dropped);
    if (tid == 0) s_count[P_KEPT] = kept, *n_recent = kept;
    __syncthreads();
    if (tid < 8) result[tid] = s_count[tid];
}

// the mask's bytes, and the opt-in past 64 KB of LDS with the kernel's static part, as k_cull does it
template <typename Kernel> hipError_t mask_lds(Kernel kernel, int cap_points, size_t *bytes)
{
    *bytes = (size_t)((cap_points + 31) >> 5) * 4;                 // <= 64 KB
    return *bytes + 1024 > 64 * 1024 ? orbx_lds_opt_in((const void *)kernel, *bytes) : hipSuccess;
}

} // namespace

extern "C" int orbm_insert_keyframe_device(orbm_t *h, int K, int cap_kf, double *d_pose_R, double *d_pose_t, uint8_t *d_bad, const void **d_kps,
                                           const uint8_t **d_desc, int32_t *d_n, int32_t *d_slots, int stride, const uint8_t *d_valid,
                                           int cap_points, const int32_t *d_frame_mp, int n2, const double *d_frame_pose_R,
                                           const double *d_frame_pose_t, const void *frame_kps, const uint8_t *frame_desc, int32_t *d_result,
                                           void *stream)
{
    if (cap_kf < 0 || stride < 0 || cap_points < 0 || n2 < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (K < 0 || K >= cap_kf) return orbx_set_error(ORBX_E_ARG, "K must lie in [0, cap_kf)");
    if (!d_pose_R || !d_pose_t || !d_bad || !d_kps || !d_desc || !d_n) return orbx_set_error(ORBX_E_ARG, "null key-frame array");
    if (stride > 0 && !d_slots) return orbx_set_error(ORBX_E_ARG, "null slot array");
    if (cap_points > 0 && !d_valid) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if ((n2 > 0 && !d_frame_mp) || !d_frame_pose_R || !d_frame_pose_t || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (int rc = orbm_check_kf_rows(d_kps, d_desc)) return rc;
    if (int rc = orbm_check_stride(stride)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    size_t lds;
    ORB_TRY(mask_lds(k_kf_insert, cap_points, &lds));
    const KfRow row = {K, (u64 *)d_pose_R, (u64 *)d_pose_t, d_bad, d_kps, d_desc, d_n};
    hipLaunchKernelGGL(k_kf_insert, dim3(1), dim3(KF_T), lds, s, row, d_slots, stride, d_valid, cap_points, d_frame_mp, n2,
                       (const u64 *)d_frame_pose_R, (const u64 *)d_frame_pose_t, frame_kps, frame_desc, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_register_new_points_device(orbm_t *h, const int32_t *d_n_points, int32_t *d_n_registered, int K, int kf_id, int cap_points,
                                               int32_t *d_ref_kf, int32_t *d_first_kf, int32_t *d_found, int32_t *d_visible,
                                               int32_t *d_recent, int cap_recent, int32_t *d_n_recent, int32_t *d_result, void *stream)
{
    if (cap_points < 0 || cap_recent < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (K < 0 || kf_id < 0) return orbx_set_error(ORBX_E_ARG, "K and kf_id must not be negative");
    if (!d_n_points || !d_n_registered || !d_n_recent || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (cap_points > 0 && (!d_ref_kf || !d_first_kf || !d_found || !d_visible)) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if (cap_recent > 0 && !d_recent) return orbx_set_error(ORBX_E_ARG, "null recent list");
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    hipLaunchKernelGGL(k_kf_register, dim3(1), dim3(KF_T), 0, s, d_n_points, d_n_registered, K, kf_id, cap_points, d_ref_kf, d_first_kf, d_found,
                       d_visible, d_recent, cap_recent, d_n_recent, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

extern "C" int orbm_cull_map_points_device(orbm_t *h, int32_t *d_recent, int32_t *d_n_recent, int cap_recent, int cur_kf_id,
                                           const int32_t *d_first_kf, const int32_t *d_found, const int32_t *d_visible, uint8_t *d_valid,
                                           int cap_points, int n_kf, const int32_t *d_n, const uint8_t *d_bad, int32_t *d_slots, int stride,
                                           const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs,
                                           int32_t *d_code, int32_t *d_result, void *stream)
{
    if (cap_recent < 0 || cap_points < 0 || n_kf < 0 || stride < 0 || n_obs < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (cur_kf_id < 0) return orbx_set_error(ORBX_E_ARG, "cur_kf_id must not be negative");
    if (!d_n_recent || !d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (cap_recent > 0 && (!d_recent || !d_code)) return orbx_set_error(ORBX_E_ARG, "null recent list");
    if (cap_points > 0 && (!d_first_kf || !d_found || !d_visible || !d_valid || !d_obs_off)) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if (n_kf > 0 && (!d_n || !d_bad)) return orbx_set_error(ORBX_E_ARG, "null key-frame array");
    if (n_kf > 0 && stride > 0 && !d_slots) return orbx_set_error(ORBX_E_ARG, "null slot array");
    if (n_obs > 0 && (!d_obs_kf || !d_obs_kp)) return orbx_set_error(ORBX_E_ARG, "null observation array");
    if (int rc = orbm_check_stride(stride)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    size_t lds;
    ORB_TRY(mask_lds(k_kf_cull_points, cap_points, &lds));
    const MapView m = {n_kf, stride, cap_points, n_obs, d_n, d_obs_off, d_obs_kf, d_obs_kp, d_bad, d_slots, d_valid};
    hipLaunchKernelGGL(k_kf_cull_points, dim3(1), dim3(KF_T), lds, s, m, d_recent, d_n_recent, cap_recent, cur_kf_id, d_first_kf, d_found,
                       d_visible, d_code, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
