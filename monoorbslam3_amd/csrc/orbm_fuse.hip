// What the fuse does with its hits, on the device-resident slot arrays (include/orbm.h, "The fuse's hits applied on the device"):
//   orbm_fuse_apply_device   the tail of the static SearchByProjection(keyFrame, mapPoints, Map*, th) (ORBMatcher.cpp:574-589) with
//                            MapPoint::addObservation / KeyFrame::addMapPoint and MapPoint::replace (MapPoint.cpp:233-264)
//
// THE SLOT ARRAYS ARE THE TRUTH: an observation is a slot, so an add is one store and a replace rewrites the slots that name the loser.
// ONE launch of ONE workgroup of 1024 threads (the shape of orbm_map.h: a few thousand hits are latency), in phases between barriers:
//   1  the mask (one bit per table row, dynamic LDS) = the rows named by a slot of K; head[] (one int per slot of K) = empty
//   2  every entry classified on the arrays as passed -- none / dropped / gated / live -- into d_work: the hit slot of a live entry,
//      a negative class otherwise; head[s] = the first live entry of slot s (atomicMin: the value does not depend on the order)
//   3  the mask cleared; then the two premises: a live row sets its bit (set already: a row twice, refusal 1), the valid occupant of a
//      hit slot sets its bit (set already: an occupant in two hit slots, refusal 2) -- the two kinds of rows are disjoint, a live row is
//      not named by K --; then every slot of K without a hit reads its occupant's bit (set: an occupant in two slots, refusal 2)
//   4  refused: d_result and nothing else.  Else the codes of the entries that are not live, the slots with more than one live entry
//      marked, the CSR's unusable entries counted
//   5  a wave per CHAIN (the live entries of one hit slot, in list order), lanes across the observation lists.  The rows of a chain --
//      the slot's first occupant and the entries' rows -- belong to no other chain (the premises), so nothing a chain reads that decides
//      anything is written by another wave.  The winner's observations are the CSR entries of ALL the chain's rows so far whose slot
//      names the winner NOW, plus the chain's own slot of K, which is kept in registers and left out of every list walk.  A step walks
//      those lists twice: count (getNumObs of both rows), then per tile of 64 entries decide -- the loser's entry moves unless the
//      winner holds a slot of that key frame (any tile of the chain's lists, re-read: the tiles before this one are written) or an
//      earlier lane of this tile moves one there -- and store.  A chain of more than one entry finds its next entry by scanning d_work
//      forward and links the entries through d_work, so that the later steps can walk the earlier rows.
// Every count is a sum and every stored value is decided by the chain alone: the bytes do not depend on the order of anything.
// No scratch memory, no handle scratch, no allocation, no host wait.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <string>

#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orbm_internal.h"
#include "orbm_map.h"

namespace {

typedef unsigned long long u64;

constexpr int FU_T = 1024;              // the one workgroup
constexpr int FU_WAVES = FU_T / 64;
constexpr int FU_EMPTY = MAP_NONE;      // head[s]: no live entry hits slot s
constexpr int FU_MAX_NQ = 1 << 30;      // a link in d_work is -8 - (the next entry)
constexpr int FU_LINK = -8;

// d_code, and d_work's classes (-1 - code) of the entries that are not live
enum { F_NONE = 0, F_DROPPED = 1, F_GATED = 2, F_ADDED = 3, F_BAD_OCCUPANT = 4, F_LIST_REPLACED = 5, F_OCCUPANT_REPLACED = 6, F_UNDONE = 7 };
enum { R_MATCHES = 0, R_REFUSED = 1, R_ADDED = 2, R_LIST_REPLACED = 3, R_OCCUPANT_REPLACED = 4, R_CLEARED = 5, R_GATED = 6, R_DROPPED = 7 };

// the map (orbm_map.h), the chains' key frame and the entries
struct FuseView : MapView {
    int K;
    const int32_t *rows;
    int32_t *work;
};

__device__ __forceinline__ int fuse_row(const FuseView &v, int j) { return v.rows ? v.rows[j] : j; }

// row p's CSR list, the same for every lane of the wave
__device__ __forceinline__ void fuse_list(const FuseView &v, int p, int &b, int &e)
{
    map_list(v, p, b, e);
    b = uniform(b), e = uniform(e);
}

// CSR entry j as an observation: usable, its key frame not bad, not the chain's own slot (K, own) -> what its slot holds NOW
__device__ __forceinline__ bool fuse_entry(const FuseView &v, int j, int own, int &k, int &held)
{
    int i;
    if (!map_entry(v, j, k, i) || v.bad[k] || (k == v.K && i == own)) return false;
    held = ld(map_slot(v, k, i));
    return true;
}

// the rows of a chain up to its entry `last`: the slot's first occupant (o0, -1 = none), then the entries' rows in list order
constexpr int CH_START = -2, CH_HEAD = -3;
struct ChainRows {
    int o0, head, last, at;
};
__device__ __forceinline__ bool chain_next(const FuseView &v, ChainRows &c, int &r)
{
    if (c.at == CH_START) {
        c.at = CH_HEAD;
        if (c.o0 >= 0) {
            r = c.o0;
            return true;
        }
    }
    if (c.at == c.last) return false;
    const int next = c.at == CH_HEAD ? c.head : FU_LINK - uniform(ld(&v.work[c.at]));
    if (next <= c.at || next > c.last) return false;              // a link is an entry further on, never past the current one
    c.at = next;
    r = uniform(fuse_row(v, c.at));
    return true;
}

__global__ __launch_bounds__(FU_T) void k_fuse_apply(const FuseView v, const int32_t *__restrict__ best_idx, int nq, int32_t *found, const int32_t *visible,
                                                     int32_t *code, int32_t *refresh_sel, int32_t *result)
{
    extern __shared__ uint32_t s_dyn[];                            // the mask, (cap_points + 31) / 32 words, then head[stride]
    __shared__ uint32_t s_multi[ORBM_MEDIAN_MAX_STRIDE / 32];      // bit s: more than one live entry hits slot s
    __shared__ int s_count[8];
    __shared__ int s_refused[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    const int K = v.K, stride = v.stride, cap_points = v.cap_points, n_obs = v.n_obs;
    uint8_t *const valid = v.valid;
    int32_t *const work = v.work;
    uint32_t *s_mask = s_dyn;
    int *s_head = (int *)(s_dyn + ((cap_points + 31) >> 5));
    const int nK = map_slots(v, K);
    const bool bad_K = v.bad[K] != 0;
    int32_t *mine = map_slot(v, K, 0);
    // ---- 1: the rows named by a slot of K
    bits_zero<FU_T>(s_mask, cap_points);
    for (int i = tid; i < stride; i += FU_T) s_head[i] = FU_EMPTY;
    bits_zero<FU_T>(s_multi, ORBM_MEDIAN_MAX_STRIDE);
    if (tid < 8) s_count[tid] = 0;
    if (tid < 2) s_refused[tid] = 0;
    __syncthreads();
    for (int i = tid; i < nK; i += FU_T) {
        const int o = mine[i];
        if (o >= 0 && o < cap_points) bit_set(s_mask, o);
    }
    __syncthreads();
    // ---- 2: every entry on the arrays as passed (ORBMatcher.cpp:534, :574)
    int dropped = 0, gated = 0;
    for (int j = tid; j < nq; j += FU_T) {
        const int s = best_idx[j], p = fuse_row(v, j);
        int w;
        if (s < 0) w = -1 - F_NONE;
        else if (s >= nK || p < 0 || p >= cap_points) w = -1 - F_DROPPED, ++dropped;
        else if (!valid[p] || bit_test(s_mask, p)) w = -1 - F_GATED, ++gated;
        else w = s, atomicMin(&s_head[s], j);
        work[j] = w;
    }
    __syncthreads();
    // ---- 3: the premises, before anything is written
    bits_zero<FU_T>(s_mask, cap_points);
    __syncthreads();
    for (int j = tid; j < nq; j += FU_T) {
        if (work[j] < 0) continue;
        if (!bit_set(s_mask, fuse_row(v, j))) s_refused[0] = 1;              // a row in two live entries
    }
    for (int i = tid; i < nK; i += FU_T) {
        if (s_head[i] == FU_EMPTY) continue;
        const int o = mine[i];
        if (o < 0 || o >= cap_points || !valid[o]) continue;
        if (!bit_set(s_mask, o)) s_refused[1] = 1;                           // the occupant of two hit slots
    }
    __syncthreads();
    for (int i = tid; i < nK; i += FU_T) {
        if (s_head[i] != FU_EMPTY) continue;
        const int o = mine[i];
        if (o < 0 || o >= cap_points || !valid[o]) continue;
        if (bit_test(s_mask, o)) s_refused[1] = 1;                           // the occupant of a hit slot in a second slot of K
    }
    __syncthreads();
    const int refused = s_refused[0] ? 1 : s_refused[1] ? 2 : 0;
    if (refused) {
        if (tid < 8) result[tid] = tid == R_REFUSED ? refused : 0;
        return;
    }
    // ---- 4: the entries that are not live; the slots with a chain of more than one entry; the CSR's unusable entries
    for (int j = tid; j < nq; j += FU_T) {
        const int w = work[j];
        if (w < 0) code[j] = -1 - w, refresh_sel[j] = -1;
        else if (s_head[w] != j) bit_set(s_multi, w);
    }
    for (int j = tid; j < n_obs; j += FU_T) dropped += !map_usable(v, v.obs_kf[j], v.obs_kp[j]);
    __syncthreads();
    // ---- 5: a wave per chain
    int added = 0, bad_occupant = 0, list_replaced = 0, occupant_replaced = 0, undone = 0;   // the same in every lane of the wave
    int cleared = 0;                                                                         // per lane
    for (int s = wave; s < nK; s += FU_WAVES) {
        const int head = s_head[s];
        if (head == FU_EMPTY) continue;
        const bool multi = bit_test(s_multi, s);
        int cur = uniform(mine[s]);                                // what slot s holds, kept in registers from here on
        const bool cur_row = cur >= 0 && cur < cap_points;
        bool cur_valid = cur_row && valid[cur] != 0;
        const int o0 = cur_valid ? cur : -1;
        for (int j = head;;) {
            const int p = uniform(fuse_row(v, j));
            int c, sel = -1;
            if (!(cur >= 0 && cur < cap_points)) {                 // :576-578
                if (lane == 0) st(&mine[s], p);
                cur = p, cur_valid = true, c = F_ADDED, sel = p, ++added;
            } else if (!cur_valid) {                               // :579 is false; the match still counts (:587)
                c = F_BAD_OCCUPANT, ++bad_occupant;
            } else {
                int b, e;
                fuse_list(v, p, b, e);
                bool is_long = e - b > ORBM_MAX_LIST;
                fuse_list(v, cur, b, e);
                is_long |= e - b > ORBM_MAX_LIST;
                if (is_long) {
                    c = F_UNDONE, ++undone;
                } else {
                    // getNumObs() of both rows (:580)
                    int n_p = 0, n_cur = 0, r;
                    for (ChainRows a = {o0, head, j, CH_START}; chain_next(v, a, r);) {
                        fuse_list(v, r, b, e);
                        if (e - b > ORBM_MAX_LIST) continue;       // never merged: no slot of it moved
                        for (int t = b + lane; t < e; t += 64) {
                            int k, held;
                            if (!fuse_entry(v, t, s, k, held)) continue;
                            n_p += held == p, n_cur += held == cur;
                        }
                    }
                    n_p = wave_sum(n_p), n_cur = wave_sum(n_cur) + !bad_K;
                    const bool list_loses = n_cur > n_p;           // strictly: a tie replaces the occupant
                    const int L = list_loses ? p : cur, W = list_loses ? cur : p;
                    const bool own_w = list_loses && !bad_K;       // W observes K through the chain's own slot
                    // MapPoint::replace (MapPoint.cpp:249-257): the loser's observations in order
                    for (ChainRows a = {o0, head, j, CH_START}; chain_next(v, a, r);) {
                        fuse_list(v, r, b, e);
                        if (e - b > ORBM_MAX_LIST) continue;
                        for (int t0 = b; t0 < e; t0 += 64) {
                            const int t = t0 + lane;
                            int k = -1, held = -1;
                            const bool cand = t < e && fuse_entry(v, t, s, k, held) && held == L;
                            const u64 cm = __ballot(cand);
                            if (!cm) continue;
                            bool seen = cand && k == K && own_w;
                            for (u64 m = cm; m; m &= m - 1) {      // an earlier entry of this tile moves into the same key frame
                                const int l = __builtin_ctzll(m);
                                seen |= l < lane && __builtin_amdgcn_readlane(k, l) == k;
                            }
                            int r2, b2, e2;
                            for (ChainRows a2 = {o0, head, j, CH_START}; chain_next(v, a2, r2);) {   // what W holds now
                                fuse_list(v, r2, b2, e2);
                                if (e2 - b2 > ORBM_MAX_LIST) continue;
                                for (int u0 = b2; u0 < e2; u0 += 64) {
                                    const int u = u0 + lane;
                                    int k2 = -1, held2 = -1;
                                    const bool has = u < e2 && fuse_entry(v, u, s, k2, held2) && held2 == W;
                                    for (u64 m = __ballot(has); m; m &= m - 1) seen |= __builtin_amdgcn_readlane(k2, __builtin_ctzll(m)) == k;
                                }
                            }
                            if (cand) {
                                st(map_slot(v, k, v.obs_kp[t]), seen ? -1 : W);
                                cleared += seen;
                            }
                            __threadfence_block();                 // the wave's own stores, before its lanes read the slots again
                        }
                    }
                    if (!list_loses) {                             // the chain's own slot is an observation of the occupant
                        if (bad_K) cur_valid = false;              // ... unless K is bad: the slot keeps naming the loser
                        else {
                            if (lane == 0) st(&mine[s], p);
                            cur = p;
                        }
                    }
                    if (lane == 0) {
                        valid[L] = 0;
                        if (found) found[W] = (int32_t)((uint32_t)found[W] + (uint32_t)found[L] + (uint32_t)visible[L]);   // MapPoint.cpp:259-260
                    }
                    sel = W;
                    if (list_loses) c = F_LIST_REPLACED, ++list_replaced;
                    else c = F_OCCUPANT_REPLACED, ++occupant_replaced;
                }
            }
            if (lane == 0) code[j] = c, refresh_sel[j] = sel;
            if (!multi) break;
            int next = -1;                                         // the chain's next entry: the first behind j that hit slot s
            for (int t0 = j + 1; t0 < nq && next < 0; t0 += 64) {
                const int t = t0 + lane;
                const u64 m = __ballot(t < nq && ld(&work[t]) == s);
                if (m) next = t0 + __builtin_ctzll(m);
            }
            if (next < 0) break;
            if (lane == 0) st(&work[j], FU_LINK - next);
            __threadfence_block();
            j = next;
        }
    }
    block_add(s_count, {R_DROPPED, R_GATED, R_CLEARED}, {dropped, gated, cleared});
    if (lane == 0) {                                               // the chains' counts are the same in every lane of the wave
        if (undone) atomicAdd(&s_count[R_DROPPED], undone);
        if (added) atomicAdd(&s_count[R_ADDED], added);
        if (list_replaced) atomicAdd(&s_count[R_LIST_REPLACED], list_replaced);
        if (occupant_replaced) atomicAdd(&s_count[R_OCCUPANT_REPLACED], occupant_replaced);
        const int matches = added + bad_occupant + list_replaced + occupant_replaced + undone;
        if (matches) atomicAdd(&s_count[R_MATCHES], matches);
    }
    __syncthreads();
    if (tid < 8) result[tid] = s_count[tid];
}

} // namespace

extern "C" int orbm_fuse_apply_device(orbm_t *h, const int32_t *d_best_idx, const int32_t *d_rows, int nq, int n_kf, int kf_target,
                                      const int32_t *d_n, const uint8_t *d_bad, int32_t *d_slots, int stride, uint8_t *d_valid, int cap_points,
                                      const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs, int32_t *d_found,
                                      const int32_t *d_visible, int32_t *d_work, int32_t *d_code, int32_t *d_refresh_sel, int32_t *d_result,
                                      void *stream)
{
    if (!d_result) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (nq < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (!d_n || !d_bad) return orbx_set_error(ORBX_E_ARG, "null key-frame array");   // wanted even when n_kf == 0
    MapView m;
    if (int rc = orbm_map_view(&m, n_kf, d_n, d_bad, d_slots, stride, d_valid, cap_points, d_obs_off, d_obs_kf, d_obs_kp, n_obs)) return rc;
    if (kf_target < 0 || kf_target >= n_kf) return orbx_set_error(ORBX_E_ARG, "kf_target is not a key frame of the table");
    if ((d_found == nullptr) != (d_visible == nullptr)) return orbx_set_error(ORBX_E_ARG, "d_found and d_visible go together");
    if (nq > 0 && (!d_best_idx || !d_work || !d_code || !d_refresh_sel)) return orbx_set_error(ORBX_E_ARG, "null entry array");
    if (nq > FU_MAX_NQ) return orbx_set_error(ORBX_E_UNSUPPORTED, "more than 2^30 entries in one call");
    if (int rc = orbm_check_stride(stride)) return rc;
    if (int rc = orbm_check_points(cap_points)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    const size_t lds_bytes = ((size_t)((cap_points + 31) >> 5) + (size_t)stride) * 4;   // <= 64 KB + 32 KB
    if (lds_bytes + 2048 > 64 * 1024) ORB_TRY(orbx_lds_opt_in((const void *)k_fuse_apply, lds_bytes));   // with the static 1064 B: past 64 KB
    hipLaunchKernelGGL(k_fuse_apply, dim3(1), dim3(FU_T), lds_bytes, s, FuseView{m, kf_target, d_rows, d_work}, d_best_idx, nq,
                       d_found, d_visible, d_code, d_refresh_sel, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}
