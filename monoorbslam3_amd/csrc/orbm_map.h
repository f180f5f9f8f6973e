// The device-resident map as the map-side kernels see it, written once: the key frames' slot arrays, the map-point table's d_valid and
// the observation CSR (include/orbm.h, "Observations built and key frames culled on the device"), the covisibility graph, and the host
// helper that checks an entry point's map arguments and fills the view.  Internal.
//
// THE SLOT ARRAYS ARE THE TRUTH, the CSR only tells where the slots naming a row are, and it is distrusted: an index out of range is
// dropped and counted, never dereferenced (map_list, map_usable); an entry counts as an observation only while its slot names the row
// NOW and its key frame is not bad (map_live).  The kernels are ONE workgroup of 1024 threads each where the work is a few thousand
// slots and short lists -- latency, not throughput -- with a mask of one bit per table row in dynamic LDS where a row has to be
// handled once (orb_device.h: bits_zero / bit_set / bit_test).
#pragma once
#include <type_traits>

#include "orb_device.h"
#include "orbm_internal.h"

namespace {

constexpr int MAP_KEY_SHIFT = 13;          // a first-occurrence or sort key = (position of the key frame) << 13 | slot
constexpr int MAP_NONE = 0x7fffffff;       // above every key: not named
constexpr int MAP_MAX_RECENT = 32;
static_assert(ORBM_MEDIAN_MAX_STRIDE == 1 << MAP_KEY_SHIFT, "the key packs the slot index into 13 bits");

template <bool WRITE, typename T> using map_ptr = std::conditional_t<WRITE, T, const T> *;

// WRITE: the kernel may store to the slots and to d_valid.  d_bad is read as it is NOW, never through the key-frame table's pointer.
template <bool WRITE> struct MapViewOf {
    int n_kf, stride, cap_points, n_obs;
    const int32_t *kf_n;
    const uint8_t *bad;
    map_ptr<WRITE, int32_t> slots;
    map_ptr<WRITE, uint8_t> valid;
    const int32_t *obs_off, *obs_kf, *obs_kp;
};
using MapView = MapViewOf<true>;
using MapReadView = MapViewOf<false>;

template <bool WRITE> struct GraphViewOf {
    int cap, n_kf;
    map_ptr<WRITE, int32_t> weight, ord_kf, ord_n, parent;
};
using GraphView = GraphViewOf<true>;
using GraphReadView = GraphViewOf<false>;

struct RecentList {
    int32_t kf[MAP_MAX_RECENT];
};

// the slots of key frame k that exist in d_slots
template <bool W> __device__ __forceinline__ int map_slots(const MapViewOf<W> &m, int k) { return min(max(m.kf_n[k], 0), m.stride); }
template <bool W> __device__ __forceinline__ map_ptr<W, int32_t> map_slot(const MapViewOf<W> &m, int k, int i) { return m.slots + (size_t)k * m.stride + i; }

// row p's CSR list; offsets that do not describe a list inside [0, n_obs] give an empty one
template <bool W> __device__ __forceinline__ void map_list(const MapViewOf<W> &m, int p, int &b, int &e)
{
    b = m.obs_off[p], e = m.obs_off[p + 1];
    if (b < 0 || e < b || e > m.n_obs) b = e = 0;
}

// both indices usable?  (the slot index also has to exist in d_slots.)  The two sign tests as one, (k | i) >= 0, so that both indices
// are loaded side by side and a list walk pays one memory wait per entry, not two
template <bool W> __device__ __forceinline__ bool map_usable(const MapViewOf<W> &m, int k, int i)
{
    return (k | i) >= 0 && k < m.n_kf && i < map_slots(m, k);
}

// CSR entry j -> (k, i); usable?
template <bool W> __device__ __forceinline__ bool map_entry(const MapViewOf<W> &m, int j, int &k, int &i)
{
    k = m.obs_kf[j], i = m.obs_kp[j];
    return map_usable(m, k, i);
}

// a usable (k, i) as an observation of row p: its slot names the row NOW and its key frame is not bad.  RELAXED: the slot is read
// with ld, for a kernel whose other threads store to slots in the same phase (local BA's apply); a plain load otherwise
template <bool RELAXED = false, bool W> __device__ __forceinline__ bool map_live(const MapViewOf<W> &m, int k, int i, int p)
{
    return (RELAXED ? ld(map_slot(m, k, i)) : *map_slot(m, k, i)) == p && m.bad[k] == 0;
}

// CSR entry j as an observation of row p NOW -> (k, i): usable and live
template <bool RELAXED = false, bool W> __device__ __forceinline__ bool map_live_entry(const MapViewOf<W> &m, int j, int p, int &k, int &i)
{
    return map_entry(m, j, k, i) && map_live<RELAXED>(m, k, i, p);
}

// the second-entry test of the two bundle adjustments' assemblies: does a live entry of row p's list before j, in [b, j), name key
// frame k as well?  Found by re-reading the list's start: n^2 / 2 reads for a list of n, nothing for the 2-30 of a map
template <bool RELAXED = false, bool W> __device__ __forceinline__ bool map_second_entry(const MapViewOf<W> &m, int b, int j, int p, int k)
{
    bool again = false;
    int k2, i2;
    for (int j2 = b; j2 < j && !again; ++j2) again = map_live_entry<RELAXED>(m, j2, p, k2, i2) && k2 == k;
    return again;
}

// The slot walk of the two bundle adjustments' assemblies over the key frames s_kf[0 .. n_list) (LDS), slot t = (position, slot) =
// (t / stride, t % stride) of n_list * stride.  map_mark_first: every valid row named by one of those slots gets in work_row[] the least
// (position << 13 | slot) naming it (atomicMin: whatever the order); work_row holds MAP_NONE behind a barrier, the caller's barrier
// follows.  map_first_at: the row slot t names if t is that row's first occurrence, else -1 -- the caller takes the slots in order,
// a tile of THREADS at a time, and numbers what it keeps of them by a block scan
template <int THREADS, bool W> __device__ __forceinline__ void map_mark_first(const int *s_kf, int n_list, const MapViewOf<W> &m, int32_t *work_row)
{
    const int total = n_list * m.stride;                           // <= 1024 * 8192
    for (int t = threadIdx.x; t < total; t += THREADS) {
        const int l = t / m.stride, i = t - l * m.stride, k = s_kf[l];
        if (i >= map_slots(m, k)) continue;
        const int p = m.slots[(size_t)k * m.stride + i];
        if (p >= 0 && p < m.cap_points && m.valid[p]) atomicMin(&work_row[p], l << MAP_KEY_SHIFT | i);
    }
}
template <bool W> __device__ __forceinline__ int map_first_at(const int *s_kf, int total, const MapViewOf<W> &m, const int32_t *work_row, int t)
{
    if (t >= total) return -1;
    const int l = t / m.stride, i = t - l * m.stride, k = s_kf[l];
    if (i >= map_slots(m, k)) return -1;
    const int p = m.slots[(size_t)k * m.stride + i];
    return p >= 0 && p < m.cap_points && m.valid[p] && work_row[p] == (l << MAP_KEY_SHIFT | i) ? p : -1;
}

// An EdgeMono's / EdgeSE3ProjectXYZ's measurement and information from the orbx_kp record of feature i of key frame k (Optimize.cpp:871-877,
// :1228-1234): kp.pt widened, invSigma2 = (double)((1.f / size) / size) -- the reference's float expression, written once
__device__ __forceinline__ void map_edge_measurement(const void *const *kps, int k, int i, double *z, double *inv_sigma2)
{
    const orbx_kp *kp = (const orbx_kp *)kps[k] + i;
    z[0] = (double)kp->x, z[1] = (double)kp->y;
    const float size = kp->size;
    *inv_sigma2 = (double)((1.f / size) / size);
}

// a list length read from device memory, kept inside the row
template <bool W> __device__ __forceinline__ int graph_list_length(const GraphViewOf<W> &g, int k) { return min(max(g.ord_n[k], 0), g.n_kf); }

// The rows named by the slots of the key frames s_kf[0 .. n_list) (LDS), each valid row once, in the order of its first occurrence
// by (position in the list, slot) -> rows[0 .. min(n_rows, cap_rows)); returns n_rows.  A row's first occurrence is the least key
// naming it (atomicMin: whatever the atomics' order), then the slots in order, a tile of THREADS at a time, numbered by a block scan.
// Every thread of the one workgroup calls; work[cap_points] holds MAP_NONE behind a barrier and ends holding the rows' keys; s_wave is
// block_scan's; invalid and duplicates gain this thread's count of slots naming a row that is not valid / a row named before.
template <int THREADS, bool W>
__device__ __forceinline__ int map_first_rows(const int32_t *s_kf, int n_list, const MapViewOf<W> &m, int32_t *work, int32_t *rows, int cap_rows,
                                              int *s_wave, int &invalid, int &duplicates)
{
    const int tid = threadIdx.x;
    for (int t = 0; t < n_list; ++t) {
        const int k = s_kf[t], nk = map_slots(m, k);
        for (int i = tid; i < nk; i += THREADS) {
            const int p = *map_slot(m, k, i);
            if (p < 0 || p >= m.cap_points) continue;
            if (!m.valid[p]) ++invalid;
            else atomicMin(&work[p], t << MAP_KEY_SHIFT | i);
        }
    }
    __syncthreads();
    int n_rows = 0;
    for (int t = 0; t < n_list; ++t) {
        const int k = s_kf[t], nk = map_slots(m, k);
        for (int i0 = 0; i0 < nk; i0 += THREADS) {
            const int i = i0 + tid;
            int p = -1;
            bool first = false;
            if (i < nk) {
                p = *map_slot(m, k, i);
                if (p >= 0 && p < m.cap_points && m.valid[p]) {
                    first = ld(&work[p]) == (t << MAP_KEY_SHIFT | i);
                    duplicates += !first;
                }
            }
            int tile;
            const int at = n_rows + block_scan<THREADS / 64>(first, s_wave, tile);
            if (first && at < cap_rows) rows[at] = p;
            n_rows += tile;
        }
    }
    return n_rows;
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------
// An entry point's map arguments, every ORBX_E_ARG case of them in one order: without the CSR, with it, and with it into the view.
// The limits (orbm_check_stride, orbm_check_points) stay with the caller, behind ITS other arguments' checks: an argument error wins
// over a limit.
inline int orbm_check_slots(int n_kf, const int32_t *d_n, const uint8_t *d_bad, const int32_t *d_slots, int stride, const uint8_t *d_valid, int cap_points)
{
    if (n_kf < 0 || stride < 0 || cap_points < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (n_kf > 0 && (!d_n || !d_bad)) return orbx_set_error(ORBX_E_ARG, "null key-frame array");
    if (n_kf > 0 && stride > 0 && !d_slots) return orbx_set_error(ORBX_E_ARG, "null slot array");
    if (cap_points > 0 && !d_valid) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    return ORBX_OK;
}
inline int orbm_check_map(int n_kf, const int32_t *d_n, const uint8_t *d_bad, const int32_t *d_slots, int stride, const uint8_t *d_valid, int cap_points,
                          const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs)
{
    if (n_obs < 0) return orbx_set_error(ORBX_E_ARG, "negative count");
    if (int rc = orbm_check_slots(n_kf, d_n, d_bad, d_slots, stride, d_valid, cap_points)) return rc;
    if (cap_points > 0 && !d_obs_off) return orbx_set_error(ORBX_E_ARG, "null map-point table array");
    if (n_obs > 0 && (!d_obs_kf || !d_obs_kp)) return orbx_set_error(ORBX_E_ARG, "null observation array");
    return ORBX_OK;
}
template <bool W>
int orbm_map_view(MapViewOf<W> *m, int n_kf, const int32_t *d_n, const uint8_t *d_bad, map_ptr<W, int32_t> d_slots, int stride,
                  map_ptr<W, uint8_t> d_valid, int cap_points, const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs)
{
    if (int rc = orbm_check_map(n_kf, d_n, d_bad, d_slots, stride, d_valid, cap_points, d_obs_off, d_obs_kf, d_obs_kp, n_obs)) return rc;
    *m = {n_kf, stride, cap_points, n_obs, d_n, d_bad, d_slots, d_valid, d_obs_off, d_obs_kf, d_obs_kp};
    return ORBX_OK;
}

// the graph's arguments: ORBX_E_ARG and the view here, the limit behind the other arguments' checks
template <bool W> int orbm_graph_view(GraphViewOf<W> *g, const orbm_covis_graph *graph, int n_kf)
{
    if (!graph) return orbx_set_error(ORBX_E_ARG, "null graph");
    if (!graph->d_weight || !graph->d_ord_kf || !graph->d_ord_n || !graph->d_parent) return orbx_set_error(ORBX_E_ARG, "null graph array");
    if (graph->cap_kf < 0 || n_kf < 0 || n_kf > graph->cap_kf) return orbx_set_error(ORBX_E_ARG, "n_kf must lie in [0, cap_kf]");
    *g = {graph->cap_kf, n_kf, graph->d_weight, graph->d_ord_kf, graph->d_ord_n, graph->d_parent};
    return ORBX_OK;
}
inline int orbm_graph_check_limit(const orbm_covis_graph *graph)
{
    return graph->cap_kf > ORBM_GRAPH_MAX_KF ? orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBM_GRAPH_MAX_KF (4096) key frames in the graph") : ORBX_OK;
}

} // namespace
