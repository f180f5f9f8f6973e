// Wave (64 lanes) and workgroup primitives of the small kernels.  Internal.  The extractor's and the best2 / top-k / resolve kernels
// keep their own.
#pragma once
#include <hip/hip_runtime.h>

namespace {
// every lane gets the sum / the least / the greatest of the wave's values: the __shfl_xor butterfly, widest step first
#define ORB_WAVE_REDUCE(name, expr)                                         \
    template <typename T> __device__ __forceinline__ T name(T v)            \
    {                                                                       \
        _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) v = (expr);      \
        return v;                                                           \
    }
ORB_WAVE_REDUCE(wave_sum, v + __shfl_xor(v, o))
ORB_WAVE_REDUCE(wave_min, min(v, __shfl_xor(v, o)))
ORB_WAVE_REDUCE(wave_max, max(v, __shfl_xor(v, o)))
#undef ORB_WAVE_REDUCE

// inclusive scan over the wave; a block scan adds one LDS slot per wave, and where its barriers sit is the caller's
__device__ __forceinline__ int wave_scan(int v)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o);
        if ((threadIdx.x & 63) >= o) v += t;
    }
    return v;
}

// exclusive scan of v over a workgroup of WAVES waves in thread order and the total; s_wave is WAVES ints; two barriers, the first
// between whatever the caller read before the scan and whatever it writes behind it
template <int WAVES> __device__ __forceinline__ int block_scan(int v, int *s_wave, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = wave_scan(v);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = inc - v;
    total = 0;
#pragma unroll 1
    for (int w = 0; w < WAVES; ++w) {
        const int x = s_wave[w];
        if (w < wave) before += x;
        total += x;
    }
    __syncthreads();                                               // read by everyone before the next scan overwrites the slots
    return before;
}

// block_scan of the pair (a, b) with one pair of barriers: both exclusive scans and both totals; s_wave is 2 x WAVES ints
template <int WAVES> __device__ __forceinline__ void block_scan2(int a, int b, int (*s_wave)[WAVES], int &ea, int &eb, int &ta, int &tb)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ia = wave_scan(a), ib = wave_scan(b);
    if (lane == 63) s_wave[0][wave] = ia, s_wave[1][wave] = ib;
    __syncthreads();
    ea = ia - a, eb = ib - b, ta = 0, tb = 0;
#pragma unroll 1
    for (int w = 0; w < WAVES; ++w) {
        const int xa = s_wave[0][w], xb = s_wave[1][w];
        if (w < wave) ea += xa, eb += xb;
        ta += xa, tb += xb;
    }
    __syncthreads();                                               // read by everyone before the next scan overwrites the totals
}

// the sums of N per-thread counts over the workgroup into s_count[slot[n]] (LDS, or a result array in device memory): block_add(s_count,
// {SLOT_A, SLOT_B}, {a, b}).  The wave reductions come first, so that their shuffles overlap; the caller's barrier follows
template <int N> __device__ __forceinline__ void block_add(int *s_count, const int (&slot)[N], const int (&v)[N])
{
    int sum[N];
#pragma unroll
    for (int n = 0; n < N; ++n) sum[n] = wave_sum(v[n]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n)
            if (sum[n]) atomicAdd(&s_count[slot[n]], sum[n]);
    }
}
__device__ __forceinline__ void block_add(int *s_count, int slot, int v)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_count[slot], v);
}

// The eight counters of a d_result.  A kernel counts in LDS and ends on flush_counts behind a barrier: one workgroup writes them, several
// add to what k_counters_clear zeroed ahead of them on the stream (LAUNCH_COUNTED of orb_host.h launches the pair).  A template only so
// that a file which never launches it gets no copy of it: a plain __global__ is emitted wherever it is seen
template <int = 0> __global__ void k_counters_clear(int32_t *__restrict__ result)
{
    if (threadIdx.x < 8) result[threadIdx.x] = 0;
}
__device__ __forceinline__ void flush_counts(const int *s_cnt, int32_t *result)
{
    if (threadIdx.x < 8) {
        const int v = s_cnt[threadIdx.x];
        if (gridDim.x == 1) result[threadIdx.x] = v;
        else if (v) atomicAdd(&result[threadIdx.x], v);
    }
}

// N per-thread floating-point sums over a workgroup of WAVES waves in a fixed order, so that the same input gives the same bytes and no
// floating-point atomic is needed.  block_sums_put: the butterfly over the wave, then lane 0 leaves sum k of [first, last) (uniform) in
// s_part[wave][k] (wave: the slot, by default the thread's own wave -- a thread that stands in for several gives the wave it stands in
// for); the caller's barrier follows; block_sums_get: sum k of the workgroup, the wave slots added in ascending order
template <int WAVES, int N>
__device__ __forceinline__ void block_sums_put(const double (&acc)[N], double (&s_part)[WAVES][N], int first = 0, int last = N, int wave = -1)
{
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (k < first || k >= last) continue;
        const double v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) s_part[wave < 0 ? (int)(threadIdx.x >> 6) : wave][k] = v;
    }
}
template <int WAVES, int N> __device__ __forceinline__ double block_sums_get(const double (&s_part)[WAVES][N], int k)
{
    double s = 0.0;
    for (int w = 0; w < WAVES; ++w) s = s + s_part[w][k];
    return s;
}

// Lanes of ONE wave write LDS that other lanes of the same wave read in the next step.  The LDS pipe serves a wave's accesses in
// issue order, so the hardware needs nothing; this keeps the COMPILER from moving a later lane's read above an earlier lane's write
// (a fence at wavefront scope and a wave barrier emit no instruction).
__device__ __forceinline__ void wave_order()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// values other threads of the workgroup (or lanes of the wave) write in the same phase, other elements or the same value: relaxed
// atomics at WORKGROUP scope, which is all a one-workgroup kernel needs: global_load / global_store with sc0 on gfx950 (at system
// scope, the default of __atomic_load_n(p, __ATOMIC_RELAXED), they carry sc0 sc1 and go past every cache)
__device__ __forceinline__ int ld(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st(int32_t *p, int x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

// a mask of one bit per row in LDS: bits_zero by a whole workgroup of THREADS threads (the caller's barrier follows); bit_set sets
// bit p and is true for the one thread that found it clear; bit_test reads it while others may set other bits
template <int THREADS> __device__ __forceinline__ void bits_zero(uint32_t *s_mask, int n_bits)
{
    for (int w = threadIdx.x; w < (n_bits + 31) >> 5; w += THREADS) s_mask[w] = 0;
}
__device__ __forceinline__ bool bit_set(uint32_t *s_mask, int p)
{
    const uint32_t bit = 1u << (p & 31);
    return !(atomicOr(&s_mask[p >> 5], bit) & bit);
}
__device__ __forceinline__ bool bit_test(const uint32_t *s_mask, int p)
{
    return __hip_atomic_load(&s_mask[p >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> (p & 31) & 1;
}
} // namespace
