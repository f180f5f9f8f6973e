// Wave primitives (64 lanes) of the small kernels.  Internal.  The extractor's and the best2 / top-k / resolve kernels keep their own.
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
} // namespace
