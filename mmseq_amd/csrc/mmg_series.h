// mmg_series.h -- the primitives every per-series post-processing kernel shares: the order-preserving key of a double, the wave sum in
// a fixed lane order, the workgroup's bitonic sort of 64-bit keys, and the round-up to a power of two.  Device inline functions only
// (no kernels), so any translation unit may include it.  Every feature built on these promises bit-identical reruns: the order of
// the operations below is the contract.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mmg_math.h"

namespace mmg {

// the smallest power of two >= v (1 for v <= 1)
template <typename T>
MMG_HD T next_pow2(T v)
{
    T p = 1;
    while (p < v) p <<= 1;
    return p;
}

// order-preserving map of doubles onto unsigned integers, and back: unsigned order of the keys is numeric order of the doubles
// (-0.0 below +0.0; the NaNs with the sign bit clear sort last, below the padding key ~0)
__device__ __forceinline__ uint64_t order_key(double x)
{
    const uint64_t b = bits_of(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double order_unkey(uint64_t k)
{
    return double_of((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}

// x[i] + x[i + 32], then 16, 8, 4, 2, 1: lane 0 ends with the sum of the wave's 64 values in the halving order (the lanes above the
// live half read themselves or dead lanes: their values are never used)
__device__ __forceinline__ double lane_fold(double x)
{
    x = x + __shfl_down(x, 32, 64);
    x = x + __shfl_down(x, 16, 64);
    x = x + __shfl_down(x, 8, 64);
    x = x + __shfl_down(x, 4, 64);
    x = x + __shfl_down(x, 2, 64);
    x = x + __shfl_down(x, 1, 64);
    return x;
}
// lane_fold, and the sum of lane 0 to every lane
__device__ __forceinline__ double lane_sum(double x)
{
    return __shfl(lane_fold(x), 0, 64);
}

// bitonic sort of PP (a power of two) keys by the whole workgroup of BLOCK threads, ascending; the keys are visible to the workgroup
// on entry (the caller synchronises after writing them); ends synchronised
template <uint32_t BLOCK>
__device__ __forceinline__ void block_sort(uint64_t *k, uint32_t PP)
{
    for (uint32_t w = 2; w <= PP; w <<= 1)
        for (uint32_t j = w >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < PP; i += BLOCK) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint64_t a = k[i], b = k[l];
                    if ((a > b) == ((i & w) == 0)) { k[i] = b; k[l] = a; }
                }
            }
            __syncthreads();
        }
}

} // namespace mmg
