// finenv_group.h -- what the row movers share (finenv_replay.hip, finenv_rollout.hip): the 16-byte
// unit, the lane group of a sample and Philox4x32-10.  Device code only; every function is inlined.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

// This thread's lane in its group of G and the sample b of that group: 256 / G samples per block
template <int G>
__device__ __forceinline__ long long group_sample(int &lane)
{
    lane = (int)threadIdx.x & (G - 1);
    return (long long)blockIdx.x * (256 / G) + ((int)threadIdx.x / G);
}

// Philox4x32-10 (Salmon et al., SC'11; Random123): counter c[4], key k[2] -> first two output words
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t &x0, uint32_t &x1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x0 = c0;
    x1 = c1;
}

}  // namespace
