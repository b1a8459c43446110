// Lane-level helpers the baseline kernel units share (stid.hip, stnorm.hip, gru.hip, stae_rows.h): each is one fixed instruction
// sequence, so units that use it round alike.
#pragma once
#include "common.h"

namespace regt {

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
// row of accumulator register i within the 32 x 32 result (the column is lane & 31)
__device__ __forceinline__ int crow(int i, int lh) { return (i & 3) + 8 * (i >> 2) + 4 * lh; }

__device__ __forceinline__ float wave_sum(float v) {          // every lane gets the same sum, in one fixed order
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ float sigm(float v) { return 1.f / (1.f + expf(-v)); }

}  // namespace regt
