// What the STAEformer forward kernels (staeformer.hip) and their backward kernels (staeformer_bwd.hip) share: the operand layout
// helpers of v_mfma_f32_32x32x2_f32 and the row statistics of add+LayerNorm.  The backward recomputes a row's mean and rstd with
// the very code the forward ran, so it gets the forward's bits.
#pragma once
#include "kernels.h"

namespace regt {
namespace stae {

constexpr int THREADS = 256;
constexpr int QT = 32;                    // queries per wave, keys per tile

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
// row of accumulator register i within the 32 x 32 result (the column is lane & 31)
__device__ __forceinline__ int crow(int i, int lh) { return (i & 3) + 8 * (i >> 2) + 4 * lh; }

// 16 consecutive floats at p (16-byte aligned) or zeros
__device__ __forceinline__ void load16(float (&r)[16], const float* p, bool live) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 v = live ? reinterpret_cast<const float4*>(p)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        r[4 * j] = v.x, r[4 * j + 1] = v.y, r[4 * j + 2] = v.z, r[4 * j + 3] = v.w;
    }
}

__device__ __forceinline__ float wave_sum(float v) {          // every lane gets the same sum, in one fixed order
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// One row of add+LayerNorm, a wave per row, element d = lane + 64 j in v[j]: leaves z - mean(z) in v (0 past D), z = r + yr, and
// returns 1 / sqrt(var + eps) (mean first, then the centred squares; biased variance).
__device__ __forceinline__ float ln_centre_row(const float* r, const float* yr, int lane, int D, float eps, float (&v)[4]) {
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = lane + 64 * j;
        v[j] = d < D ? r[d] + yr[d] : 0.f;
        sum += v[j];
    }
    const float mean = wave_sum(sum) / (float)D;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float c = lane + 64 * j < D ? v[j] - mean : 0.f;
        v[j] = c;
        sq += c * c;
    }
    return 1.0f / sqrtf(wave_sum(sq) / (float)D + eps);
}

}  // namespace stae
}  // namespace regt
