// What the STAEformer forward kernels (staeformer.hip), their backward kernels (staeformer_bwd.hip) and the whole-model training
// kernels (staeformer_train.hip) share: the operand layout helpers of v_mfma_f32_32x32x2_f32, the table index of the embedding, and
// add+LayerNorm with and without keep-bit dropout on the branch -- its row statistics and its forward and backward kernels, stated
// once as templates.  The backward recomputes a row's mean and rstd with the very code the forward ran, so it gets the forward's bits.
#pragma once
#include "kernels.h"
#include "lane_helpers.h"

namespace regt {
namespace stae {

constexpr int THREADS = 256;
constexpr int QT = 32;                    // queries per wave, keys per tile

// 16 consecutive floats at p (16-byte aligned) or zeros
__device__ __forceinline__ void load16(float (&r)[16], const float* p, bool live) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 v = live ? reinterpret_cast<const float4*>(p)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        r[4 * j] = v.x, r[4 * j + 1] = v.y, r[4 * j + 2] = v.z, r[4 * j + 3] = v.w;
    }
}

// (long)v clamped into [0, size): truncation toward zero; negative and NaN give 0.  The embedding forward reads the table row this
// names and its backward sends the row's gradient there.
__device__ __forceinline__ int table_index(float v, int size) {
    if (!(v >= 1.0f)) return 0;
    return v >= (float)size ? size - 1 : (int)v;
}

// One row of add+LayerNorm, a wave per row, element d = lane + 64 j in v[j]: leaves z - mean(z) in v (0 past D) and returns
// 1 / sqrt(var + eps) (mean first, then the centred squares; biased variance).  z = r + yr, or, with DROP, z = r + keep yr s: kw is
// the row's D / 32 keep words, bit j of word w keeps column 32 w + j; bit j of km says whether v[j]'s column was kept.
template <bool DROP>
__device__ __forceinline__ float ln_centre_row_keep(const float* r, const float* yr, const uint32_t* kw, float s, int lane, int D, float eps,
                                                    float (&v)[4], unsigned& km) {
    float sum = 0.f;
    km = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = lane + 64 * j;
        if constexpr (DROP) {
            v[j] = 0.f;
            if (d < D) {
                const unsigned bit = (kw[d >> 5] >> (d & 31)) & 1u;
                km |= bit << j;
                v[j] = r[d] + (bit ? yr[d] * s : 0.f);
            }
        } else {
            v[j] = d < D ? r[d] + yr[d] : 0.f;
        }
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

__device__ __forceinline__ float ln_centre_row(const float* r, const float* yr, int lane, int D, float eps, float (&v)[4]) {
    unsigned km;
    return ln_centre_row_keep<false>(r, yr, nullptr, 1.0f, lane, D, eps, v, km);
}

// out = LayerNorm(z) gamma + beta, one wave per row, z as in ln_centre_row_keep (keep: (M, D / 32) words, read with DROP only).
// residual and out may be the same array: a lane reads its own elements before it writes them.
template <bool DROP>
__global__ __launch_bounds__(THREADS) void stae_add_layernorm_kernel(const float* residual, const float* __restrict__ y,
                                                                     const uint32_t* __restrict__ keep, float s,
                                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                     float eps, long M, int D, float* out) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (row >= M) return;
    float v[4];
    unsigned km;
    const float rstd = ln_centre_row_keep<DROP>(residual + row * D, y + row * D, DROP ? keep + row * (D / 32) : nullptr, s, lane, D, eps, v, km);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = lane + 64 * j;
        if (d < D) out[row * D + d] = v[j] * rstd * gamma[d] + beta[d];
    }
}

constexpr int LN_ROWS = 16;               // rows per wave of the add+LayerNorm backward

// Add+LayerNorm backward, a wave per LN_ROWS consecutive rows: dz = rstd (g - mean(g) - x^ mean(g x^)) with g = dout gamma, and, with
// DROP, dy = keep dz s in the same pass (dz is the gradient of residual, dy that of y; without DROP dz is both and dy is not touched).
// partial (nwaves, 2, D): wave w's sums of dout x^ and of dout over its rows.
template <bool DROP>
__global__ __launch_bounds__(THREADS) void stae_add_layernorm_bwd_kernel(const float* __restrict__ residual, const float* __restrict__ y,
                                                                         const uint32_t* __restrict__ keep, float s,
                                                                         const float* __restrict__ gamma, const float* __restrict__ dout,
                                                                         float eps, long M, int D, float* __restrict__ dz,
                                                                         float* __restrict__ dyo, float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const long w = (long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    const long r0 = w * LN_ROWS;
    if (r0 >= M) return;
    float gm[4], dg[4], db[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = lane + 64 * j;
        gm[j] = d < D ? gamma[d] : 0.f;
        dg[j] = 0.f, db[j] = 0.f;
    }
    const long r1 = r0 + LN_ROWS < M ? r0 + LN_ROWS : M;
    for (long row = r0; row < r1; ++row) {
        float v[4], g[4];
        unsigned km;
        const float rstd = ln_centre_row_keep<DROP>(residual + row * D, y + row * D, DROP ? keep + row * (D / 32) : nullptr, s, lane, D, eps, v, km);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = lane + 64 * j;
            const float dy = d < D ? dout[row * D + d] : 0.f;
            v[j] *= rstd;                                    // x^
            g[j] = dy * gm[j];
            s1 += g[j];
            s2 = fmaf(g[j], v[j], s2);
            dg[j] = fmaf(dy, v[j], dg[j]);
            db[j] += dy;
        }
        const float m1 = wave_sum(s1) / (float)D, m2 = wave_sum(s2) / (float)D;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = lane + 64 * j;
            if (d < D) {
                const float z = rstd * (g[j] - m1 - v[j] * m2);
                dz[row * D + d] = z;
                if constexpr (DROP) dyo[row * D + d] = (km >> j) & 1u ? z * s : 0.f;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = lane + 64 * j;
        if (d < D) partial[w * 2 * D + d] = dg[j], partial[w * 2 * D + D + d] = db[j];
    }
}

}  // namespace stae
}  // namespace regt
