// Whole-model input gradient in front of the transposed aggregation (regt_input_gradient): three (M, F) products from the
// pre-activation gradients regt_backward leaves in the workspace, in ONE pass over the rows,
//   dAX = dzr [Gz; Gr] + dhp Gh      dXd = ds A0      dLX = ds A_region(row)                              (regional / uncollapsed TemporalGCN)
//   dAX = dzr [Gz; Gr] + dhp Gh      dXd = dzr P0zr + dh W0      dLX = dzr P1zr + dh W1                    (collapsed TemporalGCN)
// a segmented skinny GEMM: segment s streams A_s (M, K_s) once and multiplies each K chunk with up to three (K_s, F) weights, one per
// output -- 4 M C floats in, 3 M F floats out, HBM-bound.
//
// Tile: cell_dx_kernel's (cell_dx.hip) -- four waves own 128 rows, a wave 32 of them at the full padded width with one (F <= 32) or two
// 32 x 32 fp32 MFMA accumulators PER OUTPUT; K in chunks of 32 through LDS; rows on a 36-float stride (16-byte LDS reads of a wave start at
// sixteen distinct multiples of 4 banks; the 4-byte weight reads are served per lane half, 32 consecutive floats each: no conflict).  One
// thing differs: the next chunk's rows and weights are loaded into registers BEFORE the current chunk is multiplied, so the global loads
// are in flight across the MFMA chain and both barriers of the chunk.
// Per-row region weights (dLX of the regional model): a tile whose rows all belong to one region -- every tile but the few on a region
// boundary when the ids ascend with the node number -- takes A_region as the third weight of the ds segment.  Any other tile multiplies ds
// with A0 alone there and then runs ONE MORE SEGMENT PER REGION PRESENT in the tile, ascending: ds again (from L2), rows of other regions
// zeroed while they are staged, against that region's block.  Unsorted ids are therefore correct, only slower.
// Order: every output element is one accumulator that receives its products in the fixed order of the segments and of k inside them (a
// zeroed row adds +0); no atomics: bit-reproducible.
#include <limits.h>

#include "lane_helpers.h"
#include "kernels.h"

namespace regt {

constexpr int MDX_TM = 128, MDX_KC = 32, MDX_LDA = MDX_KC + 4;

template <int NT>
__global__ __launch_bounds__(256) void model_dx_kernel(const ModelDxArgs a) {
    constexpr int LDB = NT * 32;
    __shared__ __attribute__((aligned(16))) float As[MDX_TM * MDX_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[3][MDX_KC * LDB];
    __shared__ int row_reg[MDX_TM];          // region of each row of the tile
    __shared__ int reg_list[MDX_TM];         // impure tile: the regions present, ascending
    __shared__ int reg_count;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lh = lane >> 5, lc = lane & 31;
    const long row0 = (long)blockIdx.x * MDX_TM;
    const int F = a.F;

    // ---- the tile's regions ---------------------------------------------------------------------------------------------------------
    int reg0 = 0, nextra = 0;
    bool pure = true;
    if (a.node_region) {
        const int rmax = a.R - 1;
        reg0 = min(max(a.node_region[row0 / a.T], 0), rmax);
        int mine = reg0;
        if (tid < MDX_TM) {
            if (row0 + tid < a.M) mine = min(max(a.node_region[(row0 + tid) / a.T], 0), rmax);
            row_reg[tid] = mine;
        }
        pure = __syncthreads_and(mine == reg0) != 0;
        if (!pure) {
            if (tid == 0) {
                int cnt = 0, last = -1;
                for (;;) {
                    int mn = INT_MAX;
                    for (int i = 0; i < MDX_TM; ++i) {
                        const int v = row_reg[i];
                        if (v > last && v < mn) mn = v;
                    }
                    if (mn == INT_MAX) break;
                    reg_list[cnt++] = mn;
                    last = mn;
                }
                reg_count = cnt;
            }
            __syncthreads();
            nextra = reg_count;
        }
    }
    const int nsegs = 3 + nextra;

    f32x16 acc[3][NT];
#pragma unroll
    for (int o = 0; o < 3; ++o)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[o][n][i] = 0.f;

    // ---- staging: rows ar + 32 pass, floats ak .. ak + 3 of the chunk; weights: element e = tid + 256 i of (32 x LDB / 4) float4 --------------
    const int ar = tid >> 3, ak = (tid & 7) * 4;
    float4 ra[MDX_TM / 32], rb[3][NT];
    int has_next = 0;                        // bit o: the staged chunk multiplies into output o
    auto load = [&](int s, int k0) {
        const float* A = s == 0 ? a.A[0] : s == 1 ? a.A[1] : a.A[2];
        const int K = s == 0 ? a.K[0] : s == 1 ? a.K[1] : a.K[2];
        const float* B[3];
        int mask = -1;
        if (s < 3) {
#pragma unroll
            for (int o = 0; o < 3; ++o) B[o] = s == 0 ? a.B[0][o] : s == 1 ? a.B[1][o] : a.B[2][o];
            if (s == 2 && a.node_region) B[2] = pure ? a.Breg + (long)reg0 * a.breg_stride : nullptr;
        } else {
            mask = reg_list[s - 3];
            B[0] = B[1] = nullptr;
            B[2] = a.Breg + (long)mask * a.breg_stride;
        }
#pragma unroll
        for (int pass = 0; pass < MDX_TM / 32; ++pass) {
            const int r = ar + 32 * pass;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row0 + r < a.M && k0 + ak < K && (mask < 0 || row_reg[r] == mask)) v = *reinterpret_cast<const float4*>(A + (row0 + r) * K + k0 + ak);
            ra[pass] = v;
        }
        has_next = 0;
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            if (!B[o]) continue;             // (uniform over the workgroup)
            has_next |= 1 << o;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int e = tid + 256 * i, k = e / (LDB / 4), c = (e % (LDB / 4)) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k0 + k < K && c < F) v = *reinterpret_cast<const float4*>(B[o] + (long)(k0 + k) * F + c);
                rb[o][i] = v;
            }
        }
    };
    auto seg_k = [&](int s) { return s == 0 ? a.K[0] : s == 1 ? a.K[1] : a.K[2]; };

    int s = 0, k0 = 0;
    load(s, k0);
    for (;;) {
        __syncthreads();                     // the previous chunk has been consumed
        const int has = has_next;
#pragma unroll
        for (int pass = 0; pass < MDX_TM / 32; ++pass) *reinterpret_cast<float4*>(&As[(ar + 32 * pass) * MDX_LDA + ak]) = ra[pass];
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            if (!(has & (1 << o))) continue;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int e = tid + 256 * i, k = e / (LDB / 4), c = (e % (LDB / 4)) * 4;
                *reinterpret_cast<float4*>(&Bs[o][k * LDB + c]) = rb[o][i];
            }
        }
        __syncthreads();
        k0 += MDX_KC;
        if (k0 >= seg_k(s)) { ++s; k0 = 0; }
        const bool more = s < nsegs;
        if (more) load(s, k0);               // in flight while this chunk is multiplied
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            if (!(has & (1 << o))) continue;
#pragma unroll
            for (int j = 0; j < MDX_KC / 8; ++j) {
                const float4 av4 = *reinterpret_cast<const float4*>(&As[(wave * 32 + lc) * MDX_LDA + 8 * j + 4 * lh]);
                const float av[4] = {av4.x, av4.y, av4.z, av4.w};
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int n = 0; n < NT; ++n) acc[o][n] = mfma32(av[u], Bs[o][(8 * j + 4 * lh + u) * LDB + n * 32 + lc], acc[o][n]);
            }
        }
        if (!more) break;
    }
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        float* out = o == 0 ? a.out[0] : o == 1 ? a.out[1] : a.out[2];
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int col = n * 32 + lc;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long row = row0 + wave * 32 + crow(i, lh);
                if (row < a.M && col < F) out[row * F + col] = acc[o][n][i];
            }
        }
    }
}

// every K a multiple of 4, F a multiple of 4 and <= 64, every pointer 16-byte aligned, every output fed by at least one segment, region ids
// (node_region != NULL) select blocks Breg + id * breg_stride.  The shapes and pointers the caller has checked (api_model.hip); the region ids
// are device data nobody has read: an id outside [0, R) is clamped into it, so a corrupt table gives a wrong gradient, never a read outside Breg
int launch_model_dx(const ModelDxArgs& a, hipStream_t st) {
    REGT_CHECK_ARG(a.M > 0 && a.F > 0 && a.F % 4 == 0 && a.F <= 64 && a.T > 0 && a.R > 0, "model_dx: M=%ld F=%d T=%d R=%d (F a multiple of 4, <= 64)", a.M,
                   a.F, a.T, a.R);
    for (int s = 0; s < 3; ++s)
        REGT_CHECK_ARG(a.A[s] && a.K[s] > 0 && a.K[s] % 4 == 0, "model_dx: segment %d needs rows and K=%d a positive multiple of 4", s, a.K[s]);
    REGT_CHECK_ARG(!a.node_region || (a.Breg && a.breg_stride % 4 == 0), "model_dx: per-row regions need the region blocks");
    REGT_CHECK_ARG(a.out[0] && a.out[1] && a.out[2], "model_dx: an output is NULL");
    const dim3 grid((unsigned)cdiv(a.M, MDX_TM));
    if (a.F <= 32) hipLaunchKernelGGL(model_dx_kernel<1>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(model_dx_kernel<2>, grid, dim3(256), 0, st, a);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace regt
