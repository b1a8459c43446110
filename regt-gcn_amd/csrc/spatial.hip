// First layer of the reference's SpatialGCN (models/SpatialGCN.py:12-16, 38-41) with the period sum of layer 2 folded in:
//
//   pre_t = x_t W0^T + (L~ x_t) W1^T + b            (ChebConv K = 2, 64 output channels)
//   S     = sum_t keep_t * 2 * relu(pre_t)          (F.dropout p = 0.5 in training mode; keep = NULL: eval, S = sum_t relu(pre_t))
//
// gcn2 is linear and the periods are summed after it, so layer 2 runs once on S; this is the only work
// of the model that scales with N*T.  x_packed (N, T, F) and lx_packed = L~ x (same layout) are data: no dx.
//
// Mapping: one wave owns a tile of 16 nodes and loops over the periods in order t = 0..T-1, so S sums in a fixed order with
// no atomics.  Per period the product [x_t | L~ x_t] (16 x 2F) . [W0 | W1]^T runs on v_mfma_f32_16x16x4_f32 as four 16-channel
// tiles; a k-step of the MFMA takes feature 16j + 4q + e of part p (q = lane >> 4) from both operands, so every lane loads its
// node's row as float4s and the weights sit in registers for the whole kernel.
//   forward:  A = weights (row = channel), B = rows (column = node): lane holds channels 4q..4q+3 of node (lane & 15) -> float4
//             stores of S.
//   backward: A = rows, B = weights (same registers, roles swapped): lane holds channel (lane & 15) of nodes 4q..4q+3, which is
//             directly the A operand of dW = dG^T [x | L~ x] (the MFMA sums over q, i.e. over 4 nodes per step).  Partial dW / db
//             per wave go to a slab, reduced in a fixed order by the two stages of slab_reduce.h (no float atomics: bit-reproducible).
// Keep mask: uint32 (N*T, 2), row node*T + t, bit j of word w keeps channel 32w + j.
#include "slab_reduce.h"

namespace regt {

namespace {

constexpr int SP_C = 64;              // out_channels of the first ChebConv (models/SpatialGCN.py:14)
constexpr int SP_WAVES = 4;           // waves per workgroup
constexpr int SP_TARGET_WAVES = 2048; // backward: partial-sum slots (2 per SIMD)
constexpr int SP_CHUNK = 32;          // backward: partials summed per thread in the first reduction stage

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// w[p][j][e][tile] = W_p[tile*16 + (lane & 15)][16j + 4q + e] (0 beyond F)
template <int NJ>
__device__ __forceinline__ void load_weights(const float* __restrict__ w0, const float* __restrict__ w1, int F, float (&w)[2][NJ][4][4]) {
    const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int tile = 0; tile < 4; ++tile) {
                    const int k = 16 * j + 4 * q + e;
                    w[p][j][e][tile] = k < F ? (p ? w1 : w0)[(tile * 16 + c) * F + k] : 0.f;
                }
}

// v[p][j] = part p of row `row` at features 16j + 4q .. +3 (0 beyond F or for a dead row)
template <int NJ>
__device__ __forceinline__ void load_rows(const float* __restrict__ x, const float* __restrict__ lx, long row, bool live, int F,
                                          f32x4 (&v)[2][NJ]) {
    const int q = (threadIdx.x & 63) >> 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 16 * j + 4 * q;
        const bool ok = live && k < F;
        v[0][j] = ok ? *reinterpret_cast<const f32x4*>(x + row * F + k) : zero;
        v[1][j] = ok ? *reinterpret_cast<const f32x4*>(lx + row * F + k) : zero;
    }
}

template <int NJ>
__global__ __launch_bounds__(256) void spatial_fwd_kernel(const float* __restrict__ x, const float* __restrict__ lx,
                                                          const float* __restrict__ w0, const float* __restrict__ w1,
                                                          const float* __restrict__ b, const uint2* __restrict__ keep, int N, int T,
                                                          int F, float* __restrict__ S) {
    const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
    const long node0 = ((long)blockIdx.x * SP_WAVES + (threadIdx.x >> 6)) * 16;
    if (node0 >= N) return;
    float w[2][NJ][4][4];
    load_weights<NJ>(w0, w1, F, w);
    f32x4 bias[4], s[4];
#pragma unroll
    for (int tile = 0; tile < 4; ++tile) {
        bias[tile] = *reinterpret_cast<const f32x4*>(b + tile * 16 + 4 * q);
        s[tile] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const long node = node0 + c;
    const bool live = node < N;
    const long row0 = node * T;
    f32x4 cur[2][NJ];
    load_rows<NJ>(x, lx, row0, live, F, cur);
    for (int t = 0; t < T; ++t) {
        f32x4 nxt[2][NJ];
        load_rows<NJ>(x, lx, row0 + t + 1, live && t + 1 < T, F, nxt);
        uint2 m = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        if (keep && live) m = keep[row0 + t];
        f32x4 acc[4] = {bias[0], bias[1], bias[2], bias[3]};
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int tile = 0; tile < 4; ++tile) acc[tile] = mfma4(w[p][j][e][tile], cur[p][j][e], acc[tile]);
        const float scale = keep ? 2.f : 1.f;
#pragma unroll
        for (int tile = 0; tile < 4; ++tile) {
            const unsigned word = (tile >> 1) ? m.y : m.x;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int bit = (tile & 1) * 16 + 4 * q + r;
                const float g = fmaxf(acc[tile][r], 0.f);
                s[tile][r] += ((word >> bit) & 1u) ? g * scale : 0.f;
            }
        }
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < NJ; ++j) cur[p][j] = nxt[p][j];
    }
    if (live) {
#pragma unroll
        for (int tile = 0; tile < 4; ++tile) *reinterpret_cast<f32x4*>(S + node * SP_C + tile * 16 + 4 * q) = s[tile];
    }
}

// slab row of one wave: [dW0 (64, F) | dW1 (64, F) | db (64)]
__host__ __device__ inline long slab_stride(int F) { return 2L * SP_C * F + SP_C; }

template <int NJ>
__global__ __launch_bounds__(256) void spatial_bwd_kernel(const float* __restrict__ x, const float* __restrict__ lx,
                                                          const float* __restrict__ w0, const float* __restrict__ w1,
                                                          const float* __restrict__ b, const uint2* __restrict__ keep,
                                                          const float* __restrict__ dS, int N, int T, int F, int tiles_per_wave,
                                                          int nwaves, float* __restrict__ slab) {
    const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
    const int wave = blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
    if (wave >= nwaves) return;
    float w[2][NJ][4][4];
    load_weights<NJ>(w0, w1, F, w);
    float bias[4];
#pragma unroll
    for (int tile = 0; tile < 4; ++tile) bias[tile] = b[tile * 16 + c];
    f32x4 gw[2][NJ][4];          // dW_p[tile*16 + 4q + r][16 kb + c]
    float gb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int kb = 0; kb < NJ; ++kb)
#pragma unroll
            for (int tile = 0; tile < 4; ++tile) gw[p][kb][tile] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float scale = keep ? 2.f : 1.f;
    const long ntiles = ((long)N + 15) / 16;
    const long tile_end = min((long)(wave + 1) * tiles_per_wave, ntiles);
    for (long nt = (long)wave * tiles_per_wave; nt < tile_end; ++nt) {
        const long node0 = nt * 16;
        const long nodeA = node0 + c;              // row of the A operand (pre-activation recompute)
        const bool liveA = nodeA < N;
        long nodeD[4];                             // nodes of the accumulator rows: 4q + r
        bool liveD[4];
        float ds[4][4];                            // dS[nodeD[r]][tile*16 + c]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            nodeD[r] = node0 + 4 * q + r;
            liveD[r] = nodeD[r] < N;
#pragma unroll
            for (int tile = 0; tile < 4; ++tile) ds[tile][r] = liveD[r] ? dS[nodeD[r] * SP_C + tile * 16 + c] : 0.f;
        }
        for (int t = 0; t < T; ++t) {
            f32x4 a[2][NJ];
            load_rows<NJ>(x, lx, nodeA * T + t, liveA, F, a);
            float xb[2][NJ][4];                    // B operand of dW: part p of row nodeD[r] at feature 16 kb + c
            uint2 m[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = nodeD[r] * T + t;
#pragma unroll
                for (int kb = 0; kb < NJ; ++kb) {
                    const int k = 16 * kb + c;
                    const bool ok = liveD[r] && k < F;
                    xb[0][kb][r] = ok ? x[row * F + k] : 0.f;
                    xb[1][kb][r] = ok ? lx[row * F + k] : 0.f;
                }
                m[r] = (keep && liveD[r]) ? keep[row] : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
            }
            f32x4 acc[4];
#pragma unroll
            for (int tile = 0; tile < 4; ++tile) acc[tile] = f32x4{bias[tile], bias[tile], bias[tile], bias[tile]};
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int tile = 0; tile < 4; ++tile) acc[tile] = mfma4(a[p][j][e], w[p][j][e][tile], acc[tile]);
            float dg[4][4];
#pragma unroll
            for (int tile = 0; tile < 4; ++tile) {
                const int bit = (tile & 1) * 16 + c;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned word = (tile >> 1) ? m[r].y : m[r].x;
                    dg[tile][r] = (acc[tile][r] > 0.f && ((word >> bit) & 1u)) ? ds[tile][r] * scale : 0.f;
                    gb[tile] += dg[tile][r];
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int kb = 0; kb < NJ; ++kb)
#pragma unroll
                        for (int tile = 0; tile < 4; ++tile) gw[p][kb][tile] = mfma4(dg[tile][r], xb[p][kb][r], gw[p][kb][tile]);
        }
    }
#pragma unroll
    for (int tile = 0; tile < 4; ++tile) {        // db: lanes c, c+16, c+32, c+48 hold the four node quarters of channel tile*16 + c
        gb[tile] += __shfl_xor(gb[tile], 16);
        gb[tile] += __shfl_xor(gb[tile], 32);
    }
    float* out = slab + (long)wave * slab_stride(F);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int kb = 0; kb < NJ; ++kb) {
            const int k = 16 * kb + c;
            if (k < F) {
#pragma unroll
                for (int tile = 0; tile < 4; ++tile)
#pragma unroll
                    for (int r = 0; r < 4; ++r) out[(long)p * SP_C * F + (tile * 16 + 4 * q + r) * F + k] = gw[p][kb][tile][r];
            }
        }
    if (q == 0) {
#pragma unroll
        for (int tile = 0; tile < 4; ++tile) out[2L * SP_C * F + tile * 16 + c] = gb[tile];
    }
}

struct BwdPlan { int tiles_per_wave, nwaves, nchunks; };

BwdPlan bwd_plan(int N) {
    const long ntiles = ((long)N + 15) / 16;
    const int tpw = (int)((ntiles + SP_TARGET_WAVES - 1) / SP_TARGET_WAVES);
    const int nwaves = (int)((ntiles + tpw - 1) / tpw);
    return {tpw, nwaves, (nwaves + SP_CHUNK - 1) / SP_CHUNK};
}

template <int NJ>
int fwd_nj(const float* x, const float* lx, const float* w0, const float* w1, const float* b, const uint32_t* keep, int N, int T, int F,
           float* S, hipStream_t st) {
    const int ntiles = (N + 15) / 16;
    hipLaunchKernelGGL(spatial_fwd_kernel<NJ>, dim3(cdiv(ntiles, SP_WAVES)), dim3(256), 0, st, x, lx, w0, w1, b,
                       reinterpret_cast<const uint2*>(keep), N, T, F, S);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

template <int NJ>
int bwd_nj(const float* x, const float* lx, const float* w0, const float* w1, const float* b, const uint32_t* keep, const float* dS,
           int N, int T, int F, const BwdPlan& pl, float* slab, hipStream_t st) {
    hipLaunchKernelGGL(spatial_bwd_kernel<NJ>, dim3(cdiv(pl.nwaves, SP_WAVES)), dim3(256), 0, st, x, lx, w0, w1, b,
                       reinterpret_cast<const uint2*>(keep), dS, N, T, F, pl.tiles_per_wave, pl.nwaves, slab);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace

size_t spatial_slab_floats(int N, int T, int F) {
    if (N < 1 || T < 1 || F < 4 || F > 64 || F % 4) return 0;
    const BwdPlan pl = bwd_plan(N);
    return (size_t)(pl.nwaves + pl.nchunks) * (size_t)slab_stride(F);
}

int launch_spatial_fwd(const float* x, const float* lx, const float* w0, const float* w1, const float* b, const uint32_t* keep, int N,
                       int T, int F, float* S, hipStream_t st) {
    switch ((F + 15) / 16) {
        case 1: return fwd_nj<1>(x, lx, w0, w1, b, keep, N, T, F, S, st);
        case 2: return fwd_nj<2>(x, lx, w0, w1, b, keep, N, T, F, S, st);
        case 3: return fwd_nj<3>(x, lx, w0, w1, b, keep, N, T, F, S, st);
        default: return fwd_nj<4>(x, lx, w0, w1, b, keep, N, T, F, S, st);
    }
}

int launch_spatial_bwd(const float* x, const float* lx, const float* w0, const float* w1, const float* b, const uint32_t* keep,
                       const float* dS, int N, int T, int F, float* dw0, float* dw1, float* db, float* slab, hipStream_t st) {
    const BwdPlan pl = bwd_plan(N);
    int rc;
    switch ((F + 15) / 16) {
        case 1: rc = bwd_nj<1>(x, lx, w0, w1, b, keep, dS, N, T, F, pl, slab, st); break;
        case 2: rc = bwd_nj<2>(x, lx, w0, w1, b, keep, dS, N, T, F, pl, slab, st); break;
        case 3: rc = bwd_nj<3>(x, lx, w0, w1, b, keep, dS, N, T, F, pl, slab, st); break;
        default: rc = bwd_nj<4>(x, lx, w0, w1, b, keep, dS, N, T, F, pl, slab, st); break;
    }
    if (rc != REGT_OK) return rc;
    const long stride = slab_stride(F);
    SlabSegs sg{};
    add_seg(sg, dw0, (long)SP_C * F);
    add_seg(sg, dw1, (long)SP_C * F);
    add_seg(sg, db, SP_C);
    return launch_slab_reduce_chunked<SP_CHUNK>(slab, pl.nwaves, stride, slab + (long)pl.nwaves * stride, sg, st);
}

}  // namespace regt
