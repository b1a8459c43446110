// The flat segmented GEMM C = sum_seg A_seg B_seg^T with a fused epilogue functor: the kernel templates over the cores of
// gemm_core.h / gemm_fast.h / gemm_split.h / gemm_small.h, and the host ladder that picks one of them.  A unit that includes this
// header instantiates the kernels of its own epilogues only (gemm_fwd.hip, gemm_cell.hip).
//
//   gemm_flat_split_kernel<Epi, REGION, NP>  the three-workgroup core SplitCore (gemm_split.h): NP = 0 fp32 planes on
//                                      v_mfma_f32_32x32x2_f32 (the default), 3 = exact 3-way bf16 split, 1 = bf16 operands
//                                      (v_mfma_f32_32x32x16_bf16); gemm_flat_split8_kernel: NP = 1 with bf16-stored activations
//   gemm_flat_fast_kernel<Epi, Core>   the two-workgroup fp32 core FastCore (gemm_fast.h): weights stored [K][N],
//                                      REGT_FP32_CORE=wide
//   gemm_flat_small_kernel<Epi, ..>    the same with 64 x 64 tiles for problems of fewer than 128 big tiles (gemm_small.h)
//   gemm_flat_kernel<Epi>              generic fallback (operands that are not 16-byte tileable)
#pragma once
#include <type_traits>

#include "gemm_epilogue.h"

namespace regt {

// ---- host rules (gemm_dispatch.hip) --------------------------------------------------------------------------------------
// fewer 128 x 128 tiles than this: the chip is mostly idle and one tile's latency is the kernel's duration
constexpr long SMALL_TILE_LIMIT = 128;
// the grid of bm x bn tiles over M x N: one workgroup per tile, so the count must stay below 2^31
int gemm_tiles(long M, int N, int bm, int bn, long* tiles);
// may the K loop keep its slab descriptors in scalar registers?  0: LDS table; 1: scalar descriptors; 2: scalar descriptors and
// every segment's weights in fragment order (SEG_B_FRAG)
int uniform_ok(const GemmSegs& S, long M);
// -1: the vector cores cannot take the segments, else bit0 = BT, bit1 = has a region-masked segment, bit2 = relu on A
int fast_class(const GemmSegs& S, int N, bool vec);
// a run-time flag as a compile-time one: fn(std::true_type{}) or fn(std::false_type{})
template <class Fn>
static int with_flag(bool flag, Fn&& fn) { return flag ? fn(std::true_type{}) : fn(std::false_type{}); }

// Developer build (-DREGT_WG_TRACE, tools/wg_trace.py): the flat GEMM kernels of gemm_fwd.hip with N == REGT_WG_TRACE_N record,
// per workgroup, the 100 MHz wall clock at the start of the K loop, at its end and after the epilogue, plus HW_ID / XCC_ID
// (which CU it ran on) -- the data behind DESIGN.md's "who overlaps with whom on a CU" analysis.
#if defined(REGT_WG_TRACE) && defined(REGT_WG_TRACE_UNIT)
#define WG_TRACE_T(name) const long name = wall_clock64()
#define WG_TRACE_END(N, ta, tb)                                                                                              \
    if (threadIdx.x == 0 && WG_TILE_ID < WG_TRACE_MAX && (N) == REGT_WG_TRACE_N) {                                            \
        long* q_ = g_wg_trace + 4L * WG_TILE_ID;                                                                              \
        q_[0] = ta; q_[1] = tb; q_[2] = wall_clock64();                                                                       \
        q_[3] = ((long)__builtin_amdgcn_s_getreg((31 << 11) | 4)) | ((long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32); \
    }
#else
#define WG_TRACE_T(name)
#define WG_TRACE_END(N, ta, tb)
#endif

template <class EpiF>
__global__ __launch_bounds__(256, 2) void gemm_flat_kernel(GemmSegs S, long M, int N, EpiF epi, int vec) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tiles_n = (N + GBN - 1) / GBN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const long m0 = (long)(bid / tiles_n) * GBM;
    const int n0 = (bid % tiles_n) * GBN;
    RowMap rm{m0, 1, (int)((M - m0) < GBM ? (M - m0) : GBM)};
    GemmCore core(S, rm, n0, N, lds);
    core.find_regions();
    f32x16 acc[2][2];
    zero_acc(acc);
    core.run(acc);
    if (vec) core.for_each_vec(acc, epi);
    else core.for_each(acc, [&](int r, int c, float v) { epi(m0 + r, c, v); });
}

// Fast variant: straight-line K loop with interleaved loads (gemm_fast.h).  Requires vector-aligned
// operands, one B layout for all segments and N % 4 == 0; everything else takes the generic kernel.
template <class EpiF, class Core>
__global__ __launch_bounds__(256, 2) void gemm_flat_fast_kernel(GemmSegs S, long M, int N, EpiF epi, int relu_a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tiles_n = (N + GBN - 1) / GBN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const long m0 = (long)(bid / tiles_n) * GBM;
    const int n0 = (bid % tiles_n) * GBN;
    RowMap rm{m0, 1, (int)((M - m0) < GBM ? (M - m0) : GBM)};
    Core core(S, rm, n0, N, lds);
    core.fill_rowtab(epi);
    core.plan();
    f32x16 acc[2][2];
    zero_acc(acc);
    WG_TRACE_T(t_a);
    core.run(acc, relu_a != 0);
    WG_TRACE_T(t_b);
    core.for_each_vec(acc, epi);
    WG_TRACE_END(N, t_a, t_b);
}

// Split core with the compact LDS layout (two stages + table, epilogue in two 64-row halves): three workgroups per CU.
// NP = 0: fp32 planes on the fp32 MFMA; NP = 3: exact 3-way bf16 split (fp32-level accuracy); NP = 1: plain bf16 operands,
// fp32 accumulate (REGT_GEMM_MODE=bf16).
// (Persistent workgroups walking the tiles were tried and measured slower: the turn-around between two tiles of a slot
// goes from 7 us to 0.6 us, but the three workgroups of a CU then run in step -- all in their K loops, then all in their
// epilogues -- and the tile loop costs registers; gates GEMM 3.40 ms against 3.19 ms.  DESIGN.md section 6.)
template <class EpiF, bool REGION, int NP>
__global__ __launch_bounds__(256, 3) void gemm_flat_split_kernel(GemmSegs S, long M, int N, EpiF epi, int relu_a, int uniform) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tiles_n = (N + GBN - 1) / GBN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const long m0 = (long)(bid / tiles_n) * GBM;
    const int n0 = (bid % tiles_n) * GBN;
    RowMap rm{m0, 1, (int)((M - m0) < GBM ? (M - m0) : GBM)};
    WG_MARK(6);
    SplitCore<REGION, NP> core(S, rm, n0, N, lds, true);
    WG_MARK(7);
    core.fill_rowtab(epi);
    const bool uni = uniform != 0;                 // scalar slab descriptors (host: uniform_ok): no iteration table
    if (!uni) core.plan();
    f32x16 acc[2][2];
    // (the reset stays written out here: through zero_acc the compiler scheduled gemm_flat_split_kernel<EpiBiasActF, true, 0|3> differently)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    WG_TRACE_T(t_a);
    if (uni) core.run_uniform(acc, relu_a != 0);
    else core.run(acc, relu_a != 0);
    WG_TRACE_T(t_b);
    core.for_each_vec_halves(acc, epi);
    WG_TRACE_END(N, t_a, t_b);
}

// bf16-operand core + 8-column epilogue (bf16 storage of the activations): same K loop as gemm_flat_split_kernel<.., 1>
template <class EpiF8, bool REGION>
__global__ __launch_bounds__(256, 3) void gemm_flat_split8_kernel(GemmSegs S, long M, int N, EpiF8 epi, int uniform) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tiles_n = (N + GBN - 1) / GBN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const long m0 = (long)(bid / tiles_n) * GBM;
    const int n0 = (bid % tiles_n) * GBN;
    RowMap rm{m0, 1, (int)((M - m0) < GBM ? (M - m0) : GBM)};
    SplitCore<REGION, 1> core(S, rm, n0, N, lds, true);
    core.fill_rowtab(epi);
    const bool uni = uniform != 0;
    if (!uni) core.plan();
    f32x16 acc[2][2];
    zero_acc(acc);
    WG_TRACE_T(t_a);
    if (uniform == 2) core.run_uniform_frag(acc, false);
    else if (uni) core.run_uniform(acc, false);
    else core.run(acc, false);
    WG_TRACE_T(t_b);
    core.for_each_vec8_halves(acc, epi);
    WG_TRACE_END(N, t_a, t_b);
}

// Small problems: 64 x 64 tiles (gemm_small.h) -- same operands, segments and epilogues, a quarter of the work per tile.
template <class EpiF, bool BT, bool REGION>
__global__ __launch_bounds__(256, 4) void gemm_flat_small_kernel(GemmSegs S, long M, int N, EpiF epi, int relu_a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tiles_n = (N + SM_B - 1) / SM_B;
    const long m0 = (long)(blockIdx.x / tiles_n) * SM_B;
    const int n0 = (blockIdx.x % tiles_n) * SM_B;
    RowMap rm{m0, 1, (int)((M - m0) < SM_B ? (M - m0) : SM_B)};
    SmallCore<BT, REGION> core(S, rm, n0, N, lds);
    core.plan();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    core.run(acc, relu_a != 0);
    core.for_each_vec(acc, epi);
}

// ---- the ladder: small tiles / three-workgroup core / two-workgroup core / 8-column bf16 storage / generic --------------
template <class EpiF, class Core>
static int launch_fast_core(const GemmSegs& S, long M, int N, EpiF f, int relu, hipStream_t st) {
    long tiles;
    if (int rc = gemm_tiles(M, N, GBM, GBN, &tiles)) return rc;
    if (int rc = want_dynamic_lds<&gemm_flat_fast_kernel<EpiF, Core>>(G_FAST_LDS_BYTES)) return rc;
    hipLaunchKernelGGL((gemm_flat_fast_kernel<EpiF, Core>), dim3((unsigned)tiles), dim3(256), G_FAST_LDS_BYTES, st, S, M, N, f,
                       relu);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}
template <class EpiF, bool REGION, int NP>
static void launch_split(const GemmSegs& S, long M, int N, EpiF f, int relu, long tiles, hipStream_t st) {
    hipLaunchKernelGGL((gemm_flat_split_kernel<EpiF, REGION, NP>), dim3((unsigned)tiles), dim3(256), SplitGeom<NP>::LDS_BYTES, st, S, M, N, f, relu, uniform_ok(S, M));
}

template <class EpiF, bool BT, bool REGION>
static int launch_fast(const GemmSegs& S, long M, int N, EpiF f, int relu, hipStream_t st) {
    if (gemm_mode() == 0 && (long)cdiv(M, GBM) * cdiv(N, GBN) < SMALL_TILE_LIMIT) {
        const long tiles = (long)cdiv(M, SM_B) * cdiv(N, SM_B);
        hipLaunchKernelGGL((gemm_flat_small_kernel<EpiF, BT, REGION>), dim3((unsigned)tiles), dim3(256), SM_LDS_BYTES, st, S, M, N, f,
                           relu);
        REGT_CHECK_LAUNCH();
        return REGT_OK;
    }
    if constexpr (BT) {
        if (gemm_mode() != 0 || !fp32_core_wide()) {
            long tiles;
            if (int rc = gemm_tiles(M, N, GBM, GBN, &tiles)) return rc;
            if (gemm_mode() == 0) launch_split<EpiF, REGION, 0>(S, M, N, f, relu, tiles, st);
            else if (gemm_mode() == 1) launch_split<EpiF, REGION, 3>(S, M, N, f, relu, tiles, st);
            else launch_split<EpiF, REGION, 1>(S, M, N, f, relu, tiles, st);
            REGT_CHECK_LAUNCH();
            return REGT_OK;
        }
    }
    return launch_fast_core<EpiF, FastCore<BT, REGION>>(S, M, N, f, relu, st);
}

// bf16-operand core with the 8-column epilogue: arrays of the epilogue may be stored as bf16
template <class EpiF8, bool REGION>
static int launch_split8(const GemmSegs& S, long M, int N, EpiF8 f, hipStream_t st) {
    REGT_CHECK_ARG(gemm_mode() == 2 && N % 8 == 0, "gemm: bf16-stored activations need REGT_GEMM_MODE=bf16 and N %% 8 == 0");
    for (int q = 0; q < S.nseg; ++q)
        REGT_CHECK_ARG(!(S.seg[q].flags & SEG_B_FRAG) || uniform_ok(S, M) == 2, "gemm: fragment-order weights need every segment in that order and K %% 32 == 0");
    long tiles;
    if (int rc = gemm_tiles(M, N, GBM, GBN, &tiles)) return rc;
    hipLaunchKernelGGL((gemm_flat_split8_kernel<EpiF8, REGION>), dim3((unsigned)tiles), dim3(256), SplitGeom<1>::LDS_BYTES, st, S, M, N, f, uniform_ok(S, M));
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

template <class EpiF>
static int launch_flat(const GemmSegs& S, long M, int N, EpiF f, bool vec, hipStream_t st) {
    REGT_CHECK_ARG(M > 0 && N > 0, "gemm: empty problem M=%ld N=%d", M, N);
    for (int q = 0; q < S.nseg; ++q)
        REGT_CHECK_ARG(!(S.seg[q].flags & SEG_A_BF16), "gemm: a bf16-stored operand needs the bf16-operand vector path");
    long tiles;
    if (int rc = gemm_tiles(M, N, GBM, GBN, &tiles)) return rc;
    if (int rc = want_dynamic_lds<&gemm_flat_kernel<EpiF>>(G_LDS_BYTES)) return rc;
    hipLaunchKernelGGL(gemm_flat_kernel<EpiF>, dim3((unsigned)tiles), dim3(256), G_LDS_BYTES, st, S, M, N, f, vec ? 1 : 0);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace regt
