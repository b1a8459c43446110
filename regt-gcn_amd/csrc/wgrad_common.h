// What the weight-gradient GEMM kernels (wgrad_fp32.hip, wgrad_bf16.hip) share: the stages every one of them runs between its
// first line and its K loop -- which (chunk, tile) a workgroup works on, the chunk's rows, its clamped descriptors -- the small
// float4 helpers of their staging passes, and the one launch their two launchers are made of.  A kernel in which stating a
// stage through its helper changed the machine code keeps the stage written out, with a note; the slab store is written out in
// all of them for that reason (profiles/wgrad_units_isa.txt).
#pragma once
#include "kernels.h"
#include "gemm_epilogue.h"

namespace regt {

// Tile 128 (Nout) x BNW (Nin), K = rows of P/Q.  Both operands are staged k-major ([k][i]) exactly
// as they lie in HBM (row m contiguous along i), read back with conflict-free ds_read_b32.
constexpr int W_BK = 32;
constexpr int W_LDP = 128 + 4;
constexpr int WS_PLANE_B = 16 * 256;             // bf16 pipe: one plane of one operand of one half slab (wgrad_bf16.hip)

// Which (row chunk, output tile) workgroup blockIdx.x works on, `tpc` tiles per chunk.
// XCD-aware mapping: all tiles of one row chunk run on the same XCD (workgroup b lands on XCD b % 8), back to
// back, so the chunk's P and Q rows are fetched from HBM once and served to the other tiles from that XCD's L2.
struct WgradBlock { int tile, chunk; };
__device__ __forceinline__ WgradBlock wgrad_block(int nchunks, int tpc) {
    WgradBlock w;
    const int nfull = (nchunks / 8) * 8;                   // chunks that can be dealt 8 at a time
    const int b = blockIdx.x;
    if (b < nfull * tpc) {
        const int xcd = b & 7, li = b >> 3;
        w.chunk = (li / tpc) * 8 + xcd;
        w.tile = li % tpc;
    } else {                                               // remainder chunks: plain order
        const int r = b - nfull * tpc;
        w.chunk = nfull + r / tpc;
        w.tile = r % tpc;
    }
    return w;
}
// The rows [r0, r1) of a chunk: from the table, or `kchunk` rows each
struct WgradRows { long r0, r1; };
__device__ __forceinline__ WgradRows wgrad_chunk_rows(const WgradArgs& a, int chunk) {
    long r0, r1;
    if (a.chunk_tab) { r0 = a.chunk_tab[2 * chunk]; r1 = a.chunk_tab[2 * chunk + 1]; }
    else { r0 = (long)chunk * a.kchunk; r1 = r0 + a.kchunk < a.M ? r0 + a.kchunk : a.M; }
    return WgradRows{r0, r1};
}
// two loads of the same slot through descriptors with complementary out-of-range masks (an out-of-range lane returns 0)
__device__ __forceinline__ float4 or4(float4 a, float4 b) {
    return make_float4(__uint_as_float(__float_as_uint(a.x) | __float_as_uint(b.x)), __uint_as_float(__float_as_uint(a.y) | __float_as_uint(b.y)),
                       __uint_as_float(__float_as_uint(a.z) | __float_as_uint(b.z)), __uint_as_float(__float_as_uint(a.w) | __float_as_uint(b.w)));
}
__device__ __forceinline__ float4 relu4(float4 v) { return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)); }
// Descriptor over `bytes` from `base` (the chunk's first row: a row past the chunk's end is out of range), clamped to what a descriptor holds
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wgrad_chunk_desc(const void* base, long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(bytes < 0x7FFFFFF0L ? bytes : 0x7FFFFFF0L), 0x00020000);
}
// One launch of kernel `Kernel` as wgrad_pick sized it (the launchers of the two kernel units are a switch over this).
template <auto Kernel>
static int wgrad_launch(const WgradPick& p, const WgradArgs& a, hipStream_t st) {
    if (p.raise_lds) { if (int rc = want_dynamic_lds<Kernel>((int)p.lds)) return rc; }
    hipLaunchKernelGGL(Kernel, dim3((unsigned)p.blocks), dim3(256), p.lds, st, a);
    return REGT_OK;
}

}  // namespace regt
