// What the aggregation units share: the record of a problem and of the plan spmm_pick (spmm_dispatch.hip) makes for it, the
// launch entry of each kernel unit, and the 16-byte row pieces of the panel and row-block kernels (spmm_panel.hip).
#pragma once
#include "gemm_epilogue.h"      // pack_bf16x2: the library's one fp32 -> bf16 pair conversion

namespace regt {

// ---- the problem, and what runs for it --------------------------------------------------------------------------------------
enum SpmmForm : int { SP_SINGLE, SP_DUAL, SP_DUAL_BF16 };            // one operator (nstack stacked) | merged two-weight CSR, fp32 rows | bf16 rows
enum SpmmFamily : int { SP_CSR, SP_CSR_PASSES, SP_PANEL, SP_ROWS };  // lane group per row | the same in column passes | column panels | row blocks
struct SpmmProblem {
    SpmmForm form;
    int nrows, nstack;      // rows of the output (nstack operators of nrows / nstack nodes each; the dual forms: nstack = 1)
    int x_rows, W;          // rows of X, row width in elements
    bool aligned;           // X and the outputs are 16-byte aligned (asked of SP_SINGLE only)
};
struct SpmmPlan {
    SpmmFamily family;
    bool dual, bf;          // the kernel's DUAL and BF arguments (SP_PANEL: which of the three panel kernels)
    const struct SpRung* rung;      // SP_CSR, SP_CSR_PASSES: the rung of the form's ladder (lanes per row G, float4 chunks per lane CH)
    int PL;                 // SP_PANEL, SP_ROWS: lanes per row = panel width in 16-byte pieces (IDX = PL)
    int nnodes, nstack, x_rows;
    int W16;                // row width in 16-byte pieces (W4 of fp32 rows, W16 of bf16 rows)
    int pass16;             // SP_CSR_PASSES: 16-byte pieces per pass (the last pass takes what is left)
    int npanels, nrb, rpg, cap, rowbytes;
    unsigned x_bytes, y_bytes;
    long grid;
    int lds;                // dynamic LDS bytes
};
// Launches nothing; every refusal of launch_spmm_csr / launch_spmm_dual_x / launch_spmm_dual_bf16 is made here.
int spmm_pick(const SpmmProblem& p, SpmmPlan* plan);

struct SpmmPtrs { const int *rowptr, *col; const float *val_a, *val_l; const void* X; void *YA, *YL; };
// a rung of a lane-group ladder (spmm_csr.hip): rows of at most max_w4 float4 run on <G, CH>
struct SpRung { int max_w4, G, CH; void (*launch)(const SpmmPlan& k, const SpmmPtrs& a, int c4, int w4, hipStream_t st); };
struct SpLadder { const SpRung* rungs; int n; };
SpLadder spmm_ladder(bool merged);          // the single-operator ladder (9 rungs) or the merged one (7), widest row last: 512 float4
int spmm_launch_csr(const SpmmPlan& k, const SpmmPtrs& a, hipStream_t st);      // spmm_csr.hip: SP_CSR, SP_CSR_PASSES
int spmm_launch_panel(const SpmmPlan& k, const SpmmPtrs& a, hipStream_t st);    // spmm_panel.hip: SP_PANEL, SP_ROWS

// an empty accumulator, and what a lane past the row's width or past the live entries gathers
__device__ __forceinline__ float4 sp_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
// XCD x (workgroups land on XCD blockIdx.x % 8) owns the contiguous node chunk [c0, c0 + csz): the first nnodes % 8 chunks hold one more
struct SpChunk { int c0, csz; };
__device__ __forceinline__ SpChunk sp_chunk(int xcd, int nnodes) {
    const int q = nnodes / 8, r8 = nnodes % 8;
    return {xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q, q + (xcd < r8 ? 1 : 0)};
}
// streaming store of one 16-byte piece: the outputs are not read again by the kernel and must not evict the XCD's slice of X from its L2
__device__ __forceinline__ void sp_store_nt(float4* p, const float4& v) {
    __builtin_nontemporal_store(v.x, &p->x); __builtin_nontemporal_store(v.y, &p->y);
    __builtin_nontemporal_store(v.z, &p->z); __builtin_nontemporal_store(v.w, &p->w);
}

// ---- 16 bytes per lane of either row format: 4 fp32 or 8 bf16 elements; fp32 accumulation, one rounding at the end ----------
struct SpEnt { int col; float wa, wl; int pad; };
template <bool BF> struct SpAcc { float v[BF ? 8 : 4]; };
template <bool BF>
__device__ __forceinline__ void sp_fma(SpAcc<BF>& a, float w, const u32x4_t& x) {
    if constexpr (BF) {
        a.v[0] = fmaf(w, __uint_as_float(x.x << 16), a.v[0]); a.v[1] = fmaf(w, __uint_as_float(x.x & 0xffff0000u), a.v[1]);
        a.v[2] = fmaf(w, __uint_as_float(x.y << 16), a.v[2]); a.v[3] = fmaf(w, __uint_as_float(x.y & 0xffff0000u), a.v[3]);
        a.v[4] = fmaf(w, __uint_as_float(x.z << 16), a.v[4]); a.v[5] = fmaf(w, __uint_as_float(x.z & 0xffff0000u), a.v[5]);
        a.v[6] = fmaf(w, __uint_as_float(x.w << 16), a.v[6]); a.v[7] = fmaf(w, __uint_as_float(x.w & 0xffff0000u), a.v[7]);
    } else {
        a.v[0] = fmaf(w, __uint_as_float(x.x), a.v[0]); a.v[1] = fmaf(w, __uint_as_float(x.y), a.v[1]);
        a.v[2] = fmaf(w, __uint_as_float(x.z), a.v[2]); a.v[3] = fmaf(w, __uint_as_float(x.w), a.v[3]);
    }
}
template <bool BF>
__device__ __forceinline__ u32x4_t sp_pack(const SpAcc<BF>& a) {
    if constexpr (BF) {
        u32x4_t r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = pack_bf16x2(a.v[2 * i], a.v[2 * i + 1]);
        return r;
    } else {
        return u32x4_t{__float_as_uint(a.v[0]), __float_as_uint(a.v[1]), __float_as_uint(a.v[2]), __float_as_uint(a.v[3])};
    }
}

}  // namespace regt
