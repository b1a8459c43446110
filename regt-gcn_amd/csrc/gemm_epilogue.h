// Device helpers shared by the epilogues of the dense contractions (gemm_fwd.hip, gemm_cell.hip): the fast
// sigmoid / tanh, 16-byte loads and stores of 4 and 8 columns, the one fp32 -> bf16 pack and the accumulator reset.
#pragma once
#include "kernels.h"

// Developer build (-DREGT_WG_TRACE, tools/wg_trace.py): the trace arrays are __device__ globals, one copy per translation unit,
// and the two readers copy out gemm_fwd.hip's.  Only that unit (it defines REGT_WG_TRACE_UNIT) keeps the marks inside the cores;
// in every other unit they expand to nothing.
#if defined(REGT_WG_TRACE) && !defined(REGT_WG_TRACE_UNIT)
#undef WG_MARK
#define WG_MARK(i) do { } while (0)
#endif
#include "gemm_fast.h"
#include "gemm_split.h"
#include "gemm_small.h"

namespace regt {

// ---- epilogue functors ---------------------------------------------------------------------------
// Each functor has a scalar form (m, c, v) used when the output is not 16-byte tileable (e.g. the
// (N, O) head output) and a vector form: load() fetches the auxiliary operands of one float4,
// apply() finishes and stores it (driver: GemmCore::for_each_vec).
//
// Straight-line variants (vcol<V> / vtile<V> / vload<V> / vapply<V>, drivers: FastCore::for_each_vec, SplitCore::for_each_vec_halves):
// every decision of the functor that is uniform over a tile (which activation, bf16 or fp32 store, does this column tile
// hold the r gate, ...) is folded into the compile-time variant V = variant(n0) in [0, NVAR) -- or -1: no specialisation,
// use load/apply.  For a full tile the driver then runs a body without a single branch.  That is what keeps hipcc's
// s_waitcnt exact: with per-row `if`s every row of the epilogue became its own basic block and waited vmcnt(0) -- for
// its own loads AND for the stores of the row before it (stores count on vmcnt on gfx9): a chain of one memory round trip
// per row, 11 us (two-workgroup core) to 21 us (three-workgroup core) per 128 x 128 tile (tools/wg_trace.py).
// Column constants (bias) are loaded once per thread (Col), not once per row.
// Addresses: per array one buffer descriptor for the tile's origin (SGPRs), one per-thread byte offset (vtile) and a
// wave-uniform row step: loads take it as the instruction's scalar offset (no vector instruction per row goes into their
// addressing), STORES add it to the vector offset and keep soffset = 0.  A 16-byte buffer store with an SGPR soffset
// whose data registers the very next VALU instruction overwrites picked up the NEW value now and then on gfx950 (the
// first dword of a row came out as 1 + e^-x instead of the sigmoid: tests/test_gpu_ops.py::test_linear_sigmoid_rows); the
// compiler only pads that hazard with a wait state when soffset is an immediate (GCNHazardRecognizer: "this hazard only
// exists if the instruction is not using a register in the soffset field").  That matters more than it looks: a wave that shares its SIMD with waves streaming MFMAs gets a VALU issue
// slot only every ~64-200 cycles (tools/micro/valu_under_mfma.hip: 10x slower next to two MFMA-bound waves, whatever its
// s_setprio), so the epilogue's duration is its VALU instruction count times that, not its memory traffic.
//
// Where the compiler allows it, the per-element arithmetic of an epilogue is ONE __device__ function next to its functors, called
// by the scalar form, apply(), vapply<V>() and both widths through REGT_V4 / REGT_F8, so that the guarded path of a partial tile
// cannot round differently from the straight-line path of its full neighbour.  Where stating it once changed a kernel's machine
// code the forms stay written out, with a note (profiles/gemm_units_isa.txt lists them).
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float fast_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// two fp32 -> two bf16 in one dword (round to nearest even, v_cvt_pk_bf16_f32): the one pack of every bf16 store below
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t f = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2_t));
}
// four fp32 -> four bf16, one 8-byte store; `elem` addresses bf16 elements
__device__ __forceinline__ void st4_bf16(void* base, long elem, float4 v) {
    *reinterpret_cast<uint2*>(reinterpret_cast<char*>(base) + 2 * elem) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
}
#define REGT_V4(expr_x) make_float4(expr_x(x), expr_x(y), expr_x(z), expr_x(w))

// ---- 8 columns per thread (bf16-operand core with bf16 STORAGE of the M x C activations) ---------------------------------
// A thread owns 8 consecutive columns of a row: 16 bytes of a bf16 array, two float4 of an fp32 one -- every access of the
// epilogue stays 16 bytes wide whichever format an array has (8-byte accesses run at about half the rate).
// Functor interface: ColAux col(c) once per thread (bias), Aux load(m, c) per row (the first round is requested before the
// accumulators are staged), apply(m, c, v, col, aux).  `bf` flags are wave-uniform.
struct F8 { float4 lo, hi; };
#define REGT_F8(expr) F8{make_float4(expr(lo.x), expr(lo.y), expr(lo.z), expr(lo.w)), make_float4(expr(hi.x), expr(hi.y), expr(hi.z), expr(hi.w))}
__device__ __forceinline__ u32x4_t pack_bf16x8(const F8& v) {
    return u32x4_t{pack_bf16x2(v.lo.x, v.lo.y), pack_bf16x2(v.lo.z, v.lo.w), pack_bf16x2(v.hi.x, v.hi.y), pack_bf16x2(v.hi.z, v.hi.w)};
}
__device__ __forceinline__ F8 ld8(const void* base, long elem, int bf) {
    F8 r;
    if (bf) {
        const uint4 raw = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(base) + 2 * elem);
        r.lo = widen_bf16x4(raw.x, raw.y);
        r.hi = widen_bf16x4(raw.z, raw.w);
    } else {
        const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + 4 * elem);
        r.lo = p[0];
        r.hi = p[1];
    }
    return r;
}
__device__ __forceinline__ void st8(void* base, long elem, const F8& v, int bf) {
    if (bf) {
        const u32x4_t w = pack_bf16x8(v);
        *reinterpret_cast<uint4*>(reinterpret_cast<char*>(base) + 2 * elem) = make_uint4(w.x, w.y, w.z, w.w);
    } else {
        float4* p = reinterpret_cast<float4*>(reinterpret_cast<char*>(base) + 4 * elem);
        p[0] = v.lo;
        p[1] = v.hi;
    }
}
// 16 bytes = 8 bf16 through a buffer descriptor (straight-line variants; stores keep soffset = 0, see the note on top)
__device__ __forceinline__ u32x4_t buf_ld16(__amdgpu_buffer_rsrc_t r, int voff, int soff) { return __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0); }
__device__ __forceinline__ F8 widen8(u32x4_t raw) { return F8{widen_bf16x4(raw.x, raw.y), widen_bf16x4(raw.z, raw.w)}; }
__device__ __forceinline__ void buf_st8_bf16(__amdgpu_buffer_rsrc_t r, int voff, const F8& v) {
    __builtin_amdgcn_raw_buffer_store_b128(pack_bf16x8(v), r, voff, 0, 0);
}

// the accumulators of a tile (128 x 128: [2][2]; the weight gradients have other shapes, wgrad_common.h), before the K loop
template <int MI, int NJ>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[MI][NJ]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

}  // namespace regt
