// Forward GEMMs of the pipeline: bias + activation (embedding, head, zero-hidden cell) and the [Z | R] gates with q = R h,
// each as a 4-column epilogue (fp32 storage) and an 8-column one (bf16 storage) on the kernels of gemm_flat.h.
// Developer build (-DREGT_WG_TRACE): this is the traced unit -- tools/wg_trace.py looks at the gates GEMM (N = 2C) or, forward
// only, at the regional embedding (N = C); the trace arrays and their two readers live here.
#define REGT_WG_TRACE_UNIT
#include "gemm_epilogue.h"
#ifdef REGT_WG_TRACE
namespace regt {
__device__ long g_wg_trace[4 * WG_TRACE_MAX];
__device__ long g_wg_marks[8 * WG_TRACE_MAX];
}  // namespace regt
#endif
#include "gemm_flat.h"

namespace regt {

// ---- out = act(v + bias) -----------------------------------------------------------------------------------------------
// none / leaky_relu / relu are all "x > 0 ? x : x * ns" with ns = 1 / slope / 0 (act_slope); sigmoid / tanh for the gate GEMMs of the
// zero-hidden cell (regt_cell0_forward).  act_select<V>: 0 = the select, 1 = sigmoid, 2 = tanh; bias_act: e.act decides at run
// time (scalar form and the guarded path of both widths).  The straight-line vapply<V> bodies keep the select written out with
// ns formed once per call: through act_select<V> the compiler scheduled four kernels differently (profiles/gemm_units_isa.txt).
__device__ __forceinline__ float act_slope(const EpiBiasAct& e) { return e.act == ACT_NONE ? 1.0f : (e.act == ACT_LRELU ? e.slope : 0.0f); }
template <int V>
__device__ __forceinline__ float act_select(float x, float ns) { return V == 1 ? fast_sigmoid(x) : V == 2 ? fast_tanh(x) : (x > 0.f ? x : x * ns); }
__device__ __forceinline__ float bias_act(const EpiBiasAct& e, float x) {
    if (e.act == ACT_SIGMOID) return act_select<1>(x, 0.f);
    if (e.act == ACT_TANH) return act_select<2>(x, 0.f);
    return act_select<0>(x, act_slope(e));
}
__device__ __forceinline__ int bias_act_variant(const EpiBiasAct& e) { return e.act == ACT_SIGMOID ? 1 : (e.act == ACT_TANH ? 2 : 0); }

struct EpiBiasActF {
    EpiBiasAct e;
    __device__ __forceinline__ void operator()(long m, int c, float v) const {
        e.out[m * e.ldo + c] = bias_act(e, v + (e.bias ? e.bias[c] : 0.f));
    }
    static constexpr int ROUND_ROWS = 16;
    struct Aux { float4 b; };
    __device__ __forceinline__ Aux load(long, int c) const { return Aux{e.bias ? ld4(e.bias + c) : make_float4(0, 0, 0, 0)}; }
    __device__ __forceinline__ void apply(long m, int c, float4 v, const Aux& a) const {
#define F_(k) bias_act(e, v.k + a.b.k)
        st4(e.out + m * e.ldo + c, REGT_V4(F_));
#undef F_
    }
    // variants: 0 = none / leaky relu / relu (one select), 1 = sigmoid, 2 = tanh
    static constexpr int NVAR = 3;
    static constexpr bool HAS_ROWTAB = false;
    struct Col { float4 b; };
    struct VAux {};
    struct Tile { __amdgpu_buffer_rsrc_t out; int v, s; };
    // (-1 = the guarded path: the straight-line body addresses a tile with 32-bit byte offsets, 120 rows x ldo x 4 B must fit)
    __device__ __forceinline__ int variant(int) const { return e.ldo >= (1L << 22) ? -1 : bias_act_variant(e); }
    template <int V> __device__ __forceinline__ Col vcol(int c) const { return Col{e.bias ? ld4(e.bias + c) : make_float4(0, 0, 0, 0)}; }
    template <int V> __device__ __forceinline__ Tile vtile(const EpiGeom& g) const {
        return Tile{buf_srd(e.out + g.m0 * e.ldo + g.n0), (g.rr * (int)e.ldo + g.c) * 4, g.step * (int)e.ldo * 4};
    }
    template <int V> __device__ __forceinline__ VAux vload(const Tile&, int) const { return VAux{}; }
    template <int V> __device__ __forceinline__ void vapply(const Tile& t, int i, float4 v, const Col& col, const VAux&) const {
        const float ns = e.act == ACT_NONE ? 1.0f : (e.act == ACT_LRELU ? e.slope : 0.0f);
#define F_(k) (V == 1 ? fast_sigmoid(v.k + col.b.k) : V == 2 ? fast_tanh(v.k + col.b.k) : ((v.k + col.b.k) > 0.f ? (v.k + col.b.k) : (v.k + col.b.k) * ns))
        buf_st4(t.out, t.v + i * t.s, 0, REGT_V4(F_));
#undef F_
    }
};
struct EpiBiasAct8F {
    typedef F8 Vec;
    EpiBiasAct e;
    static constexpr int ROUND_ROWS = 4;
    struct ColAux { F8 b; };
    struct Aux {};
    __device__ __forceinline__ ColAux col(int c) const {
        return ColAux{e.bias ? ld8(e.bias, c, 0) : F8{make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0)}};
    }
    __device__ __forceinline__ Aux load(long, int) const { return Aux{}; }
    __device__ __forceinline__ void apply(long m, int c, const F8& v, const ColAux& ca, const Aux&) const {
#define F_(k) bias_act(e, v.k + ca.b.k)
        st8(e.out, m * e.ldo + c, REGT_F8(F_), e.out_bf16);
#undef F_
    }
    // straight-line variants (bf16 output): 0 = none / leaky relu / relu, 1 = sigmoid, 2 = tanh
    static constexpr int NVAR = 3;
    static constexpr bool HAS_ROWTAB = false;
    typedef ColAux Col;
    struct VAux {};
    struct Tile { __amdgpu_buffer_rsrc_t out; int v, s; };
    __device__ __forceinline__ int variant(int) const { return (!e.out_bf16 || e.ldo >= (1L << 22)) ? -1 : bias_act_variant(e); }
    template <int V> __device__ __forceinline__ Col vcol(int c) const { return col(c); }
    template <int V> __device__ __forceinline__ Tile vtile(const EpiGeom& g) const {
        return Tile{buf_srd(reinterpret_cast<const char*>(e.out) + 2 * (g.m0 * e.ldo + g.n0)), (g.rr * (int)e.ldo + g.c) * 2, g.step * (int)e.ldo * 2};
    }
    template <int V> __device__ __forceinline__ VAux vload(const Tile&, int) const { return VAux{}; }
    template <int V> __device__ __forceinline__ void vapply(const Tile& t, int i, const F8& v, const Col& ca, const VAux&) const {
        const float ns = e.act == ACT_NONE ? 1.0f : (e.act == ACT_LRELU ? e.slope : 0.0f);
#define F_(k) (V == 1 ? fast_sigmoid(v.k + ca.b.k) : V == 2 ? fast_tanh(v.k + ca.b.k) : ((v.k + ca.b.k) > 0.f ? (v.k + ca.b.k) : (v.k + ca.b.k) * ns))
        buf_st8_bf16(t.out, t.v + i * t.s, REGT_F8(F_));
#undef F_
    }
};

// ---- [Z | R] = sigmoid(v + bias), q = h R ------------------------------------------------------------------------------
// One gate and one product for every form and width.  The backward pass forms R (1 - R) from the stored gate, and for a
// saturated gate one ulp of R is a percent of 1 - R -- a tile must not round differently from its partial neighbour (folding
// the bias into the exponent's fma saved a VALU per element and moved the r-gate gradients by 1 %).
__device__ __forceinline__ float gate(float v, float b) { return fast_sigmoid(v + b); }
__device__ __forceinline__ float gated(float h, float g) { return h * g; }

// SAVE_R = false (forward-only calls, REGT_DIMS_FORWARD_ONLY): R is formed and multiplied into q exactly as before but not stored --
// only the backward pass reads it; Z and q are (the candidate kernel reads both).  Same arithmetic, one store per r element less.
template <bool SAVE_R>
struct EpiGatesT {
    EpiGates e;
    __device__ __forceinline__ void operator()(long m, int c, float v) const {
        float g = gate(v, e.bias[c]);
        if (SAVE_R || c < e.C) e.ZR[m * (2L * e.C) + c] = g;
        if (c >= e.C) e.q[m * e.C + c - e.C] = gated(e.h[m * e.C + c - e.C], g);      // fp32 storage only (vector path handles bf16)
    }
    static constexpr int ROUND_ROWS = 16;
    struct Aux { float4 b, h; };
    __device__ __forceinline__ Aux load(long m, int c) const {
        Aux a;
        a.b = ld4(e.bias + c);
        a.h = c >= e.C ? ld4(e.h + m * e.C + c - e.C) : make_float4(0, 0, 0, 0);
        return a;
    }
    __device__ __forceinline__ void apply(long m, int c, float4 v, const Aux& a) const {
#define F_(k) gate(v.k, a.b.k)
        const float4 g = REGT_V4(F_);
#undef F_
        if (SAVE_R || c < e.C) st4(e.ZR + m * (2L * e.C) + c, g);
        if (c >= e.C) {
#define F_(k) gated(a.h.k, g.k)
            const float4 qv = REGT_V4(F_);
#undef F_
            if (e.q_bf16) st4_bf16(e.q, m * e.C + c - e.C, qv);
            else st4(e.q + m * e.C + c - e.C, qv);
        }
    }
    // variants: bit 0 = the tile holds r columns (reads h, writes q = r * h), bit 1 = q stored as bf16; tiles are pure z
    // or pure r when C is a multiple of the tile width.  The arithmetic is load()/apply()'s to the bit (gate / gated above).
    static constexpr int NVAR = 4;
    static constexpr bool HAS_ROWTAB = false;
    struct Col { float4 b; };
    struct VAux { float4 h; };
    struct Tile { __amdgpu_buffer_rsrc_t zr, h, q; int vzr, vh, vq, szr, sh, sq; };
    __device__ __forceinline__ int variant(int n0) const { return e.C % GBN ? -1 : (n0 >= e.C ? 1 : 0) + (e.q_bf16 ? 2 : 0); }
    template <int V> __device__ __forceinline__ Col vcol(int c) const { return Col{ld4(e.bias + c)}; }
    template <int V> __device__ __forceinline__ Tile vtile(const EpiGeom& g) const {
        Tile t;
        if (SAVE_R || !(V & 1)) {
            t.zr = buf_srd(e.ZR + g.m0 * (2L * e.C) + g.n0);
            t.vzr = (g.rr * 2 * e.C + g.c) * 4;
            t.szr = g.step * 2 * e.C * 4;
        }
        if (V & 1) {
            const long o = g.m0 * e.C + g.n0 - e.C;
            t.h = buf_srd(e.h + o);
            t.vh = (g.rr * e.C + g.c) * 4;
            t.sh = g.step * e.C * 4;
            t.q = buf_srd((V & 2) ? reinterpret_cast<const char*>(e.q) + 2 * o : reinterpret_cast<const char*>(e.q) + 4 * o);
            t.vq = (V & 2) ? t.vh >> 1 : t.vh;
            t.sq = (V & 2) ? t.sh >> 1 : t.sh;
        }
        return t;
    }
    template <int V> __device__ __forceinline__ VAux vload(const Tile& t, int i) const {
        VAux a;
        if (V & 1) a.h = buf_ld4(t.h, t.vh, i * t.sh);
        return a;
    }
    template <int V> __device__ __forceinline__ void vapply(const Tile& t, int i, float4 v, const Col& col, const VAux& a) const {
#define F_(k) gate(v.k, col.b.k)
        const float4 g = REGT_V4(F_);
#undef F_
        if (SAVE_R || !(V & 1)) buf_st4(t.zr, t.vzr + i * t.szr, 0, g);
        if (V & 1) {
#define F_(k) gated(a.h.k, g.k)
            const float4 qv = REGT_V4(F_);
#undef F_
            if (V & 2) buf_st4_bf16(t.q, t.vq + i * t.sq, 0, qv);
            else buf_st4(t.q, t.vq + i * t.sq, 0, qv);
        }
    }
};
struct EpiGatesF : EpiGatesT<true> {};
struct EpiGatesFwdF : EpiGatesT<false> {};
template <bool SAVE_R>     // (as EpiGatesT)
struct EpiGates8T {
    typedef F8 Vec;
    EpiGates e;
    static constexpr int ROUND_ROWS = 4;
    struct ColAux { F8 b; };
    struct Aux { F8 h; };
    __device__ __forceinline__ ColAux col(int c) const { return ColAux{ld8(e.bias, c, 0)}; }
    __device__ __forceinline__ Aux load(long m, int c) const {
        Aux a;
        if (c >= e.C) a.h = ld8(e.h, m * e.C + c - e.C, e.h_bf16);
        return a;
    }
    __device__ __forceinline__ void apply(long m, int c, const F8& v, const ColAux& ca, const Aux& a) const {
#define F_(k) gate(v.k, ca.b.k)
        const F8 g = REGT_F8(F_);
#undef F_
        if (SAVE_R || c < e.C) st8(e.ZR, m * (2L * e.C) + c, g, e.zr_bf16);
        if (c >= e.C) {
#define F_(k) gated(a.h.k, g.k)
            st8(e.q, m * e.C + c - e.C, REGT_F8(F_), e.q_bf16);
#undef F_
        }
    }
    // straight-line variants (h, [Z|R] and q all stored as bf16): bit 0 = the tile holds r columns
    static constexpr int NVAR = 2;
    static constexpr bool HAS_ROWTAB = false;
    typedef ColAux Col;
    struct VAux { u32x4_t h; };
    struct Tile { __amdgpu_buffer_rsrc_t zr, h, q; int vzr, vh, szr, sh; };
    __device__ __forceinline__ int variant(int n0) const { return (e.C % GBN || !e.h_bf16 || !e.zr_bf16 || !e.q_bf16) ? -1 : (n0 >= e.C ? 1 : 0); }
    template <int V> __device__ __forceinline__ Col vcol(int c) const { return col(c); }
    template <int V> __device__ __forceinline__ Tile vtile(const EpiGeom& g) const {
        Tile t;
        if (SAVE_R || !(V & 1)) {
            t.zr = buf_srd(reinterpret_cast<const char*>(e.ZR) + 2 * (g.m0 * (2L * e.C) + g.n0));
            t.vzr = (g.rr * 2 * e.C + g.c) * 2;
            t.szr = g.step * 2 * e.C * 2;
        }
        if (V & 1) {
            const long o = g.m0 * e.C + g.n0 - e.C;
            t.h = buf_srd(reinterpret_cast<const char*>(e.h) + 2 * o);
            t.q = buf_srd(reinterpret_cast<const char*>(e.q) + 2 * o);
            t.vh = (g.rr * e.C + g.c) * 2;
            t.sh = g.step * e.C * 2;
        }
        return t;
    }
    template <int V> __device__ __forceinline__ VAux vload(const Tile& t, int i) const {
        VAux a;
        if (V & 1) a.h = buf_ld16(t.h, t.vh, i * t.sh);
        return a;
    }
    template <int V> __device__ __forceinline__ void vapply(const Tile& t, int i, const F8& v, const Col& ca, const VAux& a) const {
#define F_(k) gate(v.k, ca.b.k)
        const F8 g = REGT_F8(F_);
#undef F_
        if (SAVE_R || !(V & 1)) buf_st8_bf16(t.zr, t.vzr + i * t.szr, g);
        if (V & 1) {
            const F8 h = widen8(a.h);
#define F_(k) gated(h.k, g.k)
            buf_st8_bf16(t.q, t.vh + i * t.sh, REGT_F8(F_));
#undef F_
        }
    }
};
struct EpiGates8F : EpiGates8T<true> {};
struct EpiGates8FwdF : EpiGates8T<false> {};

int launch_gemm_bias_act(const GemmSegs& S, long M, int N, const EpiBiasAct& e, hipStream_t st) {
    const bool vec = N % 4 == 0 && e.ldo % 4 == 0 && a16(e.out) && a16(e.bias);
    const int fc = fast_class(S, N, vec);
    if (e.out_bf16) {
        REGT_CHECK_ARG(fc >= 0 && (fc & 1) && !(fc & 4) && e.ldo % 8 == 0, "bias/act gemm: bf16 output needs the bf16-operand vector path");
        return with_flag(fc & 2, [&](auto region) { return launch_split8<EpiBiasAct8F, decltype(region)::value>(S, M, N, EpiBiasAct8F{e}, st); });
    }
    if (fc >= 0 && (fc & 1))
        return with_flag(fc & 2, [&](auto region) { return launch_fast<EpiBiasActF, true, decltype(region)::value>(S, M, N, EpiBiasActF{e}, (fc >> 2) & 1, st); });
    return launch_flat(S, M, N, EpiBiasActF{e}, vec, st);
}
int launch_gemm_gates(const GemmSegs& S, long M, int N, const EpiGates& e, hipStream_t st, bool save_r) {
    REGT_CHECK_ARG(N == 2 * e.C, "gates gemm expects N == 2C");
    const bool vec = e.C % 4 == 0 && a16(e.ZR) && a16(e.h) && a16(e.q) && a16(e.bias);
    return with_flag(save_r, [&](auto save) -> int {
        using Epi = std::conditional_t<decltype(save)::value, EpiGatesF, EpiGatesFwdF>;
        using Epi8 = std::conditional_t<decltype(save)::value, EpiGates8F, EpiGates8FwdF>;
        if (e.h_bf16 || e.zr_bf16) {
            REGT_CHECK_ARG(fast_class(S, N, vec) == 1 && e.C % 8 == 0, "gates gemm: bf16-stored activations need the bf16-operand vector path");
            return launch_split8<Epi8, false>(S, M, N, Epi8{{e}}, st);
        }
        if (fast_class(S, N, vec) == 1) return launch_fast<Epi, true, false>(S, M, N, Epi{{e}}, 0, st);
        REGT_CHECK_ARG(!e.q_bf16, "gates gemm: bf16 storage of q needs the vector path");
        return launch_flat(S, M, N, Epi{{e}}, vec, st);
    });
}

}  // namespace regt

#ifdef REGT_WG_TRACE
// developer build only (not part of include/regtgcn.h): copy the workgroup trace to the host
extern "C" int regt_wg_trace_read(long* host, long nblocks) {
    if (nblocks > regt::WG_TRACE_MAX) nblocks = regt::WG_TRACE_MAX;
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(regt::g_wg_trace), sizeof(long) * 4 * nblocks);
}
extern "C" int regt_wg_marks_read(long* host, long nblocks) {
    if (nblocks > regt::WG_TRACE_MAX) nblocks = regt::WG_TRACE_MAX;
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(regt::g_wg_marks), sizeof(long) * 8 * nblocks);
}
#endif
