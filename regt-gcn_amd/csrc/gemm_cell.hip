// The GRU cell's candidate stage and the data gradients of its backward pass: the GEMMs whose epilogues read the stored gates.
//   dgrad1 (candidate: drp and dh from dq), the same behind a generated left operand (gemm_dgrad1_gen_kernel: cell_bwd and the
//   candidate data gradient in one launch), dgrad2 (gates: ds in place on dh), the dropout mask + residual add of the head
//   candidate state H~ = tanh(q Uh2^T + (A_hat x) Gh^T + ch), the blend Z h + (1 - Z) H~ and the attention-weighted sum over the T
//   periods of a node, all in the epilogue of one GEMM:
//     gemm_cand_split_kernel<NP> / gemm_cand_split8_kernel   three-workgroup core (fp32 storage / bf16 storage)
//     gemm_cand_flat_kernel<Core> / gemm_cand_flat8_kernel   small tiles and the two-workgroup cores
//     gemm_cand_kernel                                       generic fallback, the T loop inside the workgroup
//   SAVE = false in all of them (forward-only calls, REGT_DIMS_FORWARD_ONLY): H~ is blended and summed but not stored -- only the
//   backward pass reads it; a.Ht is then NULL.
// One unit, not two: compiled in a unit of their own, without a gemm_flat_split_kernel / gemm_flat_split8_kernel instantiation next
// to them, the twelve candidate kernels on SplitCore come out with their instructions in another order (profiles/gemm_units_isa.txt).
#include "gemm_flat.h"

namespace regt {

// ---- dgrad1: v = dq[m, c] ------------------------------------------------------------------------------------------------
// drp / dh / dzp through the fixed instruction sequences cb_drp / cb_dh / cb_dzp of kernels.h: left to -ffp-contract, the two-launch
// kernel and the generated-operand kernel of the bf16x3 arithmetic contracted `v R + p d Z` differently -- last-bit differences between
// two paths that tests/test_gpu_ops.py compares bit for bit.  One statement per output and width; every form of every functor calls it.
__device__ __forceinline__ float4 dgrad1_drp(float4 v, float4 h, float4 R) {
#define F_(k) cb_drp(v.k, h.k, R.k)
    return REGT_V4(F_);
#undef F_
}
__device__ __forceinline__ float4 dgrad1_dh(float4 v, float4 R, float p, float4 d, float4 Z) {
#define F_(k) cb_dh(v.k, R.k, p, d.k, Z.k)
    return REGT_V4(F_);
#undef F_
}
__device__ __forceinline__ F8 dgrad1_drp(const F8& v, const F8& h, const F8& R) {
#define F_(k) cb_drp(v.k, h.k, R.k)
    return REGT_F8(F_);
#undef F_
}
__device__ __forceinline__ F8 dgrad1_dh(const F8& v, const F8& R, float p, const F8& d, const F8& Z) {
#define F_(k) cb_dh(v.k, R.k, p, d.k, Z.k)
    return REGT_F8(F_);
#undef F_
}
// The row -> (node, period) map needs an integer division: it is done once per tile row (vrow, 128 threads, kept in LDS)
// instead of once per row slot of every thread.
__device__ __forceinline__ EpiRowEnt dgrad1_row(const EpiDgrad1& e, long m) {
    const long node = m / e.T;
    return EpiRowEnt{(int)(node * e.C * 4), e.probs[(int)(m - node * e.T)]};
}

struct EpiDgrad1F {
    EpiDgrad1 e;
    __device__ __forceinline__ void operator()(long m, int c, float v) const {
        long node = m / e.T;
        int t = (int)(m - node * e.T);
        float hv = e.h[m * e.C + c];
        float Z = e.ZR[m * (2L * e.C) + c];
        float R = e.ZR[m * (2L * e.C) + e.C + c];
        e.dzr[m * (2L * e.C) + e.C + c] = cb_drp(v, hv, R);
        e.dh[m * e.C + c] = cb_dh(v, R, e.probs[t], e.dOH[node * e.C + c], Z);
    }
    static constexpr int ROUND_ROWS = 8;
    struct Aux { float4 h, Z, R, d; float p; };
    __device__ __forceinline__ Aux load(long m, int c) const {
        const long node = m / e.T;
        Aux a;
        a.p = e.probs[(int)(m - node * e.T)];
        a.h = ld4(e.h + m * e.C + c);
        a.Z = ld4(e.ZR + m * (2L * e.C) + c);
        a.R = ld4(e.ZR + m * (2L * e.C) + e.C + c);
        a.d = ld4(e.dOH + node * e.C + c);
        return a;
    }
    __device__ __forceinline__ void apply(long m, int c, float4 v, const Aux& a) const {
        if (e.dzr_bf16) st4_bf16(e.dzr, m * (2L * e.C) + e.C + c, dgrad1_drp(v, a.h, a.R));
        else st4(e.dzr + m * (2L * e.C) + e.C + c, dgrad1_drp(v, a.h, a.R));
        st4(e.dh + m * e.C + c, dgrad1_dh(v, a.R, a.p, a.d, a.Z));
    }
    // variants: bit 0 = dzr stored as bf16
    static constexpr int NVAR = 2;
    static constexpr bool HAS_ROWTAB = true;
    struct Col {};
    struct Tile { __amdgpu_buffer_rsrc_t h, zr, d, dzr, dh; int vc, vzr, sc, szr, vd, vdzr, sdzr, rstep; const EpiRowEnt* rt; };
    __device__ __forceinline__ int variant(int) const { return e.dzr_bf16 ? 1 : 0; }
    __device__ __forceinline__ EpiRowEnt vrow(long m) const { return dgrad1_row(e, m); }
    template <int V> __device__ __forceinline__ Col vcol(int) const { return Col{}; }
    template <int V> __device__ __forceinline__ Tile vtile(const EpiGeom& g) const {
        Tile t;
        t.h = buf_srd(e.h + g.m0 * e.C + g.n0);
        t.dh = buf_srd(e.dh + g.m0 * e.C + g.n0);
        t.zr = buf_srd(e.ZR + g.m0 * (2L * e.C) + g.n0);
        t.d = buf_srd(e.dOH + g.n0);
        const long o = g.m0 * (2L * e.C) + e.C + g.n0;
        t.dzr = buf_srd((V & 1) ? reinterpret_cast<const char*>(e.dzr) + 2 * o : reinterpret_cast<const char*>(e.dzr) + 4 * o);
        t.vc = (g.rr * e.C + g.c) * 4;
        t.sc = g.step * e.C * 4;
        t.vzr = 2 * t.vc - g.c * 4;
        t.szr = 2 * t.sc;
        t.vd = g.c * 4;
        t.vdzr = (V & 1) ? t.vzr >> 1 : t.vzr;
        t.sdzr = (V & 1) ? t.szr >> 1 : t.szr;
        t.rt = g.rowtab + g.rr;
        t.rstep = g.step;
        return t;
    }
    struct VAux { float4 h, Z, R, d; float p; };
    template <int V> __device__ __forceinline__ VAux vload(const Tile& t, int i) const {
        const EpiRowEnt re = t.rt[i * t.rstep];
        VAux a;
        a.p = re.p;
        a.h = buf_ld4(t.h, t.vc, i * t.sc);
        a.Z = buf_ld4(t.zr, t.vzr, i * t.szr);
        a.R = buf_ld4(t.zr, t.vzr, i * t.szr + e.C * 4);
        a.d = buf_ld4(t.d, t.vd + re.off, 0);
        return a;
    }
    template <int V> __device__ __forceinline__ void vapply(const Tile& t, int i, float4 v, const Col&, const VAux& a) const {
        if (V & 1) buf_st4_bf16(t.dzr, t.vdzr + i * t.sdzr, 0, dgrad1_drp(v, a.h, a.R));
        else buf_st4(t.dzr, t.vdzr + i * t.sdzr, 0, dgrad1_drp(v, a.h, a.R));
        buf_st4(t.dh, t.vc + i * t.sc, 0, dgrad1_dh(v, a.R, a.p, a.d, a.Z));
    }
};
// EpiDgrad1F behind a GENERATED left operand (SplitCore::run_u_gen): with H~ at hand as well, the epilogue also forms
// dzp = g (h - H~) Z (1 - Z) -> dzr[m, c] and the row's partial attention dot <dOH[node], Z h + (1 - Z) H~> over the tile's
// 128 columns (summed over a half wave: the 32 lanes that share a row) -> rowdot[m * parts + column tile]; cell_bwd_kernel's
// three outputs without its pass over Z, h, H~.  fp32 arrays only.
// (Its apply / vapply keep the three statements written out on cb_drp / cb_dh / cb_dzp: through dgrad1_drp / dgrad1_dh the compiler
// scheduled both gemm_dgrad1_gen_kernel instantiations differently -- profiles/gemm_units_isa.txt.)
struct EpiDgrad1GenF {
    EpiDgrad1 e;
    int parts;              // C / 128 column tiles
    static constexpr int ROUND_ROWS = 8;
    // sum over the 32 lanes of a half wave (the lanes that share a tile row), in a fixed order, on the VALU's DPP path -- no LDS
    // round trips: quads, 8-lane halves, 16-lane rows, then row 0's total into row 1 (row 2's into row 3).  The total ends up in
    // lanes 16-31 / 48-63; lane 31 / 63 stores it.
    __device__ __forceinline__ static float half_wave_sum(float s) {
#define REGT_DPP_ADD(ctrl, rmask) s += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, s), ctrl, rmask, 0xF, true))
        REGT_DPP_ADD(0xB1, 0xF);     // quad_perm [1, 0, 3, 2]
        REGT_DPP_ADD(0x4E, 0xF);     // quad_perm [2, 3, 0, 1]
        REGT_DPP_ADD(0x141, 0xF);    // row_half_mirror
        REGT_DPP_ADD(0x140, 0xF);    // row_mirror
        REGT_DPP_ADD(0x142, 0xA);    // row_bcast:15 into rows 1 and 3
#undef REGT_DPP_ADD
        return s;
    }
    static constexpr int SUM_LANE = 31;
    static constexpr int EPI_AUX_BYTES = 192;     // two rounds of two rows in flight (this kernel runs two workgroups per CU: 256 VGPRs)
    struct Aux { float4 h, Z, R, d, t; float p; };
    __device__ __forceinline__ Aux load(long m, int c) const {
        const long node = m / e.T;
        Aux a;
        a.p = e.probs[(int)(m - node * e.T)];
        a.h = ld4(e.h + m * e.C + c);
        a.Z = ld4(e.ZR + m * (2L * e.C) + c);
        a.R = ld4(e.ZR + m * (2L * e.C) + e.C + c);
        a.d = ld4(e.dOH + node * e.C + c);
        a.t = ld4(e.Ht + m * e.C + c);
        return a;
    }
#define REGT_GEN_DOT(a) ((a.d.x * (a.Z.x * a.h.x + (1.0f - a.Z.x) * a.t.x) + a.d.y * (a.Z.y * a.h.y + (1.0f - a.Z.y) * a.t.y)) + \
                         (a.d.z * (a.Z.z * a.h.z + (1.0f - a.Z.z) * a.t.z) + a.d.w * (a.Z.w * a.h.w + (1.0f - a.Z.w) * a.t.w)))
    __device__ __forceinline__ void apply(long m, int c, float4 v, const Aux& a) const {
#define F_(k) cb_drp(v.k, a.h.k, a.R.k)
        st4(e.dzr + m * (2L * e.C) + e.C + c, REGT_V4(F_));
#undef F_
#define F_(k) cb_dh(v.k, a.R.k, a.p, a.d.k, a.Z.k)
        st4(e.dh + m * e.C + c, REGT_V4(F_));
#undef F_
#define F_(k) cb_dzp(__fmul_rn(a.p, a.d.k), a.h.k, a.t.k, a.Z.k)
        st4(e.dzr + m * (2L * e.C) + c, REGT_V4(F_));
#undef F_
        // (guarded path of a partial tile: the 32 lanes of a row take this branch together -- rows are uniform per half wave)
        const float s = half_wave_sum(REGT_GEN_DOT(a));
        if ((threadIdx.x & 31) == SUM_LANE) e.rowdot[m * parts + c / GBN] = s;
    }
    static constexpr int NVAR = 1;
    static constexpr bool HAS_ROWTAB = true;
    struct Col {};
    struct Tile { __amdgpu_buffer_rsrc_t h, zr, d, dzr, dh, t, rd; int vc, vzr, sc, szr, vd, vrd, srd, rstep; const EpiRowEnt* rt; };
    __device__ __forceinline__ int variant(int) const { return 0; }
    __device__ __forceinline__ EpiRowEnt vrow(long m) const {
        const long node = m / e.T;
        return EpiRowEnt{(int)(node * e.C * 4), e.probs[(int)(m - node * e.T)]};
    }
    template <int V> __device__ __forceinline__ Col vcol(int) const { return Col{}; }
    template <int V> __device__ __forceinline__ Tile vtile(const EpiGeom& g) const {
        Tile t;
        t.h = buf_srd(e.h + g.m0 * e.C + g.n0);
        t.t = buf_srd(e.Ht + g.m0 * e.C + g.n0);
        t.dh = buf_srd(e.dh + g.m0 * e.C + g.n0);
        t.zr = buf_srd(e.ZR + g.m0 * (2L * e.C) + g.n0);
        t.d = buf_srd(e.dOH + g.n0);
        t.dzr = buf_srd(e.dzr + g.m0 * (2L * e.C) + g.n0);
        t.rd = buf_srd(e.rowdot + g.m0 * parts + g.n0 / GBN);
        t.vc = (g.rr * e.C + g.c) * 4;
        t.sc = g.step * e.C * 4;
        t.vzr = 2 * t.vc - g.c * 4;
        t.szr = 2 * t.sc;
        t.vd = g.c * 4;
        t.vrd = g.rr * parts * 4;
        t.srd = g.step * parts * 4;
        t.rt = g.rowtab + g.rr;
        t.rstep = g.step;
        return t;
    }
    struct VAux { float4 h, Z, R, d, t; float p; };
    template <int V> __device__ __forceinline__ VAux vload(const Tile& t, int i) const {
        const EpiRowEnt re = t.rt[i * t.rstep];
        VAux a;
        a.p = re.p;
        a.h = buf_ld4(t.h, t.vc, i * t.sc);
        a.Z = buf_ld4(t.zr, t.vzr, i * t.szr);
        a.R = buf_ld4(t.zr, t.vzr, i * t.szr + e.C * 4);
        a.d = buf_ld4(t.d, t.vd + re.off, 0);
        a.t = buf_ld4(t.t, t.vc, i * t.sc);
        return a;
    }
    template <int V> __device__ __forceinline__ void vapply(const Tile& t, int i, float4 v, const Col&, const VAux& a) const {
#define F_(k) cb_drp(v.k, a.h.k, a.R.k)
        buf_st4(t.dzr, t.vzr + i * t.szr + e.C * 4, 0, REGT_V4(F_));
#undef F_
#define F_(k) cb_dh(v.k, a.R.k, a.p, a.d.k, a.Z.k)
        buf_st4(t.dh, t.vc + i * t.sc, 0, REGT_V4(F_));
#undef F_
#define F_(k) cb_dzp(__fmul_rn(a.p, a.d.k), a.h.k, a.t.k, a.Z.k)
        buf_st4(t.dzr, t.vzr + i * t.szr, 0, REGT_V4(F_));
#undef F_
        const float s = half_wave_sum(REGT_GEN_DOT(a));
        if ((threadIdx.x & 31) == SUM_LANE) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(s), t.rd, t.vrd + i * t.srd, 0, 0);
    }
#undef REGT_GEN_DOT
};
struct EpiDgrad18F {
    typedef F8 Vec;
    EpiDgrad1 e;
    static constexpr int ROUND_ROWS = 1;      // 33 registers of auxiliary operands per row under the 168-VGPR cap
    struct ColAux {};
    struct Aux { F8 h, Z, R, d; float p; };
    __device__ __forceinline__ ColAux col(int) const { return ColAux{}; }
    __device__ __forceinline__ Aux load(long m, int c) const {
        const long node = m / e.T;
        Aux a;
        a.p = e.probs[(int)(m - node * e.T)];
        a.h = ld8(e.h, m * e.C + c, e.h_bf16);
        a.Z = ld8(e.ZR, m * (2L * e.C) + c, e.zr_bf16);
        a.R = ld8(e.ZR, m * (2L * e.C) + e.C + c, e.zr_bf16);
        a.d = ld8(e.dOH, node * e.C + c, 0);
        return a;
    }
    __device__ __forceinline__ void apply(long m, int c, const F8& v, const ColAux&, const Aux& a) const {
        st8(e.dzr, m * (2L * e.C) + e.C + c, dgrad1_drp(v, a.h, a.R), e.dzr_bf16);
        st8(e.dh, m * e.C + c, dgrad1_dh(v, a.R, a.p, a.d, a.Z), e.dh_bf16);
    }
    // straight-line variant (h, [Z|R], dzr, dh all stored as bf16); row -> (node, period) through the LDS row table
    static constexpr int NVAR = 1;
    static constexpr bool HAS_ROWTAB = true;
    typedef ColAux Col;
    struct VAux { u32x4_t h, Z, R; float4 d0, d1; float p; };
    struct Tile { __amdgpu_buffer_rsrc_t h, zr, d, dzr, dh; int vc, vzr, sc, szr, vd, rstep; const EpiRowEnt* rt; };
    __device__ __forceinline__ int variant(int) const { return (e.h_bf16 && e.zr_bf16 && e.dzr_bf16 && e.dh_bf16) ? 0 : -1; }
    __device__ __forceinline__ EpiRowEnt vrow(long m) const { return dgrad1_row(e, m); }
    template <int V> __device__ __forceinline__ Col vcol(int) const { return Col{}; }
    template <int V> __device__ __forceinline__ Tile vtile(const EpiGeom& g) const {
        Tile t;
        t.h = buf_srd(reinterpret_cast<const char*>(e.h) + 2 * (g.m0 * e.C + g.n0));
        t.dh = buf_srd(reinterpret_cast<const char*>(e.dh) + 2 * (g.m0 * e.C + g.n0));
        t.zr = buf_srd(reinterpret_cast<const char*>(e.ZR) + 2 * (g.m0 * (2L * e.C) + g.n0));
        t.dzr = buf_srd(reinterpret_cast<const char*>(e.dzr) + 2 * (g.m0 * (2L * e.C) + e.C + g.n0));
        t.d = buf_srd(e.dOH + g.n0);
        t.vc = (g.rr * e.C + g.c) * 2;
        t.sc = g.step * e.C * 2;
        t.vzr = (g.rr * 2 * e.C + g.c) * 2;
        t.szr = 2 * t.sc;
        t.vd = g.c * 4;
        t.rstep = g.step;
        t.rt = g.rowtab + g.rr;
        return t;
    }
    template <int V> __device__ __forceinline__ VAux vload(const Tile& t, int i) const {
        const EpiRowEnt re = t.rt[i * t.rstep];
        VAux a;
        a.p = re.p;
        a.h = buf_ld16(t.h, t.vc, i * t.sc);
        a.Z = buf_ld16(t.zr, t.vzr, i * t.szr);
        a.R = buf_ld16(t.zr, t.vzr, i * t.szr + e.C * 2);
        a.d0 = buf_ld4(t.d, t.vd + re.off, 0);
        a.d1 = buf_ld4(t.d, t.vd + re.off, 16);
        return a;
    }
    template <int V> __device__ __forceinline__ void vapply(const Tile& t, int i, const F8& v, const Col&, const VAux& a) const {
        const F8 h = widen8(a.h), Z = widen8(a.Z), R = widen8(a.R), d = F8{a.d0, a.d1};
        buf_st8_bf16(t.dzr, t.vzr + i * t.szr, dgrad1_drp(v, h, R));
        buf_st8_bf16(t.dh, t.vc + i * t.sc, dgrad1_dh(v, R, a.p, d, Z));
    }
};

// ---- dgrad2: ds = (dh + v) act'(h), in place on dh ---------------------------------------------------------------------
// act' as a factor: 1, or for the leaky relu 1 / slope by the sign of h.  The 4-column forms multiply plainly, the 8-column
// ones through cb_ds of kernels.h, as they always have.  (The forms stay written out: stated as one per-element function the
// compiler scheduled gemm_flat_fast_kernel<EpiDgrad2F, ..> and gemm_flat_split8_kernel<EpiDgrad28F, false> differently --
// profiles/gemm_units_isa.txt.)
struct EpiDgrad2F {
    EpiDgrad2 e;
    __device__ __forceinline__ void operator()(long m, int c, float v) const {
        long i = m * e.C + c;
        float d = e.dh[i] + v;
        if (e.act == ACT_LRELU) d = e.h[i] > 0.f ? d : d * e.slope;
        e.dh[i] = d;
    }
    static constexpr int ROUND_ROWS = 16;
    struct Aux { float4 d, h; };
    __device__ __forceinline__ Aux load(long m, int c) const {
        Aux a;
        a.d = ld4(e.dh + m * e.C + c);
        a.h = e.act == ACT_LRELU ? ld4(e.h + m * e.C + c) : make_float4(1, 1, 1, 1);
        return a;
    }
    __device__ __forceinline__ void apply(long m, int c, float4 v, const Aux& a) const {
#define F_(k) ((a.d.k + v.k) * (a.h.k > 0.f ? 1.0f : e.slope))
        st4(e.dh + m * e.C + c, REGT_V4(F_));
#undef F_
    }
    // variants: bit 0 = leaky-relu derivative (reads h)
    static constexpr int NVAR = 2;
    static constexpr bool HAS_ROWTAB = false;
    struct Col {};
    struct VAux { float4 d, h; };
    struct Tile { __amdgpu_buffer_rsrc_t dh, h; int v, s; };
    __device__ __forceinline__ int variant(int) const { return e.act == ACT_LRELU ? 1 : 0; }
    template <int V> __device__ __forceinline__ Col vcol(int) const { return Col{}; }
    template <int V> __device__ __forceinline__ Tile vtile(const EpiGeom& g) const {
        Tile t;
        t.dh = buf_srd(e.dh + g.m0 * e.C + g.n0);
        if (V & 1) t.h = buf_srd(e.h + g.m0 * e.C + g.n0);
        t.v = (g.rr * e.C + g.c) * 4;
        t.s = g.step * e.C * 4;
        return t;
    }
    template <int V> __device__ __forceinline__ VAux vload(const Tile& t, int i) const {
        VAux a;
        a.d = buf_ld4(t.dh, t.v, i * t.s);
        if (V & 1) a.h = buf_ld4(t.h, t.v, i * t.s);
        return a;
    }
    template <int V> __device__ __forceinline__ void vapply(const Tile& t, int i, float4 v, const Col&, const VAux& a) const {
#define F_(k) ((a.d.k + v.k) * ((V & 1) ? (a.h.k > 0.f ? 1.0f : e.slope) : 1.0f))
        buf_st4(t.dh, t.v + i * t.s, 0, REGT_V4(F_));
#undef F_
    }
};
struct EpiDgrad28F {
    typedef F8 Vec;
    EpiDgrad2 e;
    static constexpr int ROUND_ROWS = 4;
    struct ColAux {};
    struct Aux { F8 d, h; };
    __device__ __forceinline__ ColAux col(int) const { return ColAux{}; }
    __device__ __forceinline__ Aux load(long m, int c) const {
        Aux a;
        a.d = ld8(e.dh, m * e.C + c, e.dh_bf16);
        if (e.act == ACT_LRELU) a.h = ld8(e.h, m * e.C + c, e.h_bf16);
        else a.h = F8{make_float4(1, 1, 1, 1), make_float4(1, 1, 1, 1)};
        return a;
    }
    __device__ __forceinline__ void apply(long m, int c, const F8& v, const ColAux&, const Aux& a) const {
#define F_(k) cb_ds(a.d.k, v.k, a.h.k > 0.f ? 1.0f : e.slope)
        st8(e.dh, m * e.C + c, REGT_F8(F_), e.dh_bf16);
#undef F_
    }
    // straight-line variants (dh and h stored as bf16): bit 0 = leaky-relu derivative (reads h)
    static constexpr int NVAR = 2;
    static constexpr bool HAS_ROWTAB = false;
    typedef ColAux Col;
    struct VAux { u32x4_t d, h; };
    struct Tile { __amdgpu_buffer_rsrc_t dh, h; int v, s; };
    __device__ __forceinline__ int variant(int) const { return (e.dh_bf16 && e.h_bf16) ? (e.act == ACT_LRELU ? 1 : 0) : -1; }
    template <int V> __device__ __forceinline__ Col vcol(int) const { return Col{}; }
    template <int V> __device__ __forceinline__ Tile vtile(const EpiGeom& g) const {
        Tile t;
        t.dh = buf_srd(reinterpret_cast<const char*>(e.dh) + 2 * (g.m0 * e.C + g.n0));
        if (V & 1) t.h = buf_srd(reinterpret_cast<const char*>(e.h) + 2 * (g.m0 * e.C + g.n0));
        t.v = (g.rr * e.C + g.c) * 2;
        t.s = g.step * e.C * 2;
        return t;
    }
    template <int V> __device__ __forceinline__ VAux vload(const Tile& t, int i) const {
        VAux a;
        a.d = buf_ld16(t.dh, t.v, i * t.s);
        if (V & 1) a.h = buf_ld16(t.h, t.v, i * t.s);
        return a;
    }
    template <int V> __device__ __forceinline__ void vapply(const Tile& t, int i, const F8& v, const Col&, const VAux& a) const {
        const F8 d = widen8(a.d);
        F8 h = d;
        if (V & 1) h = widen8(a.h);
#define F_(k) cb_ds(d.k, v.k, (V & 1) ? (h.k > 0.f ? 1.0f : e.slope) : 1.0f)
        buf_st8_bf16(t.dh, t.v + i * t.s, REGT_F8(F_));
#undef F_
    }
};

// ---- out = v (mask > 0) + add ------------------------------------------------------------------------------------------
__device__ __forceinline__ float mask_add(float mk, float v, float ad) { return (mk > 0.f ? v : 0.f) + ad; }

struct EpiMaskAddF {
    EpiMaskAdd e;
    __device__ __forceinline__ void operator()(long m, int c, float v) const {
        float o = e.mask[m * e.ldm + c] > 0.f ? v : 0.f;
        if (e.add) o += e.add[m * e.ldadd + c];
        e.out[m * e.ldo + c] = o;
    }
    static constexpr int ROUND_ROWS = 16;
    struct Aux { float4 mk, ad; };
    __device__ __forceinline__ Aux load(long m, int c) const {
        Aux a;
        a.mk = ld4(e.mask + m * e.ldm + c);
        a.ad = e.add ? ld4(e.add + m * e.ldadd + c) : make_float4(0, 0, 0, 0);
        return a;
    }
    __device__ __forceinline__ void apply(long m, int c, float4 v, const Aux& a) const {
#define F_(k) mask_add(a.mk.k, v.k, a.ad.k)
        st4(e.out + m * e.ldo + c, REGT_V4(F_));
#undef F_
    }
    // variants: bit 0 = an addend is given
    static constexpr int NVAR = 2;
    static constexpr bool HAS_ROWTAB = false;
    struct Col {};
    struct VAux { float4 mk, ad; };
    struct Tile { __amdgpu_buffer_rsrc_t out, mask, add; int vo, vm, va, so, sm, sa; };
    __device__ __forceinline__ int variant(int) const {
        return (e.ldo >= (1L << 22) || e.ldm >= (1L << 22) || (e.add && e.ldadd >= (1L << 22))) ? -1 : (e.add ? 1 : 0);    // 32-bit tile offsets
    }
    template <int V> __device__ __forceinline__ Col vcol(int) const { return Col{}; }
    template <int V> __device__ __forceinline__ Tile vtile(const EpiGeom& g) const {
        Tile t;
        t.out = buf_srd(e.out + g.m0 * e.ldo + g.n0);
        t.mask = buf_srd(e.mask + g.m0 * e.ldm + g.n0);
        if (V & 1) t.add = buf_srd(e.add + g.m0 * e.ldadd + g.n0);
        t.vo = (g.rr * (int)e.ldo + g.c) * 4; t.so = g.step * (int)e.ldo * 4;
        t.vm = (g.rr * (int)e.ldm + g.c) * 4; t.sm = g.step * (int)e.ldm * 4;
        t.va = (g.rr * (int)e.ldadd + g.c) * 4; t.sa = g.step * (int)e.ldadd * 4;
        return t;
    }
    template <int V> __device__ __forceinline__ VAux vload(const Tile& t, int i) const {
        VAux a;
        a.mk = buf_ld4(t.mask, t.vm, i * t.sm);
        a.ad = (V & 1) ? buf_ld4(t.add, t.va, i * t.sa) : make_float4(0, 0, 0, 0);
        return a;
    }
    template <int V> __device__ __forceinline__ void vapply(const Tile& t, int i, float4 v, const Col&, const VAux& a) const {
#define F_(k) mask_add(a.mk.k, v.k, a.ad.k)
        buf_st4(t.out, t.vo + i * t.so, 0, REGT_V4(F_));
#undef F_
    }
};

// dgrad_candidate with its left operand generated on the way (SplitCore::run_u_gen + EpiDgrad1GenF): cell_bwd_kernel and the candidate
// data gradient in one launch.  fp32 arithmetic; two workgroups per CU (three operand arrays in flight per A slot).
template <int NP>     // 0: fp32 MFMA; 3: exact bf16x3 split (REGT_GEMM_MODE=bf16x3) -- fp32 storage either way
__global__ __launch_bounds__(256, 2) void gemm_dgrad1_gen_kernel(GemmSegs S, long M, int N, EpiDgrad1GenF epi) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tiles_n = (N + GBN - 1) / GBN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const long m0 = (long)(bid / tiles_n) * GBM;
    const int n0 = (bid % tiles_n) * GBN;
    RowMap rm{m0, 1, (int)((M - m0) < GBM ? (M - m0) : GBM)};
    SplitCore<false, NP> core(S, rm, n0, N, lds, true);
    core.fill_rowtab(epi);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const typename SplitCore<false, NP>::AGen g{epi.e.ZR, epi.e.Ht, epi.e.dOH, epi.e.dhp, epi.e.C, (unsigned)epi.e.num_nodes * (unsigned)epi.e.C * 4u};
    core.run_u_gen(acc, g);
    core.for_each_vec_halves(acc, epi);
}

int launch_gemm_dgrad1(const GemmSegs& S, long M, int N, const EpiDgrad1& e, hipStream_t st) {
    REGT_CHECK_ARG(N == e.C, "dgrad1 gemm expects N == C");
    const bool vec = e.C % 4 == 0 && a16(e.h) && a16(e.ZR) && a16(e.dOH) && a16(e.dzr) && a16(e.dh);
    if (e.h_bf16 || e.zr_bf16 || e.dh_bf16) {
        REGT_CHECK_ARG(fast_class(S, N, vec) == 1 && e.C % 8 == 0, "dgrad1 gemm: bf16-stored activations need the bf16-operand vector path");
        return launch_split8<EpiDgrad18F, false>(S, M, N, EpiDgrad18F{e}, st);
    }
    if (fast_class(S, N, vec) == 1) return launch_fast<EpiDgrad1F, true, false>(S, M, N, EpiDgrad1F{e}, 0, st);
    REGT_CHECK_ARG(!e.dzr_bf16, "dgrad1 gemm: bf16 storage of dzr needs the bf16-operand vector path");
    if (fast_class(S, N, vec) == 0) return launch_fast<EpiDgrad1F, false, false>(S, M, N, EpiDgrad1F{e}, 0, st);
    return launch_flat(S, M, N, EpiDgrad1F{e}, vec, st);
}
int launch_gemm_dgrad1_gen(const GemmSegs& S, long M, int N, const EpiDgrad1& e, hipStream_t st) {
    REGT_CHECK_ARG(N == e.C && S.nseg == 1 && S.seg[0].K == e.C && (S.seg[0].flags & SEG_BT) && (S.seg[0].flags & SEG_VEC_B) &&
                   !(S.seg[0].flags & (SEG_A_BF16 | SEG_B_FRAG | SEG_REGION | SEG_REPEAT)), "dgrad1 (generated operand): one [N][K] weight segment with K = C");
    REGT_CHECK_ARG(gemm_dgrad1_gen_ok(M, e.C, e.num_nodes), "dgrad1 (generated operand): shape / arithmetic not covered");
    REGT_CHECK_ARG(e.Ht && e.dhp && e.rowdot && !e.dzr_bf16 && !e.h_bf16 && !e.zr_bf16 && !e.dh_bf16, "dgrad1 (generated operand): fp32 arrays, all outputs given");
    REGT_CHECK_ARG(a16(e.h) && a16(e.ZR) && a16(e.dOH) && a16(e.dzr) && a16(e.dh) && a16(e.Ht) && a16(e.dhp), "dgrad1 (generated operand): 16-byte aligned arrays");
    long tiles;
    if (int rc = gemm_tiles(M, N, GBM, GBN, &tiles)) return rc;      // (N is a multiple of the tile width: gemm_dgrad1_gen_ok)
    if (gemm_mode() == 1)
        hipLaunchKernelGGL(gemm_dgrad1_gen_kernel<3>, dim3((unsigned)tiles), dim3(256), SplitGeom<3>::LDS_BYTES, st, S, M, N, EpiDgrad1GenF{e, e.C / GBN});
    else
        hipLaunchKernelGGL(gemm_dgrad1_gen_kernel<0>, dim3((unsigned)tiles), dim3(256), SplitGeom<0>::LDS_BYTES, st, S, M, N, EpiDgrad1GenF{e, e.C / GBN});
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}
int launch_gemm_dgrad2(const GemmSegs& S, long M, int N, const EpiDgrad2& e, hipStream_t st) {
    REGT_CHECK_ARG(N == e.C, "dgrad2 gemm expects N == C");
    const bool vec = e.C % 4 == 0 && a16(e.dh) && a16(e.h);
    if (e.h_bf16 || e.dh_bf16) {
        REGT_CHECK_ARG(fast_class(S, N, vec) == 1 && e.C % 8 == 0, "dgrad2 gemm: bf16-stored activations need the bf16-operand vector path");
        return launch_split8<EpiDgrad28F, false>(S, M, N, EpiDgrad28F{e}, st);
    }
    if (fast_class(S, N, vec) == 1) return launch_fast<EpiDgrad2F, true, false>(S, M, N, EpiDgrad2F{e}, 0, st);
    if (fast_class(S, N, vec) == 0) return launch_fast<EpiDgrad2F, false, false>(S, M, N, EpiDgrad2F{e}, 0, st);
    return launch_flat(S, M, N, EpiDgrad2F{e}, vec, st);
}
int launch_gemm_mask_add(const GemmSegs& S, long M, int N, const EpiMaskAdd& e, hipStream_t st) {
    const bool vec = N % 4 == 0 && e.ldo % 4 == 0 && e.ldm % 4 == 0 && (!e.add || e.ldadd % 4 == 0) && a16(e.out) &&
                     a16(e.mask) && a16(e.add);
    if (fast_class(S, N, vec) == 0) return launch_fast<EpiMaskAddF, false, false>(S, M, N, EpiMaskAddF{e}, 0, st);
    return launch_flat(S, M, N, EpiMaskAddF{e}, vec, st);
}

// ==== candidate state ================================================================================================

// ---- candidate state, T loop inside the workgroup ------------------------------------------------
// Per period t: Ht = tanh(q_t Uh2^T + (A_hat x)_t Gh^T + ch) is stored for the backward pass, blended
// with the gate (Z*h + (1-Z)*Ht) and accumulated with the attention probability p_t in registers;
// the hidden state (N, C) is written once after the last period.
// Generic (scalar-epilogue) fallback of the candidate stage: one workgroup walks the T periods of a node tile.
template <bool SAVE>
__global__ __launch_bounds__(256, 1) void gemm_cand_kernel(CandArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tiles_n = (a.C + GBN - 1) / GBN;
    const long C = a.C;
    f32x16 acc[2][2];
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int i0 = (bid / tiles_n) * GBM;
    const int n0 = (bid % tiles_n) * GBN;
    const int nvalid = (a.num_nodes - i0) < GBM ? (a.num_nodes - i0) : GBM;
    f32x16 oh[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) oh[i][j][r] = 0.f;
    for (int t = 0; t < a.T; ++t) {
        RowMap rm{(long)i0 * a.T + t, a.T, nvalid};
        GemmCore core(a.S, rm, n0, a.C, lds);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        core.run(acc);
        const float pt = a.probs[t];
        core.for_each2(acc, oh, [&](int r, int c, float v, float o) {
            long m = rm.grow(r);
            float ht = fast_tanh(v + a.bias[c]);
            if (SAVE) a.Ht[m * C + c] = ht;
            float Z = a.ZR[m * 2 * C + c];
            float hv = a.h[m * C + c];
            return o + pt * (Z * hv + (1.0f - Z) * ht);
        });
    }
    RowMap rm{(long)i0, 1, nvalid};
    GemmCore core(a.S, rm, n0, a.C, lds);
    core.for_each(oh, [&](int r, int c, float v) { a.OH[(long)(i0 + r) * C + c] = v; });
}

// Vector path of the candidate stage: a FLAT GEMM over the (node*T + t) rows, same geometry and
// efficiency as the gate GEMM.  Rows of one node are adjacent, so the attention-weighted sum over the
// T periods is a segmented reduction inside the 128-row tile, done in LDS after the blend; a node
// that straddles two tiles (T <= 64 < 128, so never more than two) gets one partial sum from each,
// added atomically into the zero-initialised hidden state -- two addends commute, so the result is
// bit-reproducible.
template <class Core, bool SAVE>
__global__ __launch_bounds__(256, 2) void gemm_cand_flat_kernel(CandArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int BM = Core::BM, BN = Core::BN, KROW = Core::EKROW, TPR = Core::ETPR;
    const long C = a.C, M = (long)a.num_nodes * a.T;
    const int tiles_n = (a.C + BN - 1) / BN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const long m0 = (long)(bid / tiles_n) * BM;
    const int n0 = (bid % tiles_n) * BN;
    const RowMap rm{m0, 1, (int)((M - m0) < BM ? (M - m0) : BM)};
    Core core(a.S, rm, n0, a.C, lds);
    core.plan();
    typename Core::Acc acc;
    Core::zero(acc);
    core.run(acc, false);
    const int c = core.ecol();
    const int node0 = (int)(m0 / a.T);
    // epilogue rows in rounds of RR; the first round's Z / h rows are requested before the accumulators are staged through
    // LDS (their HBM latency overlaps the staging), see FastCore::for_each_vec
    constexpr int RR = Core::EROWS >= 8 ? 8 : Core::EROWS;
    float4 Z[RR], hv[RR];
    if (c < a.C) {
#pragma unroll
        for (int j = 0; j < RR; ++j) {
            const int r = core.erow(j);
            if (r < rm.nvalid) {
                Z[j] = ld4(a.ZR + (m0 + r) * 2 * C + c);
                hv[j] = ld4(a.h + (m0 + r) * C + c);
            }
        }
    }
    core.stage(acc);
    if (c < a.C) {
        const float4 b = ld4(a.bias + c);
#pragma unroll
        for (int g = 0; g < Core::EROWS / RR; ++g) {
            if (g > 0) {
#pragma unroll
                for (int j = 0; j < RR; ++j) {
                    const int r = core.erow(RR * g + j);
                    if (r < rm.nvalid) {
                        Z[j] = ld4(a.ZR + (m0 + r) * 2 * C + c);
                        hv[j] = ld4(a.h + (m0 + r) * C + c);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < RR; ++j) {
                const int r = core.erow(RR * g + j);
                if (r < rm.nvalid) {
                    const long m = m0 + r;
                    const float pt = a.probs[(int)(m % a.T)];
                    const float4 v = core.eread(RR * g + j);
#define F_(k) fast_tanh(v.k + b.k)
                    const float4 ht = REGT_V4(F_);
#undef F_
                    if (SAVE) st4(a.Ht + m * C + c, ht);
                    float4 o;
                    o.x = pt * (Z[j].x * hv[j].x + (1.0f - Z[j].x) * ht.x);
                    o.y = pt * (Z[j].y * hv[j].y + (1.0f - Z[j].y) * ht.y);
                    o.z = pt * (Z[j].z * hv[j].z + (1.0f - Z[j].z) * ht.z);
                    o.w = pt * (Z[j].w * hv[j].w + (1.0f - Z[j].w) * ht.w);
                    *reinterpret_cast<float4*>(lds + r * KROW + 4 * (threadIdx.x & (TPR - 1))) = o;   // own element
                }
            }
        }
    }
    __syncthreads();
    // segmented sum over each node's rows inside the tile
    const int node1 = (int)((m0 + rm.nvalid - 1) / a.T);
    const int items = (node1 - node0 + 1) * TPR;
    for (int it = threadIdx.x; it < items; it += 256) {
        const int node = node0 + it / TPR, c4 = it % TPR;
        const int cc = n0 + 4 * c4;
        if (cc >= a.C) continue;
        long lo = (long)node * a.T - m0, hi = lo + a.T - 1;
        // all T rows of the node inside this tile: nobody else adds to its row of the zero-initialised hidden state -- one
        // 16-byte store instead of four atomics (which remain for the tile's first / last, partial nodes)
        const bool whole = lo >= 0 && hi <= rm.nvalid - 1;
        if (lo < 0) lo = 0;
        if (hi > rm.nvalid - 1) hi = rm.nvalid - 1;
        float4 s4 = make_float4(0, 0, 0, 0);
        for (long r = lo; r <= hi; ++r) {
            const float4 v = *reinterpret_cast<const float4*>(lds + r * KROW + 4 * c4);
            s4.x += v.x; s4.y += v.y; s4.z += v.z; s4.w += v.w;
        }
        float* o = a.OH + (long)node * C + cc;
        if (whole) *reinterpret_cast<float4*>(o) = s4;
        else { atomicAdd(o + 0, s4.x); atomicAdd(o + 1, s4.y); atomicAdd(o + 2, s4.z); atomicAdd(o + 3, s4.w); }
    }
}

// The same with ZR, h and Ht stored as bf16 (bf16-operand core, REGT_GEMM_MODE=bf16): 8 columns per thread, so that the
// epilogue's reads of Z and h and its store of H~ are 16-byte accesses.
template <bool SAVE>
__global__ __launch_bounds__(256, 2) void gemm_cand_flat8_kernel(CandArgs a) {
    using Core = SplitCore<false, 1>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int BM = Core::BM, BN = Core::BN, KROW = Core::EKROW, TPR = Core::ETPR;
    const long C = a.C, M = (long)a.num_nodes * a.T;
    const int tiles_n = (a.C + BN - 1) / BN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const long m0 = (long)(bid / tiles_n) * BM;
    const int n0 = (bid % tiles_n) * BN;
    const RowMap rm{m0, 1, (int)((M - m0) < BM ? (M - m0) : BM)};
    Core core(a.S, rm, n0, a.C, lds);
    core.plan();
    typename Core::Acc acc;
    Core::zero(acc);
    core.run(acc, false);
    const int tid = threadIdx.x;
    const int c = n0 + 8 * (tid & 15);
    const int node0 = (int)(m0 / a.T);
    constexpr int RR = 4;                          // rows per round of the thread's 8 rows (tid >> 4) + 16 i
    F8 Z[RR], hv[RR];
    if (c < a.C) {
#pragma unroll
        for (int j = 0; j < RR; ++j) {
            const int r = (tid >> 4) + 16 * j;
            if (r < rm.nvalid) {
                Z[j] = ld8(a.ZR, (m0 + r) * 2 * C + c, 1);
                hv[j] = ld8(a.h, (m0 + r) * C + c, 1);
            }
        }
    }
    core.stage(acc);
    if (c < a.C) {
        const F8 b = ld8(a.bias, c, 0);
#pragma unroll
        for (int g = 0; g < 8 / RR; ++g) {
            if (g > 0) {
#pragma unroll
                for (int j = 0; j < RR; ++j) {
                    const int r = (tid >> 4) + 16 * (RR * g + j);
                    if (r < rm.nvalid) {
                        Z[j] = ld8(a.ZR, (m0 + r) * 2 * C + c, 1);
                        hv[j] = ld8(a.h, (m0 + r) * C + c, 1);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < RR; ++j) {
                const int r = (tid >> 4) + 16 * (RR * g + j);
                if (r < rm.nvalid) {
                    const long m = m0 + r;
                    const float pt = a.probs[(int)(m % a.T)];
                    float4* img = reinterpret_cast<float4*>(lds + r * KROW + 8 * (tid & 15));
                    const F8 v{img[0], img[1]};
#define F_(k) fast_tanh(v.k + b.k)
                    const F8 ht = REGT_F8(F_);
#undef F_
                    if (SAVE) st8(a.Ht, m * C + c, ht, 1);
#define F_(k) (pt * (Z[j].k * hv[j].k + (1.0f - Z[j].k) * ht.k))
                    const F8 o = REGT_F8(F_);
#undef F_
                    img[0] = o.lo;                 // own elements of the staged tile
                    img[1] = o.hi;
                }
            }
        }
    }
    __syncthreads();
    // segmented sum over each node's rows inside the tile (as gemm_cand_flat_kernel)
    const int node1 = (int)((m0 + rm.nvalid - 1) / a.T);
    const int items = (node1 - node0 + 1) * TPR;
    for (int it = threadIdx.x; it < items; it += 256) {
        const int node = node0 + it / TPR, c4 = it % TPR;
        const int cc = n0 + 4 * c4;
        if (cc >= a.C) continue;
        long lo = (long)node * a.T - m0, hi = lo + a.T - 1;
        // all T rows of the node inside this tile: nobody else adds to its row of the zero-initialised hidden state -- one
        // 16-byte store instead of four atomics (which remain for the tile's first / last, partial nodes)
        const bool whole = lo >= 0 && hi <= rm.nvalid - 1;
        if (lo < 0) lo = 0;
        if (hi > rm.nvalid - 1) hi = rm.nvalid - 1;
        float4 s4 = make_float4(0, 0, 0, 0);
        for (long r = lo; r <= hi; ++r) {
            const float4 v = *reinterpret_cast<const float4*>(lds + r * KROW + 4 * c4);
            s4.x += v.x; s4.y += v.y; s4.z += v.z; s4.w += v.w;
        }
        float* o = a.OH + (long)node * C + cc;
        if (whole) *reinterpret_cast<float4*>(o) = s4;
        else { atomicAdd(o + 0, s4.x); atomicAdd(o + 1, s4.y); atomicAdd(o + 2, s4.z); atomicAdd(o + 3, s4.w); }
    }
}

// Candidate stage on the three-workgroup core (fp32 planes NP = 0, bf16x3 NP = 3), fp32 storage.  Per 64-row half of the
// tile: H~ = tanh(acc + ch) is stored, blended (p_t (Z h + (1 - Z) H~)) back into the half's LDS image, and the rows of
// every node that intersects the half are summed and added to OH with one atomic per element -- a node of T <= 64 rows
// meets at most two halves (tile boundaries are half boundaries), so every OH element is 0 + a + b: order-independent.
// The row -> (node, period) map costs one integer division per tile ROW (row table in LDS, written before the K loop),
// not one 64-bit modulo per row slot of every thread; arrays are addressed through buffer descriptors (one per array
// and tile); a full tile runs without a single branch (see the functor notes at the top of gemm_epilogue.h).
struct CandRowEnt { int nt; float p; };        // nt = (node - first node of the tile) << 8 | period
template <int NP, bool FULL, bool SAVE>
__device__ __forceinline__ void cand_epilogue(const CandArgs& a, const SplitCore<false, NP>& core, f32x16 (&acc)[2][2], float* lds,
                                              const CandRowEnt* rowtab, long m0, int n0, int nvalid, int node0, int t0) {
    const int tid = threadIdx.x, rr = tid >> 5, c4 = 4 * (tid & 31);
    const int C = a.C;
    const bool col_ok = FULL || n0 + c4 < C;
    const __amdgpu_buffer_rsrc_t szr = buf_srd(a.ZR + m0 * (2L * C) + n0), sh = buf_srd(a.h + m0 * C + n0);
    __amdgpu_buffer_rsrc_t sht;
    if (SAVE) sht = buf_srd(a.Ht + m0 * C + n0);
    const int vc = (rr * C + c4) * 4, vzr = (rr * 2 * C + c4) * 4, sc = 8 * C * 4, szs = 2 * sc;
    const float4 b = col_ok ? ld4(a.bias + n0 + c4) : make_float4(0, 0, 0, 0);
    constexpr int RR = 4, NR = 16 / RR;
    float4 Z[2][RR], hv[2][RR];
    auto request = [&](int k, float4 (&Zd)[RR], float4 (&hd)[RR]) {
#pragma unroll
        for (int j = 0; j < RR; ++j) {
            const int i = RR * k + j;
            if (FULL || (rr + 8 * i < nvalid && col_ok)) {
                Zd[j] = buf_ld4(szr, vzr, i * szs);
                hd[j] = buf_ld4(sh, vc, i * sc);
            }
        }
    };
    request(0, Z[0], hv[0]);
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int half = k / (NR / 2);
        if (k % (NR / 2) == 0) core.stage_half(half, acc);
        if (k + 1 < NR) request(k + 1, Z[(k + 1) & 1], hv[(k + 1) & 1]);
#pragma unroll
        for (int j = 0; j < RR; ++j) {
            const int i = RR * k + j, rl = rr + 8 * (i & 7);          // row rr + 8 i of the tile = row rl of its half
            if (FULL || (rr + 8 * i < nvalid && col_ok)) {
                float* img = lds + rl * G_LDS_KROW + c4;
                const float4 v = *reinterpret_cast<const float4*>(img);
                const float pt = rowtab[rr + 8 * i].p;
#define F_(q) fast_tanh(v.q + b.q)
                const float4 ht = REGT_V4(F_);
#undef F_
                // (forward-only: the value is pinned where the store stood -- an empty asm statement, no instruction; with H~ simply
                // not stored hipcc rescheduled the rounds of the fp32 kernel into 12 spilled registers under its 168-register cap)
                if (SAVE) buf_st4(sht, vc + i * sc, 0, ht);
                else { const u32x4_t w_ = {__float_as_uint(ht.x), __float_as_uint(ht.y), __float_as_uint(ht.z), __float_as_uint(ht.w)}; asm volatile("" :: "v"(w_), "v"(vc + i * sc)); }
                const float4 Zv = Z[k & 1][j], hh = hv[k & 1][j];
#define F_(q) __fmul_rn(pt, gru_blend(Zv.q, hh.q, ht.q))
                *reinterpret_cast<float4*>(img) = REGT_V4(F_);
#undef F_
            }
        }
        if (k % (NR / 2) == NR / 2 - 1) {
            // the half is blended: segmented sums over the nodes that intersect it
            __syncthreads();
            const int r_lo = 64 * half, r_hi = (FULL ? 64 * half + 63 : (nvalid - 1 < 64 * half + 63 ? nvalid - 1 : 64 * half + 63));
            if (FULL || r_hi >= r_lo) {
                const int n_first = rowtab[r_lo].nt >> 8, n_last = rowtab[r_hi].nt >> 8;
                for (int nd = n_first + rr; nd <= n_last; nd += 8) {
                    int lo = nd * a.T - t0, hi = lo + a.T - 1;               // the node's rows in tile coordinates
                    const bool whole = lo >= r_lo && hi <= r_hi;             // all of the node's rows in this half: plain store
                    lo = lo < r_lo ? r_lo : lo;
                    hi = hi > r_hi ? r_hi : hi;
                    float4 s4 = make_float4(0, 0, 0, 0);
                    for (int r = lo; r <= hi; ++r) {
                        const float4 v = *reinterpret_cast<const float4*>(lds + (r - r_lo) * G_LDS_KROW + c4);
                        s4.x += v.x; s4.y += v.y; s4.z += v.z; s4.w += v.w;
                    }
                    if (col_ok) {
                        float* o = a.OH + (long)(node0 + nd) * C + n0 + c4;
                        if (whole) *reinterpret_cast<float4*>(o) = s4;
                        else { atomicAdd(o + 0, s4.x); atomicAdd(o + 1, s4.y); atomicAdd(o + 2, s4.z); atomicAdd(o + 3, s4.w); }
                    }
                }
            }
        }
    }
}
template <int NP, bool SAVE>
__global__ __launch_bounds__(256, 3) void gemm_cand_split_kernel(CandArgs a, int uniform) {
    using Core = SplitCore<false, NP>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const long M = (long)a.num_nodes * a.T;
    const int tiles_n = (a.C + GBN - 1) / GBN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const long m0 = (long)(bid / tiles_n) * GBM;
    const int n0 = (bid % tiles_n) * GBN;
    const RowMap rm{m0, 1, (int)((M - m0) < GBM ? (M - m0) : GBM)};
    Core core(a.S, rm, n0, a.C, lds, true);
    CandRowEnt* rowtab = reinterpret_cast<CandRowEnt*>(core.rowtab());
    // first node / period of the tile: ONE 32-bit division per thread (M < 2^31, host-checked); row r then needs a small
    // quotient only ((t0 + r) / T by float reciprocal, exact below 2^16: the +0.5 keeps it off the integer boundaries)
    const int node0 = (int)((unsigned)m0 / (unsigned)a.T), t0 = (int)m0 - node0 * a.T;
    if (threadIdx.x < GBM) {
        const int x = t0 + (threadIdx.x < rm.nvalid ? threadIdx.x : 0), q = (int)(((float)x + 0.5f) * (1.0f / (float)a.T));
        rowtab[threadIdx.x] = CandRowEnt{(q << 8) | (x - q * a.T), a.probs[x - q * a.T]};
    }
    if (!uniform) core.plan();
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    if (uniform) core.run_uniform(acc, false);
    else core.run(acc, false);
    if (rm.nvalid == GBM && n0 + GBN <= a.C) cand_epilogue<NP, true, SAVE>(a, core, acc, lds, rowtab, m0, n0, GBM, node0, t0);
    else cand_epilogue<NP, false, SAVE>(a, core, acc, lds, rowtab, m0, n0, rm.nvalid, node0, t0);
}

// The same with Z, h and H~ stored as bf16 (REGT_GEMM_MODE=bf16, bf16-operand core NP = 1): 8 columns per thread (16-byte
// accesses of the bf16 arrays), row slots i = 0 .. 7: row (tid >> 4) + 16 i.
template <bool FULL, bool SAVE>
__device__ __forceinline__ void cand8_epilogue(const CandArgs& a, const SplitCore<false, 1>& core, f32x16 (&acc)[2][2], float* lds,
                                               const CandRowEnt* rowtab, long m0, int n0, int nvalid, int node0, int t0) {
    const int tid = threadIdx.x, rr = tid >> 4, c8 = 8 * (tid & 15);
    const int C = a.C;
    const bool col_ok = FULL || n0 + c8 < C;
    const __amdgpu_buffer_rsrc_t szr = buf_srd(reinterpret_cast<const char*>(a.ZR) + 2 * (m0 * (2L * C) + n0)),
                                 sh = buf_srd(reinterpret_cast<const char*>(a.h) + 2 * (m0 * C + n0));
    __amdgpu_buffer_rsrc_t sht;
    if (SAVE) sht = buf_srd(reinterpret_cast<const char*>(a.Ht) + 2 * (m0 * C + n0));
    const int vc = (rr * C + c8) * 2, vzr = (rr * 2 * C + c8) * 2, sc = 16 * C * 2, szs = 2 * sc;
    F8 b{make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0)};
    if (col_ok) b = ld8(a.bias, n0 + c8, 0);
    constexpr int RR = 2, NR = 8 / RR;
    u32x4_t Z[2][RR], hv[2][RR];
    auto request = [&](int k, u32x4_t (&Zd)[RR], u32x4_t (&hd)[RR]) {
#pragma unroll
        for (int j = 0; j < RR; ++j) {
            const int i = RR * k + j;
            if (FULL || (rr + 16 * i < nvalid && col_ok)) {
                Zd[j] = buf_ld16(szr, vzr, i * szs);
                hd[j] = buf_ld16(sh, vc, i * sc);
            }
        }
    };
    request(0, Z[0], hv[0]);
#pragma unroll
    for (int k = 0; k < NR; ++k) {
        const int half = k / (NR / 2);
        if (k % (NR / 2) == 0) core.stage_half(half, acc);
        if (k + 1 < NR) request(k + 1, Z[(k + 1) & 1], hv[(k + 1) & 1]);
#pragma unroll
        for (int j = 0; j < RR; ++j) {
            const int i = RR * k + j, rl = rr + 16 * (i & 3);
            if (FULL || (rr + 16 * i < nvalid && col_ok)) {
                float4* img = reinterpret_cast<float4*>(lds + rl * G_LDS_KROW + c8);
                const F8 v{img[0], img[1]};
                const float pt = rowtab[rr + 16 * i].p;
#define F_(q) fast_tanh(v.q + b.q)
                const F8 ht = REGT_F8(F_);
#undef F_
                if (SAVE) buf_st8_bf16(sht, vc + i * sc, ht);
                const F8 Zv = widen8(Z[k & 1][j]), hh = widen8(hv[k & 1][j]);
#define F_(q) __fmul_rn(pt, gru_blend(Zv.q, hh.q, ht.q))
                const F8 o = REGT_F8(F_);
#undef F_
                img[0] = o.lo;
                img[1] = o.hi;
            }
        }
        if (k % (NR / 2) == NR / 2 - 1) {
            __syncthreads();
            // the half is blended: per block of `node_sum_rows` rows (the whole half, or the 16 rows a wave of the row-owning fused
            // kernel holds) the rows of every node that meets the block are summed in row order
            const int brows = a.node_sum_rows == 16 ? 16 : 64;
            for (int r_lo = 64 * half; r_lo < 64 * half + 64; r_lo += brows) {
            const int r_end = r_lo + brows - 1, r_hi = FULL ? r_end : (nvalid - 1 < r_end ? nvalid - 1 : r_end);
            if (FULL || r_hi >= r_lo) {
                const int n_first = rowtab[r_lo].nt >> 8, n_last = rowtab[r_hi].nt >> 8;
                for (int nd = n_first + rr; nd <= n_last; nd += 16) {
                    int lo = nd * a.T - t0, hi = lo + a.T - 1;
                    const bool whole = lo >= r_lo && hi <= r_hi;
                    lo = lo < r_lo ? r_lo : lo;
                    hi = hi > r_hi ? r_hi : hi;
                    float4 s0 = make_float4(0, 0, 0, 0), s1 = s0;
                    for (int r = lo; r <= hi; ++r) {
                        const float4* p = reinterpret_cast<const float4*>(lds + (r - 64 * half) * G_LDS_KROW + c8);
                        const float4 u = p[0], w = p[1];
                        s0.x += u.x; s0.y += u.y; s0.z += u.z; s0.w += u.w;
                        s1.x += w.x; s1.y += w.y; s1.z += w.z; s1.w += w.w;
                    }
                    if (col_ok) {
                        float* o = a.OH + (long)(node0 + nd) * C + n0 + c8;
                        if (whole) {
                            reinterpret_cast<float4*>(o)[0] = s0;
                            reinterpret_cast<float4*>(o)[1] = s1;
                        } else {
                            atomicAdd(o + 0, s0.x); atomicAdd(o + 1, s0.y); atomicAdd(o + 2, s0.z); atomicAdd(o + 3, s0.w);
                            atomicAdd(o + 4, s1.x); atomicAdd(o + 5, s1.y); atomicAdd(o + 6, s1.z); atomicAdd(o + 7, s1.w);
                        }
                    }
                }
            }
            }
        }
    }
}
template <bool SAVE>
__global__ __launch_bounds__(256, 3) void gemm_cand_split8_kernel(CandArgs a, int uniform) {
    using Core = SplitCore<false, 1>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const long M = (long)a.num_nodes * a.T;
    const int tiles_n = (a.C + GBN - 1) / GBN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const long m0 = (long)(bid / tiles_n) * GBM;
    const int n0 = (bid % tiles_n) * GBN;
    const RowMap rm{m0, 1, (int)((M - m0) < GBM ? (M - m0) : GBM)};
    Core core(a.S, rm, n0, a.C, lds, true);
    CandRowEnt* rowtab = reinterpret_cast<CandRowEnt*>(core.rowtab());
    const int node0 = (int)((unsigned)m0 / (unsigned)a.T), t0 = (int)m0 - node0 * a.T;
    if (threadIdx.x < GBM) {
        const int x = t0 + (threadIdx.x < rm.nvalid ? threadIdx.x : 0), q = (int)(((float)x + 0.5f) * (1.0f / (float)a.T));
        rowtab[threadIdx.x] = CandRowEnt{(q << 8) | (x - q * a.T), a.probs[x - q * a.T]};
    }
    if (!uniform) core.plan();
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    if (uniform == 2) core.run_uniform_frag(acc, false);
    else if (uniform) core.run_uniform(acc, false);
    else core.run(acc, false);
    if (rm.nvalid == GBM && n0 + GBN <= a.C) cand8_epilogue<true, SAVE>(a, core, acc, lds, rowtab, m0, n0, GBM, node0, t0);
    else cand8_epilogue<false, SAVE>(a, core, acc, lds, rowtab, m0, n0, rm.nvalid, node0, t0);
}

template <class Core, bool SAVE>
static int launch_cand_flat(const CandArgs& a, unsigned grid, int lds_bytes, hipStream_t st) {
    if (int rc = want_dynamic_lds<&gemm_cand_flat_kernel<Core, SAVE>>(lds_bytes)) return rc;
    hipLaunchKernelGGL((gemm_cand_flat_kernel<Core, SAVE>), dim3(grid), dim3(256), lds_bytes, st, a);
    return REGT_OK;
}
// the vector kernels over `ftiles` 128 x 128 tiles of the flat (node * T + t) rows
template <bool SAVE>
static int launch_cand_vec(const CandArgs& a, long M, long ftiles, hipStream_t st) {
    const unsigned grid = (unsigned)ftiles;
    // three-workgroup kernels (fp32 storage): 64-row halves need T <= 64 (a node meets at most two halves)
    const bool three = !a.act_bf16 && !fp32_core_wide() && gemm_mode() != 2 && (gemm_mode() == 1 || ftiles >= SMALL_TILE_LIMIT) && M < (1L << 31);
    if (three && gemm_mode() == 0) {
        hipLaunchKernelGGL((gemm_cand_split_kernel<0, SAVE>), dim3(grid), dim3(256), SplitGeom<0>::LDS_BYTES, st, a, uniform_ok(a.S, M));
    } else if (three) {
        hipLaunchKernelGGL((gemm_cand_split_kernel<3, SAVE>), dim3(grid), dim3(256), SplitGeom<3>::LDS_BYTES, st, a, uniform_ok(a.S, M));
    } else if (gemm_mode() == 1) {
        return launch_cand_flat<SplitCore<false, 3>, SAVE>(a, grid, G_FAST_LDS_BYTES, st);
    } else if (gemm_mode() == 2 && a.act_bf16 && a.C % 8 == 0 && M < (1L << 31) && !fp32_core_wide()) {
        for (int q = 0; q < a.S.nseg; ++q)
            REGT_CHECK_ARG(!(a.S.seg[q].flags & SEG_B_FRAG) || uniform_ok(a.S, M) == 2, "candidate gemm: fragment-order weights need K %% 32 == 0");
        hipLaunchKernelGGL(gemm_cand_split8_kernel<SAVE>, dim3(grid), dim3(256), SplitGeom<1>::LDS_BYTES, st, a, uniform_ok(a.S, M));
    } else if (gemm_mode() == 2 && a.act_bf16) {
        for (int q = 0; q < a.S.nseg; ++q)
            REGT_CHECK_ARG(!(a.S.seg[q].flags & SEG_B_FRAG), "candidate gemm: fragment-order weights need the three-workgroup kernel");
        REGT_CHECK_ARG(a.C % 8 == 0, "candidate gemm: bf16 storage needs C %% 8 == 0");
        if (int rc = want_dynamic_lds<&gemm_cand_flat8_kernel<SAVE>>(G_FAST_LDS_BYTES)) return rc;
        hipLaunchKernelGGL(gemm_cand_flat8_kernel<SAVE>, dim3(grid), dim3(256), G_FAST_LDS_BYTES, st, a);
    } else if (gemm_mode() == 2) {
        return launch_cand_flat<SplitCore<false, 1>, SAVE>(a, grid, G_FAST_LDS_BYTES, st);
    } else if (ftiles < SMALL_TILE_LIMIT) {    // small graph: 64 x 64 tiles (a node's T <= 64 rows still span at most two)
        hipLaunchKernelGGL((gemm_cand_flat_kernel<SmallCore<true, false>, SAVE>), dim3((unsigned)(cdiv(M, SM_B) * cdiv(a.C, SM_B))), dim3(256), SM_LDS_BYTES, st, a);
    } else {
        return launch_cand_flat<FastCore<true, false>, SAVE>(a, grid, G_FAST_LDS_BYTES, st);
    }
    return REGT_OK;
}
// `save` = false: the forward-only kernels (H~ not stored, a.Ht ignored); the choice of core is the same either way
int launch_gemm_candidate(const CandArgs& a, hipStream_t st, bool save) {
    REGT_CHECK_ARG(a.num_nodes > 0 && a.T > 0 && a.C > 0, "candidate gemm: empty problem");
    REGT_CHECK_ARG(!save || a.Ht, "candidate gemm: the training form stores H~ (Ht is NULL)");
    long tiles = (long)cdiv(a.num_nodes, GBM) * cdiv(a.C, GBN);
    const bool vec = a.C % 4 == 0 && a16(a.ZR) && a16(a.h) && a16(a.Ht) && a16(a.OH) && a16(a.bias) &&
                     fast_class(a.S, a.C, true) == 1;
    REGT_CHECK_ARG(!a.act_bf16 || (vec && gemm_mode() == 2), "candidate gemm: bf16-stored activations need the bf16-operand vector path");
    if (vec) {
        const long M = (long)a.num_nodes * a.T;
        long ftiles;
        if (int rc = gemm_tiles(M, a.C, GBM, GBN, &ftiles)) return rc;
        REGT_CHECK_ARG(a.T <= 255, "candidate gemm: T > 255");
        if (int rc = launch_zero_f32(a.OH, (long)a.num_nodes * a.C, st)) return rc;
        if (int rc = with_flag(save, [&](auto sv) { return launch_cand_vec<decltype(sv)::value>(a, M, ftiles, st); })) return rc;
    } else {
        for (int q = 0; q < a.S.nseg; ++q)
            REGT_CHECK_ARG(!(a.S.seg[q].flags & SEG_A_BF16), "candidate gemm: a bf16-stored operand needs the bf16-operand vector path");
        if (int rc = with_flag(save, [&](auto sv) -> int {
                constexpr bool SAVE = decltype(sv)::value;
                if (int rc = want_dynamic_lds<&gemm_cand_kernel<SAVE>>(G_LDS_BYTES)) return rc;
                hipLaunchKernelGGL(gemm_cand_kernel<SAVE>, dim3((unsigned)tiles), dim3(256), G_LDS_BYTES, st, a);
                return REGT_OK;
            })) return rc;
    }
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace regt
