// The forward / backward pipeline of the RegT-GCN hot path and the format decisions of a step.
//
// Formulation (validated against the oracle in tests/test_fused_math.py):
// every sparse operator of the reference acts on the *input* x, so
//   * A_hat x and L~ x are aggregated once per snapshot at width T*F (one stacked SpMM) and are
//     constants w.r.t. the parameters -- the backward pass has no sparse op;
//   * every weight that multiplies a width-F quantity is folded into a (C,F) "composed" weight
//     (A0 = (sum_r Wl_r) W0, A_r = Wl_r W1, G_k = U_k[:, :C] V_k), so the only K=C contractions
//     left are the three hidden-state GEMMs of the GRU cell.
// Rows of all (M = N*T, .) activations are ordered node-major: m = node*T + t.
#include <algorithm>

#include "api_internal.h"

namespace regt {

// REGT_GEMM_MODE=bf16: the intermediates that only ever feed matrix-core operands -- q = h*R (forward -> backward), dhp and
// dzp|drp (inside the backward) -- are STORED as bf16: their producer rounds them once instead of every consumer rounding
// them while staging, which is the same arithmetic at half the HBM bytes for these buffers (7.5 of the step's ~37 row-units).
// Needs the vector kernels everywhere (C a multiple of the 128-column tile, so that no GEMM falls back to the generic core).
bool bf16_intermediates(const regt_dims& d) { return gemm_mode() == 2 && d.C % GBN == 0 && d.F % 4 == 0; }
// ... and, where the fused forward kernel applies (fused.hip: C = 256, F = 64, node-disjoint regions), x, A_hat x and L~ x as
// well: the snapshot is rounded once while it is packed, the aggregation reads and writes bf16 rows (cfg-5).
// REGT_XBF=0 keeps them fp32 and the three-launch forward (A/B timing; tests/test_gpu_fused.py compares the two bit for bit).
static bool xbf_wanted() { return !(t_call_flags & REGT_DIMS_NO_BF16_ROWS) && option(OPT_XBF); }
static bool fused_bwd_wanted() { return !(t_call_flags & REGT_DIMS_NO_FUSED_BWD) && option(OPT_FUSED_BWD); }      // REGT_FUSED_BWD
// TemporalGCN / A3T-GCN (regional = 0): the hidden input h = x W0^T + (L~ x) W1^T + b has NO activation (models/TemporalGCN.py:88 --
// RegT-GCN applies leaky_relu, RegionalTemporalGCN.py:143), so wherever the gates use h LINEARLY it folds into the input:
//     h [Uz2; Ur2]^T = x ([Uz2; Ur2] W0)^T + (L~ x) ([Uz2; Ur2] W1)^T + ([Uz2; Ur2] b)^T
// -- the gate GEMM runs at K = 3 F instead of C + F, and in the backward pass the K = 2 C data gradient of the gates (ds, which only
// ever fed weight gradients of that linear map) and the (2C x C) weight gradient dzr^T h become (2C x F) contractions on x and L~ x
// plus tiny compositions.  h itself is still formed: the reset gate multiplies it (q = h * R) and the blend reads it.
// REGT_TGCN_COLLAPSE=0 / regt_set_option("tgcn_collapse", 0): the uncollapsed form (A/B, tests).
static bool tcollapse_wanted() { return option(OPT_TGCN_COLLAPSE) != 0; }
static inline const float* byte_off(const float* p, long bytes) { return reinterpret_cast<const float*>(reinterpret_cast<const char*>(p) + bytes); }

// bf16 mode with bf16-stored activations: the GEMM weights get per-step bf16 copies in MFMA fragment order (SEG_B_FRAG: every
// wave loads its B fragments straight into registers) when every K is a multiple of the 32-k slab
static bool frag_shape_ok(const regt_dims& d) {
    return bf16_intermediates(d) && d.F % 32 == 0 && d.C % 128 == 0 && !gemm_desc_table_forced() && !fp32_core_wide();
}
static bool weights_frag(const regt_dims& d) {
    // ... and every GEMM of the step fits the 64-slab descriptor table of the bf16-operand core (SplitCore::plan_u): the
    // regional embedding repeats its K = F segment once per region a 128-row tile can meet, the gate data gradient has K = 2C
    const long reg_slabs = (long)(std::min<long>(d.R, 128 / d.T + 2) + 1) * (d.F / 32);
    return frag_shape_ok(d) && reg_slabs <= 64 && (2L * d.C + d.F) / 32 <= 64;
}
static bool xbf_ok(const regt_dims& d, const regt_graph& g, bool h_ext, int x_rows, bool packed_fp32) {
    // (fragment-order weights without weights_frag()'s bound on the regional GEMM's slab table: the fused kernel has none)
    return xbf_wanted() && frag_shape_ok(d) && d.regional && d.R > 1 && !g.overlap && !h_ext && g.m_rowptr && g.m_col && g.m_val_a && g.m_val_l &&
           g.chunk_tab && g.chunk_region && g.n_chunks > 0 &&
           fused_forward_ok(d.C, d.F) && ((long)d.T * d.F) % 64 == 0 && (!packed_fp32 || x_rows <= 2 * d.N) &&
           (long)(x_rows > d.N ? x_rows : d.N) * d.T * d.F * 2 < (1L << 32) - 4096;
}
// The row-owning fused forward (fused_rows.hip) instead of the 64-row one: C = 256, F = 32 / 64, T <= 16 and region ids sorted by node.
// The three-launch path of the same arithmetic follows with its per-node sums (CandArgs::node_sum_rows), whichever forward runs:
// the forms stay bit-identical (tests/test_gpu_fused.py).  regt_set_option("fused_rows", 0): the 64-row kernel everywhere; 2: the
// row-owning kernel as two workgroups of four waves per CU (a test variant, see kernels.h).
// regt_set_option("embed_kernel", 0): the regional embedding of the fp32 path through the general GEMM core instead of embed.hip (A/B)
static bool fused_rows_form(const regt_dims& d, const regt_graph& g) {
    return option(OPT_FUSED_ROWS) && fused_forward_rows_ok(d.C, d.F, d.T) && d.regional && !g.overlap && (d.R == 1 || g.region_sorted);
}

// the form a forward takes, decided from host-side fields only (shared by forward_common and the forward-only sizing function)
int forward_format(const regt_dims& d, const regt_graph& g, int x_rows, bool packed_fp32, bool xp_is_bf16) {
    int fmt = bf16_intermediates(d) ? FMT_QBF : 0;
    if (fmt && xbf_ok(d, g, false, x_rows, packed_fp32)) fmt |= FMT_XBF | (xp_is_bf16 ? FMT_XCALLER : 0);
    if (!d.regional && !g.overlap && !(fmt & FMT_QBF) && tcollapse_wanted()) fmt |= FMT_TCOLLAPSE;
    return fmt;
}

// The form of one step, derived in one place from (dims, fmt, whether the hidden input is the caller's); forward_impl and backward_impl
// read the same one.
// Two sources stay apart: `ibf` is THIS call's arithmetic -- the forward stores q in it --, `qbf` is what `fmt` says the forward stored;
// the entry points check that they agree before a backward runs.
struct StepForm {
    int ibf;        // bf16_intermediates(d): q, dhp, dzp|drp are stored as bf16
    int qbf;        // fmt: q was stored as bf16
    int abf;        // ... and h, [Z|R], H~ (dh / ds in the backward) too: everything M x C, unless the hidden input is the caller's
    int xbf;        // fmt: x, A_hat x, L~ x hold bf16 rows
    bool tcol;      // fmt: TemporalGCN, the gates' linear use of h folded into x, L~ x (never with a caller's hidden input: it is not that h)
    bool wfr;       // fragment-order bf16 copies of the GEMM weights (the forward also needs node-disjoint regions for them)
    bool split;     // the three-workgroup GEMM cores: the data gradients read transposed copies of the gate weights
    bool save;      // the forward stores what only the backward reads (not a forward-only call)
};
static StepForm step_form(const regt_dims& d, int fmt, bool h_ext) {
    StepForm f;
    f.ibf = bf16_intermediates(d) ? 1 : 0;
    f.qbf = fmt & FMT_QBF;
    f.abf = f.ibf && !h_ext ? 1 : 0;
    f.xbf = (fmt & FMT_XBF) ? 1 : 0;
    f.tcol = (fmt & FMT_TCOLLAPSE) != 0 && !h_ext;
    f.wfr = f.abf && weights_frag(d) && d.regional;
    // (gemm_split.h: fp32 planes, bf16x3 split, bf16 take weights as [N][K] only; REGT_FP32_CORE=wide keeps the fp32 path on the
    // two-workgroup core, which reads the weights as they are)
    f.split = gemm_mode() != 0 || !fp32_core_wide();
    f.save = !(fmt & FMT_FWDONLY);
    return f;
}

static inline bool fits32(long v) { return v >= INT_MIN && v <= INT_MAX; }
static SgTerm term(const float* A, long sai, long sak, long sab, const float* B, long sbk, long sbj, long sbb, int k, int batch = 1,
            int sum_batch = 0) {
    const bool ok = fits32(sai) && fits32(sak) && fits32(sab) && fits32(sbk) && fits32(sbj) && fits32(sbb) && batch <= SHRT_MAX && k >= 0;
    return SgTerm{A, B, (int)sai, (int)sak, (int)sab, (int)sbk, (int)sbj, (int)sbb, ok ? k : -1, (short)batch, (short)sum_batch};
}
static void add_task(SgBatch& b, float* C, long sci, long scj, long scb, int m, int n, int nbatch, const float* init, long init_si,
              std::initializer_list<SgTerm> terms, long init_sj = 0) {
    bool ok = b.ntask < SG_MAX_TASKS && fits32(sci) && fits32(scj) && fits32(scb) && fits32(init_si) && fits32(init_sj) && nbatch <= SHRT_MAX &&
              terms.size() <= 3;
    for (const SgTerm& q : terms) ok = ok && q.k >= 0;
    if (!ok) { b.overflow = 1; return; }
    SgTask& t = b.task[b.ntask++];
    t = SgTask{};
    t.C = C; t.sci = (int)sci; t.scj = (int)scj; t.scb = (int)scb; t.m = m; t.n = n; t.nbatch = (short)nbatch; t.init = init;
    t.init_si = (int)init_si; t.init_sj = (int)init_sj;
    for (const SgTerm& q : terms) t.term[t.nterm++] = q;
}

// owned region block [lo, hi) of a graph (regt_graph.region_lo / region_hi; 0, 0 = all)
static void region_range(const regt_dims& d, const regt_graph& g, int* lo, int* hi) {
    *lo = 0; *hi = d.R;
    if (g.region_hi > g.region_lo && g.region_lo >= 0 && g.region_hi <= d.R) { *lo = g.region_lo; *hi = g.region_hi; }
}

// All weight compositions of one step in ONE launch (SURVEY/DESIGN section 3, item 2); compose_backward is its mirror.
// `tcol` adds the TemporalGCN compositions of the collapsed gate GEMM.
static int compose_forward(const regt_dims& d, const regt_graph& g, const regt_params& p, const Layout& L, hipStream_t st, bool tcol = false) {
    const int C = d.C, F = d.F, R = d.R;
    const long RC = (long)R * C;
    SgBatch b{};
    if (d.regional) {
        int lo, hi;
        region_range(d, g, &lo, &hi);
        // S = sum_r Wl_r ;  A0 = S W0 ;  A_r = Wl_r W1 (owned regions only) ;  b' = S b_c + b_l
        TRY(launch_sum_region_blocks(p.region_w, L.S, C, R, st));
        add_task(b, L.A0, F, 1, 0, C, F, 1, nullptr, 0, {term(L.S, C, 1, 0, p.cheb_w0, F, 1, 0, C)});
        add_task(b, L.Aall + (long)lo * C * F, F, 1, (long)C * F, C, F, hi - lo, nullptr, 0,
                 {term(p.region_w + (long)lo * C, RC, 1, C, p.cheb_w1, F, 1, 0, C)});
        add_task(b, L.bprime, 1, 0, 0, C, 1, 1, p.region_b, 1, {term(L.S, C, 1, 0, p.cheb_bias, 1, 0, 0, C)});
    }
    for (int k = 0; k < 3; ++k) {
        float* G = k < 2 ? L.Gzr + (long)k * C * F : L.Gh;
        float* c = k < 2 ? L.czr + (long)k * C : L.ch;
        // G_k = U_k[:, :C] V_k ;  c_k = U_k[:, :C] beta_k + u_k
        add_task(b, G, F, 1, 0, C, F, 1, nullptr, 0, {term(p.gate_w[k], 2L * C, 1, 0, p.conv_lin_w[k], F, 1, 0, C)});
        add_task(b, c, 1, 0, 0, C, 1, 1, p.gate_b[k], 1, {term(p.gate_w[k], 2L * C, 1, 0, p.conv_bias[k], 1, 0, 0, C)});
    }
    if (tcol) {
        for (int k = 0; k < 2; ++k) {
            const float* U2 = p.gate_w[k] + C;          // (C x C), row stride 2C: the H half of linear_z / linear_r
            // P0_k = U_k2 W0 ; P1_k = U_k2 W1 ; c'_k = u_k + U_k1 beta_k + U_k2 b
            add_task(b, L.P0zr + (long)k * C * F, F, 1, 0, C, F, 1, nullptr, 0, {term(U2, 2L * C, 1, 0, p.cheb_w0, F, 1, 0, C)});
            add_task(b, L.P1zr + (long)k * C * F, F, 1, 0, C, F, 1, nullptr, 0, {term(U2, 2L * C, 1, 0, p.cheb_w1, F, 1, 0, C)});
            add_task(b, L.czr2 + (long)k * C, 1, 0, 0, C, 1, 1, p.gate_b[k], 1,
                     {term(p.gate_w[k], 2L * C, 1, 0, p.conv_bias[k], 1, 0, 0, C), term(U2, 2L * C, 1, 0, p.cheb_bias, 1, 0, 0, C)});
        }
    }
    return launch_small_gemm_multi(b, st);
}

// head of every model on the path: relu -> linear1 -> relu -> linear2 (models/RegionalTemporalGCN.py:35-38); y1 (N, H1) is kept
// for the backward pass
int head_forward(const regt_dims& d, const regt_params& p, const float* hidden, float* y1, float* pred, hipStream_t st) {
    const int N = d.N, C = d.C, O = d.O, H1 = d.H1;
    EpiBiasAct e{y1, H1, p.head1_b, ACT_RELU, 0.f};
    PROF("head_fwd", st);
    TRY(launch_gemm_bias_act(one_seg(make_seg(hidden, C, p.head1_w, nullptr, C, INT_MAX, C, true, SEG_RELU_A)), N, H1, e, st));
    if (head2_skinny_ok(H1, O, y1, p.head2_w)) return launch_head2_fwd(y1, p.head2_w, p.head2_b, pred, N, H1, O, st);
    EpiBiasAct e2{pred, O, p.head2_b, ACT_NONE, 0.f};
    return launch_gemm_bias_act(one_seg(make_seg(y1, H1, p.head2_w, nullptr, H1, INT_MAX, H1, true)), N, O, e2, st);
}

// bf16 copies, in MFMA fragment order, of the weights the forward GEMMs read (bf16 arithmetic with fragment-order weights: regional
// models only, so A0 / A_r are the composed ones).  C % 128 == 0: region r of A_r starts at block row r C / 32.
static int weights_to_frag(const regt_dims& d, const regt_params& p, const Layout& L, const WbPtrs& wb, hipStream_t st) {
    const int F = d.F, C = d.C;
    CvtBatch cb{};
    cb.n = 0;
    for (int k = 0; k < 3; ++k) cb.t[cb.n++] = CvtTask{p.gate_w[k] + C, 2L * C, C, C, const_cast<float*>(wb.U[k])};
    cb.t[cb.n++] = CvtTask{L.Gzr, F, 2 * C, F, const_cast<float*>(wb.Gzr)};
    cb.t[cb.n++] = CvtTask{L.Gh, F, C, F, const_cast<float*>(wb.Gh)};
    cb.t[cb.n++] = CvtTask{L.A0, F, C, F, const_cast<float*>(wb.A0)};
    cb.t[cb.n++] = CvtTask{L.Aall, F, d.R * C, F, const_cast<float*>(wb.Aall)};
    PROF("weights_bf16", st);
    return launch_cvt_bf16_frag(cb, st);
}

// The forward on bf16 rows (FMT_XBF, chosen by xbf_ok): x, A_hat x, L~ x as bf16 rows and the whole cell as ONE kernel -- the row-owning
// one (fused_rows.hip) where fused_rows_form() holds, else the 64-row one (fused.hip) --, then the head.
static int forward_bf16_rows(const regt_dims& d, const regt_graph& g, const regt_params& p, const float* x, const float* xp_ext, int x_rows,
                             float* pred, float* hidden, const Layout& L, hipStream_t st, bool skip_pack, int fmt, bool save) {
    const int N = d.N, T = d.T, F = d.F, C = d.C;
    const void* Xb = (fmt & FMT_XCALLER) ? static_cast<const void*>(xp_ext) : static_cast<const void*>(L.Xp);
    if (!(fmt & FMT_XCALLER) && !skip_pack) {
        PROF("pack_x", st);
        if (xp_ext) TRY(launch_cvt_rows_bf16(xp_ext, L.Xp, (long)x_rows * T * F, st));
        else TRY(launch_pack_x_bf16(x, L.Xp, N, F, T, st));
    }
    {
        PROF("spmm", st);
        TRY(launch_spmm_dual_bf16(g.m_rowptr, g.m_col, g.m_val_a, g.m_val_l, Xb, L.AX, L.LX, N, xp_ext ? x_rows : N, T * F, st));
    }
    const WbPtrs wb = wb_ptrs(L.Wb, C, F);
    TRY(side_join(st));                      // composed weights ready
    TRY(weights_to_frag(d, p, L, wb, st));
    {
        FusedFwdArgs a{};
        a.X = Xb; a.LX = L.LX; a.AX = L.AX;
        a.A0f = wb.A0; a.Aallf = wb.Aall; a.ar_stride = wb.ar_stride;
        a.Uzf = wb.U[0]; a.Urf = wb.U[1]; a.Uhf = wb.U[2]; a.Gzrf = wb.Gzr; a.Ghf = wb.Gh;
        a.bprime = L.bprime; a.czr = L.czr; a.ch = L.ch; a.probs = L.probs;
        a.node_region = d.R > 1 ? g.node_region : nullptr;
        a.h = L.h; a.ZR = L.ZR; a.q = L.q; a.Ht = L.Ht; a.OH = hidden;      // (forward-only layout: all four NULL, never touched)
        a.M = (long)N * T; a.T = T; a.slope = d.lrelu_slope; a.act_lrelu = 1; a.tile_ctr = L.tile_ctr;
        PROF("fused_forward", st);
        TRY(launch_zero_f32(hidden, (long)N * C, st));
        if (fused_rows_form(d, g)) TRY(launch_fused_forward_rows(a, C, F, option(OPT_FUSED_ROWS) == 2 ? 4 : 8, st, save));
        else TRY(launch_fused_forward(a, C, F, st, save));
    }
    if (d.flags & REGT_DIMS_NO_HEAD) return REGT_OK;
    return head_forward(d, p, hidden, L.y1, pred, st);
}

// The forward: weight compositions on the side stream, then either the bf16-row form above (FMT_XBF) or five stages on the launch
// stream: pack + aggregate, regional embedding, gates, candidate + blend + attention sum, head.
// `h_ext` != NULL: the cell's hidden input (M x C, rows node*T + t) comes from the caller (regt_cell_forward); the
// regional / Cheb embedding stage is skipped and only A_hat x is aggregated (graph = the N rows of A_hat).
int forward_impl(const regt_dims& d, const regt_graph& g, const regt_params& p, const float* x, const float* xp_ext,
                 int x_rows, float* pred, float* hidden, const Layout& L, hipStream_t st, bool skip_pack, const float* h_ext, int fmt) {
    const int N = d.N, T = d.T, F = d.F, C = d.C, R = d.R;
    const long M = (long)N * T;
    const float* H = h_ext ? h_ext : L.h;
    const StepForm f = step_form(d, fmt, h_ext != nullptr);
    const int qbf = f.ibf, abf = f.abf;      // the forward is q's producer: it stores q in this call's arithmetic
    const bool save = f.save;                // forward-only: the kernels that store nothing the backward alone reads
    // The weight compositions do not depend on the snapshot: they run on the side stream next to pack_x + aggregation and are
    // joined in front of their first consumer (0.03-0.10 ms per step off the critical path at every size).
    {
        hipStream_t sc = side_fork(st);
        PROF("compose_fwd", sc);
        TRY(launch_softmax_small(p.attention, L.probs, T, sc));
        TRY(compose_forward(d, g, p, L, sc, f.tcol));
    }
    if (f.xbf) return forward_bf16_rows(d, g, p, x, xp_ext, x_rows, pred, hidden, L, st, skip_pack, fmt, save);
    // 1. pack the snapshot and aggregate: [A_hat; L~] x  (one stacked SpMM over 2N rows, width T*F)
    const float* Xp = xp_ext ? xp_ext : L.Xp;
    if (!xp_ext && !skip_pack) {
        PROF("pack_x", st);
        TRY(launch_pack_x(x, L.Xp, N, F, T, st));
    }
    {
        PROF("spmm", st);
        if (h_ext)
            TRY(launch_spmm_csr(g.rowptr, g.col, g.val, Xp, L.AX, N, xp_ext ? x_rows : N, T * F, 1, st));
        else if (g.overlap)
            TRY(launch_spmm_csr(g.rowptr, g.col, g.val, Xp, L.AX, (1 + R) * N, xp_ext ? x_rows : N, T * F, 1 + R, st));
        else if (g.m_rowptr && g.m_col && g.m_val_a && g.m_val_l && ((T * F) % 32 == 0 || T * F <= 2048))
            TRY(launch_spmm_dual_x(g.m_rowptr, g.m_col, g.m_val_a, g.m_val_l, Xp, L.AX, L.LX, N, xp_ext ? x_rows : N, T * F, st));
        else
            TRY(launch_spmm_csr(g.rowptr, g.col, g.val, Xp, L.AX, 2 * N, xp_ext ? x_rows : N, T * F, 2, st));
    }
    TRY(side_join(st));                          // composed weights ready
    const float* A0 = d.regional ? L.A0 : p.cheb_w0;
    const float* Aall = d.regional ? L.Aall : p.cheb_w1;
    const float* bpr = d.regional ? L.bprime : p.cheb_bias;
    const bool wfr = f.wfr && !g.overlap;      // (the repeated segments of overlapping regions have no fragment-order form)
    const WbPtrs wb = wb_ptrs(L.Wb, C, F);
    if (wfr) TRY(weights_to_frag(d, p, L, wb, st));
    // 2. regional embedding h = act(x A0^T + (L~ x) A_region^T + b')
    if (!h_ext) {
        GemmSegs S{};
        S.nseg = 2;
        if (wfr) {
            S.seg[0] = make_seg(Xp, F, wb.A0, nullptr, F, INT_MAX, F, true, SEG_B_FRAG);
            S.seg[1] = make_seg(L.LX, F, wb.Aall, nullptr, F, INT_MAX, F, true, (R > 1 ? SEG_REGION : 0) | SEG_B_FRAG, wb.ar_stride);
        } else {
            S.seg[0] = make_seg(Xp, F, A0, nullptr, F, INT_MAX, F, true);
            S.seg[1] = make_seg(L.LX, F, Aall, nullptr, F, INT_MAX, F, true,
                                g.overlap ? SEG_REPEAT : (R > 1 ? SEG_REGION : 0), (long)C * F);
        }
        S.seg[1].a_rep_stride = M * F;
        S.seg[1].nrep = R;
        S.node_region = g.node_region;
        S.row_div = T;
        int lo, hi;
        region_range(d, g, &lo, &hi);
        S.num_regions = hi - lo;                 // a row tile can only meet the regions that own rows here
        EpiBiasAct e{L.h, C, bpr, d.regional ? ACT_LRELU : ACT_NONE, d.lrelu_slope};
        e.out_bf16 = abf;
        PROF("gemm_regional", st);
        // fp32 at C = 256, F = 32 with node-sorted region ids: the kernel written for this shape (embed.hip); everything else: the general core
        if (!wfr && !abf && gemm_mode() == 0 && !fp32_core_wide() && !gemm_desc_table_forced() && option(OPT_EMBED_KERNEL) && d.regional && !g.overlap &&
            (R == 1 || g.region_sorted) && embed_fp32_ok(M, C, F, T)) {
            TRY(launch_embed_fp32(Xp, L.LX, A0, Aall, R > 1 ? g.node_region : nullptr, bpr, L.h, M, T, ACT_LRELU, d.lrelu_slope, st));
        } else {
            TRY(launch_gemm_bias_act(S, M, C, e, st));
        }
    }
    // 3. update + reset gates: [Z|R] = sigmoid(h [Uz2;Ur2]^T + (A_hat x) [Gz;Gr]^T + [cz;cr]),  q = h*R
    {
        GemmSegs S{};
        S.nseg = 2;
        if (wfr) {
            S.seg[0] = make_seg(H, C, wb.U[0], wb.U[1], C, C, C, true, SEG_A_BF16 | SEG_B_FRAG);
            S.seg[1] = make_seg(L.AX, F, wb.Gzr, nullptr, F, INT_MAX, F, true, SEG_B_FRAG);
        } else if (f.tcol) {      // K = 3 F: the linear hidden input folded into x and L~ x
            S.nseg = 3;
            S.seg[0] = make_seg(Xp, F, L.P0zr, nullptr, F, INT_MAX, F, true);
            S.seg[1] = make_seg(L.LX, F, L.P1zr, nullptr, F, INT_MAX, F, true);
            S.seg[2] = make_seg(L.AX, F, L.Gzr, nullptr, F, INT_MAX, F, true);
        } else {
            S.seg[0] = make_seg(H, C, p.gate_w[0] + C, p.gate_w[1] + C, 2L * C, C, C, true, abf ? SEG_A_BF16 : 0);
            S.seg[1] = make_seg(L.AX, F, L.Gzr, nullptr, F, INT_MAX, F, true);
        }
        S.row_div = T;
        EpiGates e{L.ZR, H, L.q, f.tcol ? L.czr2 : L.czr, C};
        e.q_bf16 = qbf; e.h_bf16 = abf; e.zr_bf16 = abf;
        PROF("gemm_gates", st);
        TRY(launch_gemm_gates(S, M, 2 * C, e, st, save));
    }
    // 4. candidate state, GRU blend and attention-weighted sum over periods -> hidden (N,C)
    {
        CandArgs a{};
        a.S.nseg = 2;
        if (wfr) {
            a.S.seg[0] = make_seg(L.q, C, wb.U[2], nullptr, C, INT_MAX, C, true, (qbf ? SEG_A_BF16 : 0) | SEG_B_FRAG);
            a.S.seg[1] = make_seg(L.AX, F, wb.Gh, nullptr, F, INT_MAX, F, true, SEG_B_FRAG);
        } else {
            a.S.seg[0] = make_seg(L.q, C, p.gate_w[2] + C, nullptr, 2L * C, INT_MAX, C, true, qbf ? SEG_A_BF16 : 0);
            a.S.seg[1] = make_seg(L.AX, F, L.Gh, nullptr, F, INT_MAX, F, true);
        }
        a.S.row_div = T;
        a.num_nodes = N; a.T = T; a.C = C;
        a.bias = L.ch; a.ZR = L.ZR; a.h = H; a.probs = L.probs; a.Ht = L.Ht; a.OH = hidden;
        a.act_bf16 = abf;
        a.node_sum_rows = abf && fused_rows_form(d, g) ? 16 : 64;
        PROF("gemm_candidate", st);
        TRY(launch_gemm_candidate(a, st, save));
    }
    // 5. head: relu -> linear1 -> relu -> linear2  (REGT_DIMS_NO_HEAD: the caller runs it elsewhere)
    if (d.flags & REGT_DIMS_NO_HEAD) return REGT_OK;
    return head_forward(d, p, hidden, L.y1, pred, st);
}

int wgrad_full(ReduceQueue& q, const char* name, const float* P, long ldp, int Nout, const float* Q, long ldq, int Nin, int q_relu,
               long M, int kchunk, int nchunks, float* out, long ldo, float* colsum, hipStream_t st, int p_bf16, int q_bf16) {
    WgradArgs a{P, ldp, Nout, Q, ldq, Nin, q_relu, M, kchunk, nullptr, nchunks, nullptr, colsum ? 1 : 0};
    a.p_bf16 = p_bf16; a.q_bf16 = q_bf16;
    WgradSlab w;
    TRY(wgrad_launch(q, a, name, st, &w));
    return q.push(w.block(0, Nout, Nin, out, ldo).colsum(colsum, (long)Nout * Nin, Nout));
}

// backward of head_forward: weight / bias gradients of linear2 and linear1 (slabs queued on `rq`) and
// dOH = (d1 A1) * (hidden > 0) + dhidden, the gradient of the attention-weighted hidden state.
// head2_skinny_ok (output_dim <= 4) selects the row-wise kernels of the last layer; its two weight gradients then run on the side stream.
int head_backward(const regt_dims& d, const regt_params& p, const regt_grads& gr, const float* dpred, const float* dhidden,
                  const float* hidden, const float* y1, float* d1, float* dOH, ReduceQueue& rq, hipStream_t st) {
    const int N = d.N, C = d.C, O = d.O, H1 = d.H1;
    const HeadChunks hc = head_chunks(N, H1, C);
    if (head2_skinny_ok(H1, O, y1, p.head2_w)) {
        WgradSlab w2;
        TRY(wgrad_slab(rq, hc.n2, (long)O * H1 + O, H1, &w2));
        {   // d1 first: the weight gradients leave the critical path behind it (side stream)
            PROF("head_bwd", st);
            TRY(launch_head2_bwd(dpred, p.head2_w, y1, d1, N, H1, O, st));
        }
        hipStream_t ss = side_fork(st);
        {
            PROF("wgrad_head2", ss);
            TRY(launch_head2_wgrad(dpred, y1, w2.slab, N, H1, O, hc.k2, hc.n2, 1, ss));
        }
        TRY(rq.push(w2.block(0, O, H1, gr.head2_w, H1).colsum(gr.head2_b, (long)O * H1, O)));
        TRY(wgrad_full(rq, "wgrad_head1", d1, H1, H1, hidden, C, C, 1, N, hc.k1, hc.n1, gr.head1_w, C, gr.head1_b, ss));
    } else {
        TRY(wgrad_full(rq, "wgrad_head2", dpred, O, O, y1, H1, H1, 0, N, hc.k1, hc.n1, gr.head2_w, H1, gr.head2_b, st));
        // d1 = (dpred A2) * (y1 > 0)      (this head_bwd scope has always spanned wgrad_head1 as well: kept, the profile's figures stay comparable)
        EpiMaskAdd e{d1, H1, y1, H1, nullptr, 0};
        PROF("head_bwd", st);
        TRY(launch_gemm_mask_add(one_seg(make_seg(dpred, O, p.head2_w, nullptr, H1, INT_MAX, O, false)), N, H1, e, st));
        TRY(wgrad_full(rq, "wgrad_head1", d1, H1, H1, hidden, C, C, 1, N, hc.k1, hc.n1, gr.head1_w, C, gr.head1_b, st));
    }
    // dOH = (d1 A1) * (hidden > 0) + dhidden
    EpiMaskAdd e{dOH, C, hidden, C, dhidden, C};
    PROF("head_bwd", st);
    return launch_gemm_mask_add(one_seg(make_seg(d1, H1, p.head1_w, nullptr, C, INT_MAX, H1, false)), N, C, e, st);
}

// What the stages of one backward pass share.
struct Bwd {
    const regt_dims& d; const regt_graph& g; const regt_params& p; const regt_grads& gr; const Layout& L;
    StepForm f;
    WbPtrs wb;
    const float* Xp;        // the packed input the forward read
    const float* H;         // the hidden input: L.h, or the caller's (`ext`)
    float* DH;              // its gradient: L.dh, or the caller's
    bool ext;               // regt_cell_backward: no embedding stage
    hipStream_t st;
};

// Tail of the attention gradient: off the critical path (side stream), joined before the slab reduction.  `parts` partial dots per row
// are summed first (1: fused backward, C / 128: generated-operand kernel); 0: cell_bwd left the per-block sums complete.
static int attention_tail(const Bwd& b, int parts) {
    const Layout& L = b.L;
    if (!b.gr.attention) return REGT_OK;
    hipStream_t sa = side_fork(b.st);
    if (parts) TRY(launch_rowdot_reduce(L.rowdot, L.dp_partial, b.d.N, b.d.T, L.cb_npb, sa, parts));
    return launch_att_bwd(L.dp_partial, L.cb_blocks, L.probs, b.gr.attention, b.d.T, sa);
}

// Data gradients of the cell: dhp, dzp | drp (the left operands of the weight gradients), dh and ds = d(hidden input), in one of
// three forms, flat:
//   fused    bf16 arithmetic with fragment-order weights: ONE kernel (fused.hip), every activation read and written once; the same
//            results bit for bit except the summation order of the attention gradient.  REGT_FUSED_BWD=0 / REGT_DIMS_NO_FUSED_BWD: off.
//   gen      fp32 / bf16x3 at sizes the 128 x 128 core covers: dhp is GENERATED inside the candidate data gradient's K loop, dzp and the
//            attention dots come out of its epilogue -- cell_bwd's pass over Z, h, H~ (5 C floats per row) does not happen
//            (gemm_split.h: run_u_gen).  REGT_DGRAD1_GEN=0: off.
//   two      cell_bwd, then the candidate data gradient.
// The gate data gradient (dgrad_gates) follows gen and two -- the fused kernel holds it -- unless the collapsed TemporalGCN form never
// forms ds.
static int data_gradients(const Bwd& b) {
    const regt_dims& d = b.d; const regt_params& p = b.p; const Layout& L = b.L; const StepForm& f = b.f; const WbPtrs& wb = b.wb;
    const int N = d.N, T = d.T, C = d.C;
    const long M = (long)N * T;
    hipStream_t st = b.st;
    if (f.split) {      // transposed copies of the three C x C blocks (h, z, r)
        PROF("transpose_gate_w", st);
        TRY(launch_transpose3(p.gate_w[2] + C, p.gate_w[0] + C, p.gate_w[1] + C, 3, L.UT, C, C, 2L * C, st));
    }
    if (f.wfr) {
        CvtBatch cb{};
        cb.n = 3;
        for (int k = 0; k < 3; ++k) cb.t[k] = CvtTask{L.UT + (long)k * C * C, C, C, C, const_cast<float*>(wb.UT[k])};
        PROF("weights_bf16", st);
        TRY(launch_cvt_bf16_frag(cb, st));
    }
    const bool fused = f.wfr && !b.ext && fused_backward_ok(C) && fused_bwd_wanted();
    const bool gen = !fused && f.split && !f.ibf && !f.abf && gemm_dgrad1_gen_ok(M, C, N) && al16(L.Ht) && al16(L.dhp);
    if (fused) {
        FusedBwdArgs a{};
        a.ZR = L.ZR; a.h = b.H; a.Ht = L.Ht; a.dOH = L.dOH; a.probs = L.probs;
        a.UhTf = wb.UT[0]; a.UzTf = wb.UT[1]; a.UrTf = wb.UT[2];
        a.dhp = L.dhp; a.dzr = L.dzr; a.dh = b.DH; a.rowdot = L.rowdot;
        a.M = M; a.T = T; a.slope = d.lrelu_slope; a.act_lrelu = d.regional ? 1 : 0; a.tile_ctr = L.tile_ctr;
        {
            PROF("fused_backward", st);
            TRY(launch_fused_backward(a, C, st));
        }
        return attention_tail(b, 1);
    }
    if (gen) {
        EpiDgrad1 e{b.H, L.ZR, L.dOH, L.probs, L.dzr, b.DH, C, T};
        e.Ht = L.Ht; e.dhp = L.dhp; e.rowdot = L.rowdot; e.num_nodes = N;
        {
            PROF("dgrad_candidate", st);      // (A is generated: the segment's pointer is not read)
            TRY(launch_gemm_dgrad1_gen(one_seg(make_seg(L.dhp, C, L.UT, nullptr, C, INT_MAX, C, true), T), M, C, e, st));
        }
        TRY(attention_tail(b, C / 128));
    } else {
        CellBwdArgs a{L.dOH, L.probs, L.ZR, b.H, L.Ht, L.dhp, L.dzr, L.dp_partial, N, T, C, L.cb_npb};
        a.out_bf16 = f.ibf; a.in_bf16 = f.abf;
        {
            PROF("cell_bwd", st);
            TRY(launch_cell_bwd(a, st));
        }
        TRY(attention_tail(b, 0));
        // dq = dhp Uh2 ; drp -> dzr[:, C:], dh = dq*R + p_t dOH Z
        const GemmSeg s = f.wfr   ? make_seg(L.dhp, C, wb.UT[0], nullptr, C, INT_MAX, C, true, SEG_A_BF16 | SEG_B_FRAG)
                        : f.split ? make_seg(L.dhp, C, L.UT, nullptr, C, INT_MAX, C, true, f.ibf ? SEG_A_BF16 : 0)
                                  : make_seg(L.dhp, C, p.gate_w[2] + C, nullptr, 2L * C, INT_MAX, C, false);
        EpiDgrad1 e{b.H, L.ZR, L.dOH, L.probs, L.dzr, b.DH, C, T};
        e.dzr_bf16 = f.ibf; e.h_bf16 = f.abf; e.zr_bf16 = f.abf; e.dh_bf16 = f.abf;
        PROF("dgrad_candidate", st);
        TRY(launch_gemm_dgrad1(one_seg(s, T), M, C, e, st));
    }
    if (f.tcol) return REGT_OK;      // ds is never formed: dh alone feeds dW0 / dW1 / db
    // ds = (dh + dzp Uz2 + drp Ur2) * act'(h)
    GemmSegs S{};
    S.nseg = 2;
    if (f.wfr) {      // (drp first: the accumulation order of the fused kernel, which multiplies drp while dzp is still on its way)
        S.seg[0] = make_seg(byte_off(L.dzr, 2L * C), 2L * C, wb.UT[2], nullptr, C, INT_MAX, C, true, SEG_A_BF16 | SEG_B_FRAG);
        S.seg[1] = make_seg(L.dzr, 2L * C, wb.UT[1], nullptr, C, INT_MAX, C, true, SEG_A_BF16 | SEG_B_FRAG);
    } else if (f.split) {
        const int fl = f.ibf ? SEG_A_BF16 : 0;
        S.seg[0] = make_seg(byte_off(L.dzr, (f.ibf ? 2L : 4L) * C), 2L * C, L.UT + 2L * C * C, nullptr, C, INT_MAX, C, true, fl);
        S.seg[1] = make_seg(L.dzr, 2L * C, L.UT + (long)C * C, nullptr, C, INT_MAX, C, true, fl);
    } else {
        S.seg[0] = make_seg(L.dzr, 2L * C, p.gate_w[0] + C, nullptr, 2L * C, INT_MAX, C, false);
        S.seg[1] = make_seg(L.dzr + C, 2L * C, p.gate_w[1] + C, nullptr, 2L * C, INT_MAX, C, false);
    }
    S.row_div = T;
    EpiDgrad2 e{b.DH, b.H, C, d.regional ? ACT_LRELU : ACT_NONE, d.lrelu_slope};
    e.h_bf16 = f.abf; e.dh_bf16 = f.abf;
    PROF("dgrad_gates", st);
    return launch_gemm_dgrad2(S, M, C, e, st);
}

// ---- weight gradients of the K = C contractions and of the composed (C, F) weights -----------------------------------------------------
// The (C x F)-sized gradients (Gh, Gzr, A0 | A_r) are HBM-bound -- they stream dhp / dzp|drp / ds for a K = F..2F product -- while the
// two big ones (Uh, Uzr) sit on the matrix pipe.  All run on the launch stream (issuing the former on the side stream so that the two
// kinds overlap measured as noise).

// dUh = dhp^T q, column sums -> dch
static int wgrad_Uh(const Bwd& b, ReduceQueue& rq) {
    const Layout& L = b.L; const StepForm& f = b.f;
    const int C = b.d.C;
    const long M = (long)b.d.N * b.d.T;
    int kc = L.kchunk, nc = L.nchunks;
    if (!f.ibf && !f.qbf) wgrad_wide_chunking(C, C, M, &kc, &nc);
    return wgrad_full(rq, "wgrad_Uh", L.dhp, C, C, L.q, C, C, 0, M, kc, nc, b.gr.gate_w[2] + C, 2L * C, L.dch, b.st, f.ibf, f.qbf);
}
// dG = P^T (A_hat x) for P = dhp (Nout = C: dGh) or dzp|drp (Nout = 2C: dGzr)
static int wgrad_G(const Bwd& b, ReduceQueue& rq, const char* name, const float* P, int Nout, float* out) {
    const Layout& L = b.L; const StepForm& f = b.f;
    const int F = b.d.F;
    const long M = (long)b.d.N * b.d.T;
    int kc = L.kchunk_s, nc = L.nchunks_s;
    if (!f.ibf && !f.xbf && F <= 32) wgrad_skinny_chunking(Nout, M, &kc, &nc);
    return wgrad_full(rq, name, P, Nout, Nout, L.AX, F, F, 0, M, kc, nc, out, F, nullptr, b.st, f.ibf, f.xbf);
}
// [dUz2; dUr2] = dzr^T h, column sums -> [dcz; dcr]
static int wgrad_Uzr(const Bwd& b, ReduceQueue& rq) {
    const Layout& L = b.L; const StepForm& f = b.f;
    const int C = b.d.C;
    const long M = (long)b.d.N * b.d.T;
    int kc = L.kchunk, nc = L.nchunks;
    if (!f.ibf && !f.abf) wgrad_wide_chunking(2 * C, C, M, &kc, &nc);
    WgradArgs a{L.dzr, 2L * C, 2 * C, b.H, C, C, 0, M, kc, nullptr, nc, nullptr, 1};
    a.p_bf16 = f.ibf; a.q_bf16 = f.abf;
    WgradSlab w;
    TRY(wgrad_launch(rq, a, "wgrad_Uzr", b.st, &w));
    for (int k = 0; k < 2; ++k)
        TRY(rq.push(w.block((long)k * C * C, C, C, b.gr.gate_w[k] + C, 2L * C).colsum(k == 0 ? L.dczr : nullptr, 2L * C * C, 2 * C)));
    return REGT_OK;
}
// Collapsed TemporalGCN: [dP0 | dP1] = dzr^T [x | L~ x]  (2C x 2F), column sums -> [dcz; dcr]: what is left of dzr^T h (compose_backward
// turns it into dUz2 / dUr2 / dW0 / dW1 / db).  One launch with a two-part right-hand side when F is a multiple of the 32-column
// tile, else one launch per part.
static int wgrad_P01(const Bwd& b, ReduceQueue& rq) {
    const Layout& L = b.L; const StepForm& f = b.f;
    const int F = b.d.F, C = b.d.C;
    const long M = (long)b.d.N * b.d.T;
    const bool two = F % 32 == 0;
    const int Nin = two ? 2 * F : F;
    for (int part = 0; part < (two ? 1 : 2); ++part) {
        int kcs = L.kchunk_s, ncs = L.nchunks_s;
        if (!f.ibf && !f.xbf && Nin <= 64) wgrad_skinny_chunking(2 * C, M, &kcs, &ncs);      // one wave of workgroups
        WgradArgs a{L.dzr, 2L * C, 2 * C, part ? L.LX : b.Xp, F, Nin, 0, M, kcs, nullptr, ncs, nullptr, part == 0 ? 1 : 0};
        if (two) { a.Q2 = L.LX; a.ldq2 = F; a.nin_split = F; }
        WgradSlab w;
        TRY(wgrad_launch(rq, a, "wgrad_P01", b.st, &w));
        TRY(rq.push(w.block(0, 2 * C, Nin, L.dP01 + (two ? 0 : part * F), 2L * F).colsum(part == 0 ? L.dczr : nullptr, 2L * C * Nin, 2 * C)));
    }
    return REGT_OK;
}
// Paired form (bf16 rows, the fused kernels' layout): dUh | dGh = dhp^T [q | A_hat x] and dUzr | dGzr = dzr^T [h | A_hat x] as ONE launch
// each -- the A_hat x part is a third column tile of the same row chunk on the same XCD, so dhp / dzp|drp cross HBM once instead of
// twice.  Measured: slower than the four launches (1.86 vs 1.44 ms at the cfg-5 shard) while every tile issued the loads of BOTH
// right-hand operands; since a column tile that lies entirely in one operand issues one load (wgrad_split_kernel q_tile) and with the
// ring kernel it wins (0.64 + 0.43 against 0.54 + 0.35 + 0.29 + 0.18 ms).  Hence the default: paired whenever the ring kernel is active --
// regt_set_option("wgrad_pairs", 0 | 1 | 2 = follow the ring kernel).
static int wgrad_paired(const Bwd& b, ReduceQueue& rq) {
    const Layout& L = b.L;
    const int F = b.d.F, C = b.d.C;
    const long M = (long)b.d.N * b.d.T;
    WgradSlab w;
    {
        int kc = L.kchunk, nc = L.nchunks;
        wgrad_ring_chunking(C, C + F, M, &kc, &nc);          // one wave of workgroups (ring kernel), else the layout's chunks
        WgradArgs a{L.dhp, C, C, L.q, C, C + F, 0, M, kc, nullptr, nc, nullptr, 1};
        a.p_bf16 = 1; a.q_bf16 = 1; a.Q2 = L.AX; a.ldq2 = F; a.nin_split = C;
        TRY(wgrad_launch(rq, a, "wgrad_UhGh", b.st, &w));
        TRY(rq.push(w.block(0, C, C, b.gr.gate_w[2] + C, 2L * C).colsum(L.dch, (long)C * (C + F), C)));
        TRY(rq.push(w.block(C, C, F, L.dGh, F)));
    }
    int kc = L.kchunk, nc = L.nchunks;
    wgrad_ring_chunking(2 * C, C + F, M, &kc, &nc);
    WgradArgs a{L.dzr, 2L * C, 2 * C, b.H, C, C + F, 0, M, kc, nullptr, nc, nullptr, 1};
    a.p_bf16 = 1; a.q_bf16 = 1; a.Q2 = L.AX; a.ldq2 = F; a.nin_split = C;
    TRY(wgrad_launch(rq, a, "wgrad_UzrGzr", b.st, &w));
    for (int k = 0; k < 2; ++k)
        TRY(rq.push(w.block((long)k * C * (C + F), C, C, b.gr.gate_w[k] + C, 2L * C).colsum(k == 0 ? L.dczr : nullptr, 2L * C * (C + F), 2 * C)));
    return rq.push(w.block(C, 2 * C, F, L.dGzr, F));
}
// Embedding gradients dA0 = ds^T x (column sums -> db') and dA_r = ds^T (L~ x), per region.  (TemporalGCN: the Cheb weights themselves.)
static int wgrad_embedding(const Bwd& b, ReduceQueue& rq) {
    if (b.ext) return REGT_OK;      // no embedding stage behind a caller-supplied hidden input
    const regt_dims& d = b.d; const regt_graph& g = b.g; const Layout& L = b.L; const StepForm& f = b.f;
    const int F = d.F, C = d.C, R = d.R;
    const long M = (long)d.N * d.T;
    float* dA0 = d.regional ? L.dA0 : b.gr.cheb_w0;
    float* dAall = d.regional ? L.dAall : b.gr.cheb_w1;
    float* dbpr = d.regional ? L.dbprime : b.gr.cheb_bias;
    if (!g.overlap && R > 1 && F % 32 == 0) {
        // node-disjoint regions (the headline case): dA0 and dA_r share ds -- one launch over the region-pure row chunks with
        // [x | L~ x] as a two-part right-hand side, so that ds is read from HBM once
        REGT_CHECK_ARG(g.chunk_tab && g.chunk_region && g.n_chunks > 0, "backward: region chunk table missing");
        WgradArgs a{L.dh, C, C, b.Xp, F, 2 * F, 0, M, 0, g.chunk_tab, g.n_chunks, nullptr, 1};
        a.Q2 = L.LX; a.ldq2 = F; a.nin_split = F;
        a.p_bf16 = f.abf; a.q_bf16 = f.xbf;
        WgradSlab w;
        TRY(wgrad_launch(rq, a, "wgrad_A0_Ar", b.st, &w));
        TRY(rq.push(w.block(0, C, F, dA0, F).colsum(dbpr, 2L * C * F, C)));
        int lo, hi;
        region_range(d, g, &lo, &hi);           // only the owned region blocks have rows here (and are read later)
        return rq.push(w.block(F, C, F, dAall + (long)lo * C * F, F).groups(g.chunk_region, hi - lo, lo, (long)C * F));
    }
    TRY(wgrad_full(rq, "wgrad_A0", L.dh, C, C, b.Xp, F, F, 0, M, L.kchunk_s, L.nchunks_s, dA0, F, dbpr, b.st, f.abf, 0));
    if (g.overlap) {   // one unmasked (C x F) gradient per region: dA_r = ds^T (L~_r x)
        for (int r = 0; r < R; ++r)
            TRY(wgrad_full(rq, "wgrad_Ar", L.dh, C, C, L.LX + (long)r * M * F, F, F, 0, M, L.kchunk_s, L.nchunks_s,
                           dAall + (long)r * C * F, F, nullptr, b.st, f.abf, 0));
        return REGT_OK;
    }
    if (R == 1) return wgrad_full(rq, "wgrad_Ar", L.dh, C, C, L.LX, F, F, 0, M, L.kchunk_s, L.nchunks_s, dAall, F, nullptr, b.st, f.abf, 0);
    // per-region dA_r = sum over the region's rows of ds^T (L~ x), over the region-pure row chunks
    REGT_CHECK_ARG(g.chunk_tab && g.chunk_region && g.n_chunks > 0, "backward: region chunk table missing");
    WgradArgs a{L.dh, C, C, L.LX, F, F, 0, M, 0, g.chunk_tab, g.n_chunks, nullptr, 0};
    a.p_bf16 = f.abf;
    WgradSlab w;
    TRY(wgrad_launch(rq, a, "wgrad_Ar", b.st, &w));
    return rq.push(w.block(0, C, F, dAall, F).groups(g.chunk_region, R, 0, (long)C * F));
}

// One branch per form, each complete in itself: paired (bf16 rows with the ring kernel, see wgrad_paired), collapsed (TemporalGCN,
// FMT_TCOLLAPSE: dzr^T h becomes dzr^T [x | L~ x]) or plain; then the embedding gradients.
static int weight_gradients(const Bwd& b, ReduceQueue& rq) {
    const Layout& L = b.L; const StepForm& f = b.f;
    const int F = b.d.F, C = b.d.C;
    const int pairs_opt = option(OPT_WGRAD_PAIRS);
    const bool pairs = (pairs_opt == 2 ? wgrad_ring_active() : pairs_opt == 1) && f.ibf && f.qbf && f.abf && f.xbf && !b.ext && !f.tcol &&
                       C % 128 == 0 && F % 8 == 0;
    if (pairs) {
        TRY(wgrad_paired(b, rq));
    } else if (f.tcol) {
        TRY(wgrad_Uh(b, rq));
        TRY(wgrad_G(b, rq, "wgrad_Gh", L.dhp, C, L.dGh));
        TRY(wgrad_P01(b, rq));
        TRY(wgrad_G(b, rq, "wgrad_Gzr", L.dzr, 2 * C, L.dGzr));
    } else {
        TRY(wgrad_Uh(b, rq));
        TRY(wgrad_G(b, rq, "wgrad_Gh", L.dhp, C, L.dGh));
        TRY(wgrad_Uzr(b, rq));
        TRY(wgrad_G(b, rq, "wgrad_Gzr", L.dzr, 2 * C, L.dGzr));
    }
    return wgrad_embedding(b, rq);
}

// Back through the weight compositions of compose_forward (tiny; one launch of at most 19 tasks: nothing below reads what another
// task writes -- G0 = dA0 W0^T + db' b_c^T, what EVERY block of d tgnn.linear.weight receives, is summed inside each block's task
// instead of through a buffer).
static int compose_backward(const Bwd& b) {
    const regt_dims& d = b.d; const regt_graph& g = b.g; const regt_params& p = b.p; const regt_grads& gr = b.gr; const Layout& L = b.L;
    const int F = d.F, C = d.C, R = d.R;
    PROF("compose_bwd", b.st);
    SgBatch sb{};
    for (int k = 0; k < 3; ++k) {
        const float* dG = k < 2 ? L.dGzr + (long)k * C * F : L.dGh;
        const float* dc = k < 2 ? L.dczr + (long)k * C : L.dch;
        // dU_k[:, :C] = dG_k V_k^T + dc_k beta_k^T
        add_task(sb, gr.gate_w[k], 2L * C, 1, 0, C, C, 1, nullptr, 0,
                 {term(dG, F, 1, 0, p.conv_lin_w[k], 1, F, 0, F), term(dc, 1, 0, 0, p.conv_bias[k], 0, 1, 0, 1)});
        // dV_k = U_k[:, :C]^T dG_k ; dbeta_k = U_k[:, :C]^T dc_k
        // (stated transposed -- output "rows" j, "columns" i -- so that consecutive lanes walk the CONTIGUOUS index i of the
        // left factor U_k[k, i]; as (i, j) every k-step of a lane group touched lines 2C floats apart)
        add_task(sb, gr.conv_lin_w[k], 1, F, 0, F, C, 1, nullptr, 0, {term(dG, 1, F, 0, p.gate_w[k], 2L * C, 1, 0, C)});
        add_task(sb, gr.conv_bias[k], 1, 0, 0, C, 1, 1, nullptr, 0, {term(p.gate_w[k], 1, 2L * C, 0, dc, 1, 0, 0, C)});
    }
    for (int k = 0; k < 3; ++k)      // du_k = dc_k
        add_task(sb, gr.gate_b[k], 1, 0, 0, C, 1, 1, k < 2 ? L.dczr + (long)k * C : L.dch, 1, {});
    if (b.f.tcol) {
        // back through P0_k = U_k2 W0, P1_k = U_k2 W1, c'_k = c_k + U_k2 b  (k = z, r):
        //   dU_k2 = dP0_k W0^T + dP1_k W1^T + dc_k b^T ;  dW0 += sum_k U_k2^T dP0_k ;  dW1 += sum_k U_k2^T dP1_k ;  db += sum_k U_k2^T dc_k
        // (dW0 / dW1 / db already hold the direct path dh^T x / dh^T L~ x / colsum dh from the slab reduction: added in place;
        // the last three stated transposed -- output "rows" f, "columns" c -- so that lanes walk the contiguous index of U_k2)
        const float* dP0[2] = {L.dP01, L.dP01 + (long)C * 2 * F};
        const float* dP1[2] = {L.dP01 + F, L.dP01 + (long)C * 2 * F + F};
        const float* dc[2] = {L.dczr, L.dczr + C};
        for (int k = 0; k < 2; ++k)
            add_task(sb, gr.gate_w[k] + C, 2L * C, 1, 0, C, C, 1, nullptr, 0,
                     {term(dP0[k], 2L * F, 1, 0, p.cheb_w0, 1, F, 0, F), term(dP1[k], 2L * F, 1, 0, p.cheb_w1, 1, F, 0, F),
                      term(dc[k], 1, 0, 0, p.cheb_bias, 0, 1, 0, 1)});
        add_task(sb, gr.cheb_w0, 1, F, 0, F, C, 1, gr.cheb_w0, 1,
                 {term(dP0[0], 1, 2L * F, 0, p.gate_w[0] + C, 2L * C, 1, 0, C), term(dP0[1], 1, 2L * F, 0, p.gate_w[1] + C, 2L * C, 1, 0, C)}, F);
        add_task(sb, gr.cheb_w1, 1, F, 0, F, C, 1, gr.cheb_w1, 1,
                 {term(dP1[0], 1, 2L * F, 0, p.gate_w[0] + C, 2L * C, 1, 0, C), term(dP1[1], 1, 2L * F, 0, p.gate_w[1] + C, 2L * C, 1, 0, C)}, F);
        add_task(sb, gr.cheb_bias, 1, 0, 0, C, 1, 1, gr.cheb_bias, 1,
                 {term(p.gate_w[0] + C, 1, 2L * C, 0, dc[0], 1, 0, 0, C), term(p.gate_w[1] + C, 1, 2L * C, 0, dc[1], 1, 0, 0, C)});
    }
    if (d.regional) {
        const long RC = (long)R * C;
        int lo, hi;
        region_range(d, g, &lo, &hi);
        // dWl_r = G0 + dA_r W1^T for the owned regions, G0 alone for the others (their rows live on other GPUs);
        // G0 = dA0 W0^T + db' b_c^T (A0 and b' sum over all regions)
        const SgTerm g0a = term(L.dA0, F, 1, 0, p.cheb_w0, 1, F, 0, F), g0b = term(L.dbprime, 1, 0, 0, p.cheb_bias, 0, 1, 0, 1);
        add_task(sb, gr.region_w + (long)lo * C, RC, 1, C, C, C, hi - lo, nullptr, 0,
                 {g0a, g0b, term(L.dAall + (long)lo * C * F, F, 1, (long)C * F, p.cheb_w1, 1, F, 0, F)});
        if (lo > 0) add_task(sb, gr.region_w, RC, 1, C, C, C, lo, nullptr, 0, {g0a, g0b});
        if (hi < R) add_task(sb, gr.region_w + (long)hi * C, RC, 1, C, C, C, R - hi, nullptr, 0, {g0a, g0b});
        // dW0 = S^T dA0 ; dW1 = sum_{owned r} Wl_r^T dA_r ; db_c = S^T db' ; db_l = db'
        // (both stated transposed, see dV_k above: tgnn.linear.weight rows are R*C floats apart)
        add_task(sb, gr.cheb_w0, 1, F, 0, F, C, 1, nullptr, 0, {term(L.dA0, 1, F, 0, L.S, C, 1, 0, C)});
        add_task(sb, gr.cheb_w1, 1, F, 0, F, C, 1, nullptr, 0,
                 {term(L.dAall + (long)lo * C * F, 1, F, (long)C * F, p.region_w + (long)lo * C, RC, 1, C, C, hi - lo, 1)});
        add_task(sb, gr.cheb_bias, 1, 0, 0, C, 1, 1, nullptr, 0, {term(L.S, 1, C, 0, L.dbprime, 1, 0, 0, C)});
        add_task(sb, gr.region_b, 1, 0, 0, C, 1, 1, L.dbprime, 1, {});
    }
    return launch_small_gemm_multi(sb, b.st);
}

// The backward, four stages in this order: head, data gradients of the cell, weight gradients (their slab reductions deferred into ONE
// launch, ReduceQueue), and back through the weight compositions.  No sparse op: A_hat x and L~ x are constants.
// `h_ext` / `dh_ext` != NULL (regt_cell_backward): the hidden input was supplied by the caller; its gradient is
// written to dh_ext and the embedding-stage gradients (A0 / A_r / Cheb weights) are skipped.
int backward_impl(const regt_dims& d, const regt_graph& g, const regt_params& p, const regt_grads& gr,
                  const float* dpred, const float* dhidden, const float* hidden, const float* xp_ext, const Layout& L0,
                  hipStream_t st, int fmt, const float* h_ext, float* dh_ext) {
    const StepForm f = step_form(d, fmt, h_ext != nullptr);
    // REGT_DIMS_NO_HEAD: no head stage; the caller's dhidden IS dOH (every stage below only reads it)
    const bool no_head = (d.flags & REGT_DIMS_NO_HEAD) != 0;
    Layout Lh = L0;
    if (no_head) Lh.dOH = const_cast<float*>(dhidden);
    const Layout& L = Lh;
    const Bwd b{d, g, p, gr, L, f, wb_ptrs(L.Wb, d.C, d.F),
                (xp_ext && (!f.xbf || (fmt & FMT_XCALLER))) ? xp_ext : L.Xp, h_ext ? h_ext : L.h, dh_ext ? dh_ext : L.dh, h_ext != nullptr, st};
    ReduceQueue rq(L.slab, L.slab_floats, st);
    if (!no_head) TRY(head_backward(d, p, gr, dpred, dhidden, hidden, L.y1, L.d1, L.dOH, rq, st));
    TRY(data_gradients(b));
    TRY(weight_gradients(b, rq));
    TRY(rq.flush());      // every slab reduction of this backward pass, one launch
    return compose_backward(b);
}

}  // namespace regt
