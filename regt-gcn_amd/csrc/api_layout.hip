// Workspace layouts of the step and of the zero-hidden cell, and the sizing functions: a layout made with base == NULL is its own size.
#include "api_internal.h"

namespace regt {

namespace {
// bump allocator of the layouts: 256-byte aligned pieces of `base` (NULL: sizes only), counted in floats unless asked in bytes
struct Arena {
    char* base;
    size_t off = 0;
    float* bytes(size_t nbytes) {
        size_t o = off;
        off += (nbytes + 255) & ~size_t(255);
        return base ? reinterpret_cast<float*>(base + o) : nullptr;
    }
    float* operator()(long nfloats) { return bytes((size_t)nfloats * 4); }
};
// bf16 copies of the GEMM weights in MFMA fragment order (REGT_GEMM_MODE=bf16, weights_frag()): Uz, Ur, Uh, UT x 3 (C x C
// each), Gzr (2C x F), Gh (C x F), A0 (C x F), A_r (R x (C x F)); rows padded to 128 -- sized in floats; the blocks of wb_ptrs
long wb_floats(long C, long F, long R) { return (6 * frag_bytes(C, C) + frag_bytes(2 * C, F) + (2 + R) * frag_bytes(C, F)) / 4 + 64; }
}  // namespace

WbPtrs wb_ptrs(const float* Wb, long C, long F) {
    const char* b = reinterpret_cast<const char*>(Wb);
    WbPtrs w;
    long o = 0;
    for (int k = 0; k < 3; ++k) { w.U[k] = reinterpret_cast<const float*>(b + o); o += frag_bytes(C, C); }
    for (int k = 0; k < 3; ++k) { w.UT[k] = reinterpret_cast<const float*>(b + o); o += frag_bytes(C, C); }
    w.Gzr = reinterpret_cast<const float*>(b + o); o += frag_bytes(2 * C, F);
    w.Gh = reinterpret_cast<const float*>(b + o); o += frag_bytes(C, F);
    w.A0 = reinterpret_cast<const float*>(b + o); o += frag_bytes(C, F);
    w.Aall = reinterpret_cast<const float*>(b + o);
    w.ar_stride = frag_bytes(C, F);
    return w;
}

// Row chunks of the head's two weight gradients (N rows -- nodes, not node x period rows).  Rounds 1-4 gave both max(512, N / 64)-row
// chunks: 64 workgroups for dW2 (a latency-bound serial walk: 199 us for 51 MB at cfg-3) and 128 for dW1 -- and at one region per
// GPU (12 500 rows) 25 chunks, fewer workgroups than at twice the rows.  Now: dW2 ~1000 chunks of >= 64 rows (its slabs are O x H1
// floats), dW1 ~three workgroups per CU with >= 128 rows per chunk (its slabs are H1 x C floats: more chunks = more slab traffic).
HeadChunks head_chunks(long N, int H1, int C) {
    HeadChunks h;
    long k2 = ((N + 1023) / 1024 + 7) / 8 * 8;
    if (k2 < 64) k2 = 64;
    h.k2 = (int)k2; h.n2 = (int)((N + k2 - 1) / k2);
    const long tiles = (long)((H1 + 127) / 128) * ((C + 127) / 128), want = 768 / (tiles > 0 ? tiles : 1);
    long k1 = ((N + want - 1) / (want > 0 ? want : 1) + 31) / 32 * 32;
    if (k1 < 128) k1 = 128;
    h.k1 = (int)k1; h.n1 = (int)((N + k1 - 1) / k1);
    return h;
}

Layout make_layout(const regt_dims& d, int n_chunks_tab, int overlap, char* base) {
    Layout L{};
    const long N = d.N, T = d.T, F = d.F, C = d.C, R = d.R, O = d.O, H1 = d.H1;
    const long M = N * T;
    Arena take{base};
    L.Xp = take(M * F);
    L.AX = take((overlap ? 1 + R : 2) * M * F);      // A_hat x, then L~ x (merged) or one L~_r x per region
    L.LX = L.AX ? L.AX + M * F : nullptr;
    L.h = take(M * C);
    L.ZR = take(M * 2 * C);
    L.q = take(M * C);
    L.Ht = take(M * C);
    L.y1 = take(N * H1);
    L.probs = take(T);
    L.S = take(C * C);
    take(C * C);      // (C, C) no longer used by the backward: reserved so that no offset moves
    L.A0 = take(C * F);
    L.Aall = take(R * C * F);
    L.bprime = take(C);
    L.Gzr = take(2 * C * F);
    L.Gh = take(C * F);
    L.czr = take(2 * C);
    L.ch = take(C);
    L.P0zr = take(2 * C * F);
    L.P1zr = take(2 * C * F);
    L.czr2 = take(2 * C);
    L.dP01 = take(2 * C * 2 * F);
    L.UT = take(3 * C * C);
    L.Wb = take(wb_floats(C, F, R));
    L.dOH = take(N * C);
    L.d1 = take(N * H1);
    L.dhp = take(M * C);
    L.dzr = take(M * 2 * C);
    L.dh = take(M * C);
    long kc = ((M + 127) / 128 + 31) / 32 * 32;     // ~128 row chunks: 512-1024 wgrad workgroups, half the slab traffic of 256
    if (kc < 128) kc = 128;                          // small graphs: short K loops in many workgroups (latency-bound regime)
    L.kchunk = (int)kc;
    L.nchunks = (int)((M + kc - 1) / kc);
    long ks = ((M + 511) / 512 + 31) / 32 * 32;     // skinny (C x F) gradients: memory-bound, want >= 1024 small workgroups
                                                    // (dGh / dGzr on fp32 rows pick their own count per launch: wgrad_skinny_chunking)
    if (ks < 128) ks = 128;
    L.kchunk_s = (int)ks;
    L.nchunks_s = (int)((M + ks - 1) / ks);
    L.cb_npb = (int)((N + 2047) / 2048);
    L.cb_npb = (L.cb_npb + 3) / 4 * 4;
    L.cb_blocks = cell_bwd_blocks((int)N, L.cb_npb);
    L.dp_partial = take((long)L.cb_blocks * T);
    // per-row <dOH, H'>: one float per row (fused backward kernel, fused.hip) or one partial dot per 128-column tile of the row
    // (fp32 candidate data gradient with a generated left operand, gemm_dgrad1_gen_kernel)
    L.rowdot = take(M * (C / 128 > 1 ? C / 128 : 1));
    L.tile_ctr = reinterpret_cast<unsigned*>(take(16));      // tile counter of the persistent fused kernels (fused.hip, fused_rows.hip)
    // one slab region per weight gradient (their reductions are deferred into one launch, ReduceQueue): the sum of
    // Uh, Uzr (wide), Gh, Gzr, A0, A_r (skinny), head1, head2 -- 64 floats of slack each for alignment
    // (chunk counts: the launches pick their own -- wgrad_wide / _skinny / _ring_chunking -- so every region is sized for the larger of
    // the layout's count and what those can return; the paired bf16 launches write (C + F)-wide slabs)
    auto nmax = [&](long layout_chunks, int nout, int nin) { const long b = wgrad_chunk_bound(nout, nin, M); return b > layout_chunks ? b : layout_chunks; };
    long slab = nmax(L.nchunks, C, C + F) * ((long)C * (C + F) + C) + nmax(L.nchunks, 2 * C, C + F) * (2L * C * (C + F) + 2 * C)
              + nmax(L.nchunks_s, C, F) * (C * F) + nmax(L.nchunks_s, 2 * C, F) * (2 * C * F) + (long)L.nchunks_s * (C * F + C)
              + (long)head_chunks(N, (int)H1, (int)C).n1 * (H1 * C + H1 + O * H1 + O) + (long)head_chunks(N, (int)H1, (int)C).n2 * (O * H1 + O) + 8 * 64
              + nmax(L.nchunks_s, 2 * C, 2 * F) * (2 * C * 2 * F + 2 * C) + 64;   // FMT_TCOLLAPSE: dzr^T [x | L~ x] (one or two launches)
    const long ar_uniform = (long)L.nchunks_s * C * F, ar_tab = (long)(n_chunks_tab > 0 ? n_chunks_tab : 1) * C * F;
    slab += ar_tab > ar_uniform ? ar_tab : ar_uniform;
    slab += (long)(n_chunks_tab > 0 ? n_chunks_tab : 1) * (C * F + C);     // fused dA0 | dA_r slabs over the region chunk table
    L.slab_floats = slab;
    L.slab = take(slab);
    L.dA0 = take(C * F);
    L.dAall = take(R * C * F);
    L.dbprime = take(C);
    L.dGzr = take(2 * C * F);
    L.dGh = take(C * F);
    L.dczr = take(2 * C);
    L.dch = take(C);
    L.bytes = take.off;
    return L;
}

// Workspace of a forward-only call (REGT_DIMS_FORWARD_ONLY, regt_forward_only_workspace_bytes): what the forward itself reads back,
// nothing that only the backward reads, none of the backward's temporaries.
//   fused (the FMT_XBF form: fused_fwd_kernel / fused_fwd_rows_kernel): NO M x C array -- h and q cross LDS / registers, Z stays in
//     registers.  bf16 rows of A_hat x and L~ x, y1, the composed weights and their fragment-order copies, the tile counter, and
//     LAST the bf16 copy of the packed input (x_rows rows: a region shard's halo rows lengthen the workspace at its end; not used
//     when the caller's bf16 buffer is read in place).
//   every other form: h, [Z | R] with its (M, 2C) leading dimension -- the R half is never written --, q: four M x C element arrays
//     (the gate kernel reads h, the candidate kernel q, Z and h); no H~.  A width-C array for Z would save one more, at the price of
//     a second leading dimension in the gate and candidate epilogues' address arithmetic, which the training kernels share.
Layout make_layout_fwd(const regt_dims& d, int overlap, bool fused, long x_rows, char* base) {
    Layout L{};
    const long N = d.N, T = d.T, F = d.F, C = d.C, R = d.R, H1 = d.H1;
    const long M = N * T;
    Arena take{base};
    if (fused) {
        L.AX = take.bytes((size_t)M * F * 2);
        L.LX = take.bytes((size_t)M * F * 2);
    } else {
        L.Xp = take(M * F);
        L.AX = take((overlap ? 1 + R : 2) * M * F);
        L.LX = L.AX ? L.AX + M * F : nullptr;
        L.h = take(M * C);
        L.ZR = take(M * 2 * C);
        L.q = take(M * C);
    }
    L.y1 = take(N * H1);
    L.probs = take(T);
    L.S = take(C * C);
    L.A0 = take(C * F);
    L.Aall = take(R * C * F);
    L.bprime = take(C);
    L.Gzr = take(2 * C * F);
    L.Gh = take(C * F);
    L.czr = take(2 * C);
    L.ch = take(C);
    if (!fused) {
        L.P0zr = take(2 * C * F);
        L.P1zr = take(2 * C * F);
        L.czr2 = take(2 * C);
    }
    L.Wb = take(wb_floats(C, F, R));
    L.tile_ctr = reinterpret_cast<unsigned*>(take(16));
    if (fused) L.Xp = take.bytes((size_t)(x_rows > N ? x_rows : N) * T * F * 2);
    L.bytes = take.off;
    return L;
}

// Form and layout of a forward-only call: the ONE rule of the sizing functions and of forward_common.  `packed`: the caller hands in
// x_rows packed rows (regt_forward_packed / _packed_bf16).  The form is the training forward's for the same call (xbf_ok with the
// same x_rows and row type), so the flag never changes which kernels' arithmetic runs.  The fused form converts packed fp32 rows into
// the workspace, all x_rows of them (make_layout_fwd puts them last); every other case sizes Xp for the N own rows.
Layout forward_only_layout(const regt_dims& d, const regt_graph& g, bool packed, int x_rows, bool xp_is_bf16, char* base, int* fmt) {
    *fmt = forward_format(d, g, packed ? x_rows : d.N, packed && !xp_is_bf16, xp_is_bf16);
    const bool conv = (*fmt & FMT_XBF) && !(*fmt & FMT_XCALLER) && packed;
    return make_layout_fwd(d, g.overlap, (*fmt & FMT_XBF) != 0, conv ? x_rows : d.N, base);
}

Layout0 make_layout0(const regt_dims& d, int kz, int kh, char* base) {
    Layout0 L{};
    const long N = d.N, T = d.T, C = d.C, O = d.O, H1 = d.H1, M = N * T;
    Arena take{base};
    L.Z = take(M * C); L.Ht = take(M * C); L.y1 = take(N * H1); L.probs = take(T);
    L.dOH = take(N * C); L.d1 = take(N * H1); L.dzp = take(M * C); L.dhp = take(M * C);
    long ks = ((M + 511) / 512 + 31) / 32 * 32;           // skinny (C x k) gradients: memory-bound, many small workgroups
    if (ks < 128) ks = 128;
    L.kchunk = (int)ks; L.nchunks = (int)((M + ks - 1) / ks);
    L.cb_npb = (int)((N + 2047) / 2048);
    L.cb_npb = (L.cb_npb + 3) / 4 * 4;
    L.cb_blocks = cell_bwd_blocks((int)N, L.cb_npb);
    L.dp_partial = take((long)L.cb_blocks * T);
    L.slab_floats = (long)L.nchunks * (C * kz + C) + (long)L.nchunks * (C * kh + C) + (long)head_chunks(N, (int)H1, (int)C).n1 * (H1 * C + H1 + O * H1 + O) + (long)head_chunks(N, (int)H1, (int)C).n2 * (O * H1 + O) + 8 * 64;
    L.slab = take(L.slab_floats);
    L.bytes = take.off;
    return L;
}

int check_dims(const regt_dims* d) {
    REGT_CHECK_ARG(d != nullptr, "dims is NULL");
    REGT_CHECK_ARG(d->N > 0 && d->T > 0 && d->F > 0 && d->C > 0 && d->R > 0 && d->O > 0 && d->H1 > 0,
                   "dims: all of N,T,F,C,R,O,H1 must be positive (N=%d T=%d F=%d C=%d R=%d O=%d H1=%d)", d->N, d->T,
                   d->F, d->C, d->R, d->O, d->H1);
    REGT_CHECK_ARG(d->F % 4 == 0, "dims: F=%d must be a multiple of 4 (16-byte feature rows)", d->F);
    REGT_CHECK_ARG(d->C % 4 == 0, "dims: C=%d must be a multiple of 4", d->C);
    // (T <= 64: every element of the hidden state is the sum of at most two partial sums -- bit-reproducible; beyond that a node
    // spans three or more 64-row blocks and the order of the float atomics shows in the last bits)
    REGT_CHECK_ARG(d->T <= 255, "dims: T=%d exceeds 255 periods", d->T);
    REGT_CHECK_ARG((long)d->N * d->T < (1L << 31), "dims: N*T too large");
    REGT_CHECK_ARG(d->arith >= REGT_ARITH_DEFAULT && d->arith <= REGT_ARITH_BF16, "dims: arith=%d is not one of REGT_ARITH_*", d->arith);
    return REGT_OK;
}

}  // namespace regt

using namespace regt;

extern "C" {

size_t regt_workspace_bytes(const regt_dims* dims, int32_t n_chunks, int32_t overlap) {
    if (check_dims(dims)) return 0;
    return make_layout(*dims, n_chunks, overlap, nullptr).bytes;
}

size_t regt_forward_only_workspace_bytes(const regt_dims* dims, const regt_graph* graph) {
    if (check_dims(dims)) return 0;
    if (!graph) { set_error("regt_forward_only_workspace_bytes: graph is NULL"); return 0; }
    CallScope call(dims);
    int fmt;
    return forward_only_layout(*dims, *graph, false, dims->N, false, nullptr, &fmt).bytes;
}

size_t regt_forward_only_packed_workspace_bytes(const regt_dims* dims, const regt_graph* graph, int32_t x_rows, int32_t x_is_bf16) {
    if (check_dims(dims)) return 0;
    if (!graph) { set_error("regt_forward_only_packed_workspace_bytes: graph is NULL"); return 0; }
    if (x_rows < dims->N) { set_error("regt_forward_only_packed_workspace_bytes: x_rows=%d < N=%d", x_rows, dims->N); return 0; }
    CallScope call(dims);
    int fmt;
    const size_t bytes = forward_only_layout(*dims, *graph, true, x_rows, x_is_bf16 != 0, nullptr, &fmt).bytes;
    if (x_is_bf16 && !(fmt & FMT_XBF)) {
        set_error("regt_forward_only_packed_workspace_bytes: bf16 input rows need bf16 arithmetic and a shape the fused forward covers");
        return 0;
    }
    return bytes;
}

size_t regt_cell0_workspace_bytes(const regt_dims* dims, int32_t kz, int32_t kh) {
    if (!dims || dims->N <= 0 || dims->T <= 0 || dims->C <= 0 || dims->O <= 0 || dims->H1 <= 0 || kz <= 0 || kh <= 0) return 0;
    return make_layout0(*dims, kz, kh, nullptr).bytes;
}

}  // extern "C"
