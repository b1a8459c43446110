// Host rules of the weight gradients out[Nout x Nin] = P^T Q: the row chunking every launch uses, and which of the kernels of
// wgrad_fp32.hip / wgrad_bf16.hip a gradient runs on, with what grid and dynamic LDS (wgrad_pick).  No kernel lives here
// (tests/op_bars.py::expected_kernel restates the choice; tests/test_wgrad_plan_cpu.py pins it case by case).
#include "wgrad_common.h"

namespace regt {

// Depth of the register ring of wgrad_bf16_ring_kernel: regt_set_option("wgrad_ring", d) = 0 (the one-half-slab-ahead kernel
// wgrad_split_kernel<1, true, true>: same slabs bit for bit) | 4 | 6 (default) | 8 half slabs of lead.
static int wgrad_ring_depth() { return option(OPT_WGRAD_RING); }
static int wgrad_tile_rows() { return option(OPT_WGRAD_TILE); }       // 128 | 256 (default) output rows per tile of the ring kernel
bool wgrad_ring_active() { return wgrad_ring_depth() > 0; }

// One wave of workgroups: `nch` chunks of kc = roundup32(ceil(M / nch)) rows.  Chunks shorter than `min_rows` are refused (small problems
// keep many short chunks: the latency-bound regime); chunks past 32768 rows (the kernels' 32-bit row offsets) become whole waves of
// shorter ones.  false: not applicable, *kchunk / *nchunks keep the caller's chunking.
static bool wave_chunks(long nch, long M, long min_rows, int* kchunk, int* nchunks) {
    if (nch < 1) return false;
    long kc = ((M + nch - 1) / nch + 31) / 32 * 32;
    if (kc < min_rows) return false;
    if (kc > 32768) {
        const long waves = (kc + 32767) / 32768;
        kc = ((M + nch * waves - 1) / (nch * waves) + 31) / 32 * 32;
    }
    *kchunk = (int)kc;
    *nchunks = (int)((M + kc - 1) / kc);
    return true;
}
// Row chunking for a ring-kernel launch whose workgroups are ALL resident at once and fill every slot: chunks x tiles = CUs x
// workgroups per CU.  The tiles of a chunk share their operands through L2 only while they walk the chunk in step; started
// together they do, started as slots free up (1.5 waves of workgroups at 128 chunks x 6 tiles) they do not, and the half-filled
// last wave costs as much as a full one.  Fewer, longer chunks also mean fewer slabs to write and reduce.
// regt_set_option("wgrad_wave", 0): the layout's ~128 chunks.  false: not applicable, keep the caller's chunking.
// (The same switch, under the fp32 arithmetic, turns the wave-owned kernel and its one-chunk-per-CU sizing off -- wgrad_wave_shape
// below: in both arithmetics it means "chunks sized to one wave of resident workgroups", and no launch is reached by both meanings.)
// The same for the wide fp32 / bf16x3 kernels (wgrad3_kernel: three workgroups per CU; wgrad_split_kernel<3>: two): chunks x
// (128 x 128 tiles) = one full wave of workgroups instead of ~128 chunks (768 instead of 1024 / 512 workgroups for dUzr / dUh at
// C = 256).  These kernels are MFMA-bound, so it buys little: -0.05 ms of 4.0 at cfg-3, -0.01 ms at the W = 8 shard shape
// (profiles/r04_wgrad_wave32_ab.txt; two waves mean more slabs to reduce: slower).
bool wgrad_wide_chunking(int Nout, int Nin, long M, int* kchunk, int* nchunks) {
    if (gemm_mode() == 2 || fp32_core_wide() || Nin <= 32) return false;
    if (wgrad_wave_shape(Nout, Nin) && wgrad_wave_chunking(Nout, M, kchunk, nchunks)) return true;
    const int per_cu = gemm_mode() == 1 ? 2 : 3;
    const long tpc = (long)cdiv(Nout, 128) * cdiv(Nin, 128);
    return wave_chunks((long)device_cus() * per_cu / tpc, M, 512, kchunk, nchunks);
}
// The wave-owned kernel (wgrad_wave_kernel: ONE workgroup per CU, each computing a whole 256 x 256 output tile of its row chunk): one
// row chunk per CU, so Nout = 256 is one full wave of workgroups and Nout = 512 two (the two tiles of a chunk run side by side on one
// XCD and share Q through its L2).  Chunks shorter than WG_WAVE_MIN_ROWS are refused: the kernel's prologue (two slabs in flight
// before the first MFMA), its 256 KB slab store per workgroup and the reduction of one slab per CU are paid per chunk whatever its
// length, while wgrad3_kernel's chunking writes and reduces 192 / 96 slabs instead of 256.  The gate is 128 slabs per chunk: the whole
// step is measured at cfg-3's 147 slabs; the kernel alone also wins at 128 and at 64 slabs (138 / 142 and 135 / 141 against 124 / 127
// and 120 / 130 TFLOP/s, profiles/wgrad_wave_ab.txt), but there the added slabs' reduction is not in the figure -- smaller problems
// keep wgrad3_kernel.
// regt_set_option("wgrad_wave", 0): wgrad3_kernel and its chunking.
constexpr long WG_WAVE_MIN_ROWS = 128 * W_BK;
bool wgrad_wave_shape(int Nout, int Nin) { return gemm_mode() == 0 && !fp32_core_wide() && option(OPT_WGRAD_WAVE) && Nin == 256 && Nout > 0 && Nout % 256 == 0; }
// The smallest row count the wave-owned kernel is chosen for: every CU gets a chunk of WG_WAVE_MIN_ROWS rows.  (From there on the
// chunker's rounding of a chunk to whole slabs leaves at most one CU in 64 without a chunk.)
long wgrad_wave_min_rows() { return (long)device_cus() * WG_WAVE_MIN_ROWS; }
bool wgrad_wave_chunking(int Nout, long M, int* kchunk, int* nchunks) {
    (void)Nout;                                    // (every 256-row tile of a chunk is a workgroup of its own: the count does not depend on it)
    return M >= wgrad_wave_min_rows() && wave_chunks(device_cus(), M, WG_WAVE_MIN_ROWS, kchunk, nchunks);
}
// Skinny gradients (Nin <= 32: wgrad_kernel<32>, HBM-bound on their left operand): chunks x row tiles = two
// workgroups per CU, all resident at once -- at cfg-3 the layout's 507 chunks are 1.3 (dGh) / 2.6 (dGzr) waves of workgroups.
bool wgrad_skinny_chunking(int Nout, long M, int* kchunk, int* nchunks) {
    constexpr int per_cu = 2;
    return wave_chunks((long)device_cus() * per_cu / cdiv(Nout, 128), M, 512, kchunk, nchunks);
}
bool wgrad_ring_chunking(int Nout, int Nin, long M, int* kchunk, int* nchunks) {
    if (!wgrad_ring_active() || !option(OPT_WGRAD_WAVE)) return false;
    const bool wide = wgrad_tile_rows() == 256 && Nout % 256 == 0;
    const int per_cu = wide || wgrad_ring_depth() >= 8 ? 2 : 3;           // register-limited workgroups per CU of the variant launched
    const long tpc = (long)cdiv(Nout, wide ? 256 : 128) * cdiv(Nin, 128);
    return wave_chunks((long)device_cus() * per_cu / tpc, M, 512, kchunk, nchunks);
}
// Upper bound of the row chunks ANY of the three per-launch chunkers above can return for a (Nout x Nin) gradient over M rows, whatever
// the arithmetic / switches at launch time: make_layout sizes the slab regions with it (the layout's own ~128 / ~512 chunks were too few
// once the launches started to pick their counts: C = 128 in fp32 asks for 768 chunks of dUh).  The same rule over the three largest
// budgets, with no chunk refused (32 rows is what the rounding gives any M > 0).
long wgrad_chunk_bound(int Nout, int Nin, long M) {
    const long cus = device_cus();
    // (The wave-owned fp32 kernel's one chunk per CU has no candidate here: the workspace stays what it was.  make_layout asks with
    // Nin = C + F, and the regions it sizes for dUh and dUzr together hold the 256 slabs of either launch -- the largest, dUzr's,
    // is 512 x (C C + C) floats against 512 x (C (C + F) + C) reserved, tests/test_wgrad_choice_wave.py.  The slab regions are one
    // pool: when both launches' slabs do not fit beside the rest, ReduceQueue reduces what is queued first.)
    const long cand[3] = {cus * 3 / ((long)cdiv(Nout, 128) * cdiv(Nin, 128)),      // wide fp32 / bf16x3, ring (128-row tiles)
                          cus * 2 / cdiv(Nout, 128),                               // skinny
                          cus * 3 / ((long)cdiv(Nout, 256) * cdiv(Nin, 128))};     // ring (256-row tiles)
    int best = 0;
    for (long nch : cand) {
        int kc = 0, n = 0;
        if (wave_chunks(nch, M, 32, &kc, &n) && n > best) best = n;
    }
    return best;
}
long wgrad_slab_stride(const WgradArgs& a) { return (long)a.Nout * a.Nin + (a.colsum ? a.Nout : 0); }

// Every column tile of a row chunk forms the column sums of P although only tile 0 stores them:
// the tiles of a chunk share P (and Q between row tiles) through their XCD's L2 and only find each other's lines there while they walk
// the chunk in step -- with less work the other tiles run ahead and every tile reads its operands from HBM (measured on the bf16
// ring kernel: 0.90 / 0.51 ms against 0.71 / 0.45 ms for the two paired gradients of the cfg-5 shard).
static int pick_kernel(const WgradArgs& a, WgradPick* p, bool any_rows);
static int launch_picked(const WgradArgs& a, hipStream_t st, bool any_rows, WgradKernel* ran) {
    WgradArgs am = a;
    am.all_csum = a.colsum && a.p_bf16 && a.q_bf16;     // (fp32 kernels: measured no gain, +0.02 ms on the MFMA-bound wgrad3_kernel)
    WgradPick p;
    if (int rc = pick_kernel(am, &p, any_rows)) return rc;
    if (ran) *ran = p.kernel;
    if (int rc = p.kernel < WG_SPLIT3 ? launch_wgrad_fp32(p, am, st) : launch_wgrad_bf16(p, am, st)) return rc;
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}
int launch_wgrad(const WgradArgs& a, hipStream_t st) { return launch_picked(a, st, false, nullptr); }
// The same launch for regt_wgrad_slabs: any_rows lifts the row gate of the wave-owned kernel (the kernel on chunks of a few slabs);
// *ran: the choice
int launch_wgrad_slabs(const WgradArgs& a, hipStream_t st, bool any_rows, WgradKernel* ran) { return launch_picked(a, st, any_rows, ran); }
const char* wgrad_kernel_name(WgradKernel k) {
    static const char* const names[] = {"wgrad_kernel<32>", "wgrad_kernel<32, bf16 P>", "wgrad_kernel<64>", "wgrad_kernel<128>", "wgrad3_kernel",
                                        "wgrad_kernel_generic<32>", "wgrad_kernel_generic<128>", "wgrad_wave_kernel", "wgrad_split_kernel<3>",
                                        "wgrad_split_kernel<1>", "wgrad_split_kernel<1, bf16 Q>", "wgrad_split_kernel<1, bf16 P>",
                                        "wgrad_split_kernel<1, bf16 P, bf16 Q>", "wgrad_bf16_ring_kernel<4, 2>", "wgrad_bf16_ring_kernel<6, 2>",
                                        "wgrad_bf16_ring_kernel<8, 2>", "wgrad_bf16_ring_kernel<2, 4>", "wgrad_bf16_ring_kernel<4, 4>"};
    static_assert(sizeof(names) / sizeof(names[0]) == WG_RING_4_4 + 1, "one name per WgradKernel, in its order");
    return names[k];
}
// The kernel of a weight gradient, its grid and its dynamic LDS; launches nothing and makes every refusal.
int wgrad_pick(const WgradArgs& a, WgradPick* p) { return pick_kernel(a, p, false); }
// any_rows: the wave-owned kernel is not held to its row gate (every CU a chunk of WG_WAVE_MIN_ROWS rows); every other condition stays
static int pick_kernel(const WgradArgs& a, WgradPick* p, bool any_rows) {
    const auto pick = [p](WgradKernel k, long nblocks, size_t bytes, bool raise_lds) { *p = WgradPick{k, nblocks, bytes, raise_lds}; return REGT_OK; };
    // a ring-kernel instantiation: `bytes` of dynamic LDS, raised past the 48 KB any kernel may ask for
    const auto ring_pick = [&](WgradKernel k, long nblocks, size_t bytes) { return pick(k, nblocks, bytes, bytes > 48 * 1024); };
    REGT_CHECK_ARG(a.Nout > 0 && a.Nin > 0 && a.nchunks > 0, "wgrad: empty problem");
    // a two-part right-hand side runs on the skinny fp32 kernel, except under the bf16 arithmetic with Nin <= 128 (one
    // column tile of the bf16-pipe kernel: at F = 64 the fused dA0 / dA_r gradient is fp32-MFMA-bound on the skinny kernel)
    // (any width when both parts are stored as bf16: the fused [q | A_hat x] / [h | A_hat x] gradients of the bf16-row layout)
    const bool q2_split = a.Q2 && gemm_mode() == 2 && a.Nin > 32 && (a.Nin <= 128 || a.q_bf16) && !a.q_relu && a.nin_split % (a.q_bf16 ? 8 : 4) == 0 &&
                          !fp32_core_wide() && (!a.q_bf16 || a.ldq2 % 8 == 0);
    // (a bf16-stored right-hand side of width <= 32 -- A_hat x rows at F = 32 -- also takes the bf16-pipe kernel: the skinny one
    // stages fp32 rows only; the stage is HBM-bound on its left operand either way)
    const bool wide = (a.Nin > 32 || (a.q_bf16 && gemm_mode() == 2 && !a.Q2)) && (!a.Q2 || q2_split);
    const bool fast = a.ldp % 4 == 0 && a.ldq % 4 == 0 && a.Nout % 4 == 0 && a.Nin % 4 == 0 && a16(a.P) && a16(a.Q) &&
                      a.ldp < (1L << 20) && a.ldq < (1L << 20) && (a.chunk_tab || a.kchunk <= 65536) &&
                      (!a.Q2 || (a.ldq2 % 4 == 0 && a.ldq2 < (1L << 20) && a16(a.Q2) && a.nin_split % 32 == 0));
    // (fp32 rows, 32 < Nin <= 64 -- the fused [x | L~ x] right-hand side at F = 32: one 64-column tile; regt_set_option("wgrad_bnw64", 0): two of 32)
    const int bnw64 = option(OPT_WGRAD_BNW64);
    const bool mid = !wide && fast && bnw64 && !a.p_bf16 && !a.q_bf16 && a.Nin > 32 && a.Nin <= 64 && (!a.Q2 || a.nin_split < 64);
    const int bnw = wide ? 128 : (mid ? 64 : 32);
    long blocks = (long)cdiv(a.Nout, 128) * cdiv(a.Nin, bnw) * a.nchunks;
    REGT_CHECK_ARG(blocks < (1L << 31), "wgrad: too many blocks");
    size_t lds = 2 * (size_t)(W_BK * W_LDP + W_BK * (bnw + 4)) * 4;
    REGT_CHECK_ARG(!a.Q2 || fast, "wgrad: a second right-hand operand needs 16-byte tileable operands and nin_split %% 32 == 0");
    REGT_CHECK_ARG(!(a.p_bf16 || a.q_bf16) || fast, "wgrad: bf16 operands need the vector kernels");
    if (wide) {
        if (fast && gemm_mode() == 1) return pick(WG_SPLIT3, blocks, 4 * 3 * WS_PLANE_B, true);
        if (fast && gemm_mode() == 2) {
            REGT_CHECK_ARG(!(a.p_bf16 || a.q_bf16) || (a.Nout % 8 == 0 && a.Nin % 8 == 0 && a.ldp % 8 == 0 && a.ldq % 8 == 0 && !a.q_relu),
                           "wgrad: bf16-stored operands need 8-element aligned rows");
            const size_t lb = 4 * 1 * WS_PLANE_B;
            const int ring = wgrad_ring_depth();
            // (the ring kernel's descriptors end with the chunk: chunk rows x row bytes must stay below 2^31)
            const long ld_max = std::max(a.ldp, std::max(a.ldq, a.Q2 ? a.ldq2 : 0L));
            const long rows_max = a.chunk_tab ? a.M : (long)a.kchunk + 32;
            const bool ring_ok = a.p_bf16 && a.q_bf16 && ring > 0 && (!a.Q2 || a.nin_split % 128 == 0) && 2 * rows_max * ld_max < (1L << 31);
            // 256-row tiles where the output has them (regt_set_option("wgrad_tile", 128 | 256)); ring of 2 there
            // ("wgrad_ring256" = 2 | 4; 6 half slabs of three 16-byte loads spill).  Two beats four, 0.585 + 0.350
            // against 0.63 + 0.383 ms at the cfg-5 shard: what is in flight (workgroups x slots x 12 KB per XCD) competes with the lines
            // the chunk's other tiles are about to ask for in the 4 MiB L2, and the tile that comes second finds its rows there anyway
            if (ring_ok && wgrad_tile_rows() == 256 && a.Nout % 256 == 0) {
                const long blocks4 = (long)(a.Nout / 256) * cdiv(a.Nin, 128) * a.nchunks;
                return ring_pick(option(OPT_WGRAD_RING256) == 2 ? WG_RING_2_4 : WG_RING_4_4, blocks4, 2 * 3 * WS_PLANE_B);
            }
            if (ring_ok) return ring_pick(ring >= 8 ? WG_RING_8_2 : (ring >= 6 ? WG_RING_6_2 : WG_RING_4_2), blocks, lb);
            return pick((WgradKernel)(WG_SPLIT1 + 2 * (a.p_bf16 != 0) + (a.q_bf16 != 0)), blocks, lb, false);
        }
        if (fast && !fp32_core_wide()) {
            REGT_CHECK_ARG(!(a.p_bf16 || a.q_bf16), "wgrad: bf16-stored operands with the fp32 kernel");
            // one wave per SIMD owning a 128 x 128 block: 256-column right-hand sides, whole 256-row output tiles, and enough rows that
            // every CU has a chunk of WG_WAVE_MIN_ROWS, in chunks as wgrad_wave_chunking sizes them (workgroups for 7 of 8 CUs at
            // least, no chunk count that leaves the chunks short).  Its scalar row offsets run up to 28 rows into the second slab past
            // a chunk's last, ragged one: (chunk rows + 96) x row bytes must stay below 2^31.
            const long rows_max = a.chunk_tab ? a.M : (long)a.kchunk;
            const bool wave_rows = a.M >= wgrad_wave_min_rows() && 8L * a.nchunks * (a.Nout / 256) >= 7L * device_cus() &&
                                   2 * a.M >= (long)a.nchunks * WG_WAVE_MIN_ROWS;
            if (wgrad_wave_shape(a.Nout, a.Nin) && !a.q_relu && (any_rows || wave_rows) && 4 * (rows_max + 96) * std::max(a.ldp, a.ldq) < (1L << 31))
                return pick(WG_WAVE, (long)(a.Nout / 256) * a.nchunks, 2 * 2 * W_BK * (256 + 4) * 4, true);
            return pick(WG_WIDE3, blocks, 4 * 16 * 132 * 4, false);
        }
        if (fast) {
            REGT_CHECK_ARG(!(a.p_bf16 || a.q_bf16), "wgrad: bf16-stored operands with the fp32 wide kernel");
            return pick(WG_WIDE128, blocks, lds, true);
        }
        return pick(WG_GENERIC128, blocks, lds, true);
    }
    if (fast) {
        REGT_CHECK_ARG(!a.q_bf16 && (!a.p_bf16 || (a.Nout % 8 == 0 && a.ldp % 8 == 0)), "wgrad: skinny kernel takes a bf16-stored P only");
        if (a.p_bf16) return pick(WG_SKINNY32_PBF, blocks, lds, false);
        return mid ? pick(WG_MID64, blocks, lds, true) : pick(WG_SKINNY32, blocks, lds, false);
    }
    return pick(WG_GENERIC32, blocks, lds, false);
}

}  // namespace regt
