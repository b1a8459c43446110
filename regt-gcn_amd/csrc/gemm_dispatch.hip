// Host rules of the dense contractions: which arithmetic, which core and which K-loop form a GEMM of given segments runs on.
// No kernel lives here; the launchers of gemm_flat.h and gemm_cell.hip ask these predicates
// (tests/op_bars.py::expected_kernel restates them).
#include "gemm_flat.h"

namespace regt {

// 0: fp32 MFMA (default).  1: exact 3-way bf16 split of both operands, six partial products on the bf16 matrix pipe
// (gemm_split.h) for the GEMMs whose B operand is stored [N][K].  2: plain bf16 operands (one product), fp32 accumulate --
// reduced precision, the arithmetic BASELINE configs[4] names.  The process default is OPT_GEMM_MODE (REGT_GEMM_MODE, regt_set_gemm_mode).
// per-call override (regt_dims.arith, set for the duration of one entry point on the calling thread by CallScope): two models of
// one process can run different arithmetics without touching the process default
static thread_local int t_gemm_mode = -1;
int gemm_mode_override(int mode) { const int prev = t_gemm_mode; t_gemm_mode = mode; return prev; }
int gemm_mode() { return t_gemm_mode >= 0 ? t_gemm_mode : option(OPT_GEMM_MODE); }
// REGT_FP32_CORE=wide: fp32 GEMMs on the 2-workgroup-per-CU core (gemm_fast.h) instead of the 3-workgroup one, for A/B timing
bool fp32_core_wide() { return option(OPT_FP32_CORE) == 1; }

int gemm_tiles(long M, int N, int bm, int bn, long* tiles) {
    *tiles = (long)cdiv(M, bm) * cdiv(N, bn);
    REGT_CHECK_ARG(*tiles < (1L << 31), "gemm: too many tiles");
    return REGT_OK;
}

// the K loop may keep its slab descriptors in scalar registers (SplitCore::run_u): every K a multiple of the 32-k slab, byte offsets of a tile's rows within 31 bits.  REGT_GEMM_DESC=table forces the LDS table.
bool gemm_desc_table_forced() { return option(OPT_GEMM_DESC) == 1; }
int uniform_ok(const GemmSegs& S, long M) {
    if (gemm_desc_table_forced()) return 0;
    int frag = 0;
    long slabs = 0;
    for (int s = 0; s < S.nseg; ++s) {
        const GemmSeg& g = S.seg[s];
        if (g.K % GBK != 0 || g.K <= 0) return 0;
        if ((g.flags & SEG_REGION) && (g.flags & SEG_A_BF16)) return 0;       // bf16 rows are never region-masked
        if (g.lda * 4 * (GBM + 1) >= (1L << 31) || g.ldb * 4 * (GBN + 1) >= (1L << 31)) return 0;
        if (g.flags & SEG_B_FRAG) ++frag;
        // the bf16-operand core keeps the tile's slab descriptors in LDS, 64 at most (SplitCore::plan_u)
        const long reps = (g.flags & SEG_REGION) ? std::min<long>(S.num_regions > 0 ? S.num_regions : 1, GBM / (S.row_div > 0 ? S.row_div : 1) + 2)
                                                 : ((g.flags & SEG_REPEAT) ? g.nrep : 1);
        slabs += reps * (g.K / GBK);
    }
    if (gemm_mode() == 2 && slabs > 64) return 0;
    (void)M;
    if (frag == 0) return 1;
    return frag == S.nseg && gemm_mode() == 2 ? 2 : 0;
}

int fast_class(const GemmSegs& S, int N, bool vec) {
    if (!vec || N % 4 != 0 || S.nseg < 1) return -1;
    int bt = -1, region = 0, relu = 0;
    long iters = 0;
    for (int s = 0; s < S.nseg; ++s) {
        const GemmSeg& g = S.seg[s];
        if (!(g.flags & SEG_VEC_A) || !(g.flags & SEG_VEC_B) || g.K % 4 != 0) return -1;
        // only the bf16-operand core reads bf16 rows: 16-byte loads of 8 k, never region-masked
        if ((g.flags & SEG_A_BF16) && (gemm_mode() != 2 || !(g.flags & SEG_BT) || g.K % 8 != 0 || g.lda % 8 != 0 ||
                                       (g.flags & (SEG_REGION | SEG_REPEAT | SEG_RELU_A)))) return -1;
        const int b = (g.flags & SEG_BT) ? 1 : 0;
        if (bt >= 0 && bt != b) return -1;
        bt = b;
        if (g.flags & SEG_REGION) region = 1;
        if (g.flags & SEG_RELU_A) relu = 1;
        if (b && g.nsplit < N && g.nsplit % GBN != 0) return -1;      // a column tile must not straddle B0 | B1
        if (g.lda >= (1L << 22) || g.ldb >= (1L << 22)) return -1;    // 32-bit byte offsets inside a tile
        if ((g.flags & SEG_REPEAT) && g.a_rep_stride % 4 != 0) return -1;
        // worst case of a region-masked segment: every node of a row tile lies in another region (node ids not sorted by
        // region) -- a 128-row tile of node-major rows meets at most 128 / row_div + 2 nodes; never more than all regions
        long reps = 1;
        if (g.flags & SEG_REGION) {
            const long by_rows = GBM / (S.row_div > 0 ? S.row_div : 1) + 2;
            reps = S.num_regions > 0 ? S.num_regions : 1;
            if (by_rows < reps) reps = by_rows;
        } else if (g.flags & SEG_REPEAT) {
            reps = g.nrep;
        }
        iters += (long)cdiv(g.K, GBK) * reps;
    }
    if (relu && S.nseg != 1) return -1;
    if (iters > G_MAX_ITERS) return -1;
    return bt | (region << 1) | (relu << 2);
}

// REGT_DGRAD1_GEN=0: keep cell_bwd + dgrad_candidate as two launches (A/B timing; same dhp / dzp / drp / dh to the bit, the
// attention gradient in another fixed summation order)
static bool dgrad1_gen_wanted() { return option(OPT_DGRAD1_GEN) != 0; }
bool gemm_dgrad1_gen_ok(long M, int C, int num_nodes) {
    return dgrad1_gen_wanted() && (gemm_mode() == 0 || gemm_mode() == 1) && !fp32_core_wide() && !gemm_desc_table_forced() && C % GBN == 0 && C % GBK == 0 &&
           (long)cdiv(M, GBM) * (C / GBN) >= SMALL_TILE_LIMIT && M < (1L << 31) && (long)num_nodes * C * 4 < (1L << 31) &&
           (long)C * 8 * (GBM + 1) < (1L << 31);
}

}  // namespace regt
