// Which aggregation kernel runs: spmm_pick states the choice of the three forms (one operator, merged two-weight operator on fp32
// rows, on bf16 rows) once, side by side, and makes every refusal; the public launchers pick and then launch what was picked
// (spmm_csr.hip, spmm_panel.hip).  Host code only.  tests/op_bars.py::expected_kernel restates the choice in Python;
// tests/test_spmm_plan_cpu.py pins both, case by case, against a record taken from the one file this used to be.
#include "spmm_common.h"

namespace regt {

// An X up to this size lives in the eight 4 MiB L2s anyway: lane groups over whole rows, no panel schedule
constexpr long SP_L2_RESIDENT_BYTES = 24L << 20;
// 256-byte panels (half the passes over the CSR, 16 lanes per row) while an XCD's slice of X (chunk x 256 B) stays NEAR its 4 MiB L2:
// measured faster up to a 4.0 MB slice (cfg-5 shard, 15 625 nodes per XCD: 0.27 vs 0.38 ms with 128-byte panels, round 3; the
// round-1 limit of 3.7 MB was a guess that left this case on 128-byte panels)
constexpr long SP_WIDE_SLICE_MAX = 9L << 19;     // 4.7 MB
// 256-byte column panels (two cache lines per neighbour: half the passes over the CSR) while an XCD's slice of X (node chunk x 256 B)
// stays around its 4 MiB L2, else 128-byte ones; REGT_SPMM_PL=8|16 forces one (tools/spmm_pmc.sh)
static bool panel_wide(int nnodes) {
    const int pl = option(OPT_SPMM_PL);
    return pl ? pl == 16 : (long)cdiv(nnodes, 8) * 256 <= SP_WIDE_SLICE_MAX;
}
// lanes per row: a wide panel (also a forced one) still needs rows of whole 256-byte panels
static int panel_lanes(int nnodes, bool whole_wide_panels) { return panel_wide(nnodes) && whole_wide_panels ? 16 : 8; }

// ---- the row-block kernel: eligibility and the rows-per-group choice ------------------------------------------------------------
// LDS entries per workgroup (16 B each, behind the 260-int row pointer slice): what 8 (fp32 rows, 64 VGPRs) or 5 (bf16 rows, 84 VGPRs)
// resident workgroups per CU leave each of them
static int rows_cap(bool bf) { return (163840 / (bf ? 5 : 8) - 260 * 4 - 64) / 16; }
static int rows_rpg(int nnodes, int PL, bool bf) {
    const int chunk = cdiv(nnodes, 8), groups = 256 / PL;
    int rpg = cdiv(chunk, groups * (bf ? 150 : 240));     // all workgroups of an XCD resident at once: 32 CUs x 8 (5) workgroups, some slack
    if (rpg < 1) rpg = 1;
    return rpg;
}
// REGT_SPMM_ROWS / regt_set_option("spmm_rows"): 1 = row-block kernel where eligible, 0 (default) = panel kernels
static bool rows_wanted() { return option(OPT_SPMM_ROWS) != 0; }
// at most 256 rows per workgroup: the row pointer slice in LDS holds 256 rows
static bool rows_fit(int nnodes, int PL, bool bf) { return (256 / PL) * rows_rpg(nnodes, PL, bf) <= 256; }
// eligible (fp32 rows): rows are whole panels, every byte offset fits 32 bits, at most 256 rows per workgroup
static bool rows_ok(int nnodes, long x_rows, long rowbytes, int PL) {
    return rows_wanted() && rowbytes % (PL * 16) == 0 && x_rows * rowbytes < (1L << 32) - 4096 && (long)nnodes * rowbytes < (1L << 32) - 4096 &&
           rows_fit(nnodes, PL, false);
}

static void plan_rows(SpmmPlan& k, long x_rows, int rowbytes) {
    k.family = SP_ROWS;
    k.rowbytes = rowbytes;
    k.npanels = rowbytes / (k.PL * 16);
    k.rpg = rows_rpg(k.nnodes, k.PL, k.bf);
    k.cap = rows_cap(k.bf);
    k.nrb = cdiv(cdiv(k.nnodes, 8), (256 / k.PL) * k.rpg);
    k.grid = 8L * k.nrb;
    k.x_bytes = (unsigned)(x_rows * rowbytes);
    k.y_bytes = (unsigned)((long)k.nnodes * rowbytes);
    k.lds = k.cap * 16 + 260 * 4;
}
// eight XCD node chunks x panels x operators x blocks of 256 / PL rows
static void plan_panel(SpmmPlan& k) {
    k.family = SP_PANEL;
    k.npanels = k.W16 / k.PL;
    k.nrb = cdiv(cdiv(k.nnodes, 8), 256 / k.PL);
    k.grid = 8L * k.npanels * k.nstack * k.nrb;
}
// one lane group per row: the first rung that holds W4 float4 (the caller has seen to W4 <= 512, the last rung of both ladders)
static void plan_csr(SpmmPlan& k, int W4) {
    const SpLadder ladder = spmm_ladder(k.dual);
    int r = 0;
    while (r + 1 < ladder.n && W4 > ladder.rungs[r].max_w4) ++r;
    k.family = SP_CSR;
    k.rung = &ladder.rungs[r];
    const int groups = 256 / k.rung->G;
    k.grid = ((long)k.nnodes * k.nstack + groups - 1) / groups;
    if (k.grid > 256L * 64) k.grid = 256L * 64;
}

int spmm_pick(const SpmmProblem& p, SpmmPlan* plan) {
    SpmmPlan k = {};
    const int W = p.W, nstack = p.form == SP_SINGLE ? p.nstack : 1;
    k.dual = p.form != SP_SINGLE;
    k.bf = p.form == SP_DUAL_BF16;
    k.nstack = nstack;
    k.x_rows = p.x_rows;
    switch (p.form) {
        case SP_SINGLE: {
            REGT_CHECK_ARG(p.nrows > 0 && W > 0, "spmm: empty problem");
            REGT_CHECK_ARG(W % 4 == 0, "spmm: row width %d must be a multiple of 4 floats", W);
            REGT_CHECK_ARG(p.aligned, "spmm: X/Y must be 16-B aligned");
            REGT_CHECK_ARG(nstack >= 1 && p.nrows % nstack == 0, "spmm: nrows=%d not a multiple of nstack=%d", p.nrows, nstack);
            const int W4 = k.W16 = W / 4;
            k.nnodes = p.nrows / nstack;
            // Panels when X cannot live in the XCDs' L2s anyway, rows are whole cache lines and the graph is not small.  (The merged
            // form below has no node-count condition and takes panels for rows wider than 2048 floats whatever the size of X.)
            if (W4 % 8 == 0 && (long)p.x_rows * W * 4 > SP_L2_RESIDENT_BYTES && k.nnodes >= 4096) {
                k.PL = panel_lanes(k.nnodes, W4 % 16 == 0);
                // one operator: the row-block kernel (CSR entries in LDS, the workgroup walks all panels) where wanted and eligible
                if (nstack == 1 && rows_ok(k.nnodes, p.x_rows, 4L * W, k.PL)) { plan_rows(k, p.x_rows, 4 * W); break; }
                plan_panel(k);
                REGT_CHECK_ARG(k.grid < (1L << 31), "spmm: grid too large");
                break;
            }
            if (W4 > 512) {         // column passes of the widest lane-group kernel
                plan_csr(k, 512);
                k.family = SP_CSR_PASSES;
                k.pass16 = 512;
                break;
            }
            plan_csr(k, W4);
            break;
        }
        case SP_DUAL: {
            REGT_CHECK_ARG(p.nrows > 0 && W > 0 && W % 4 == 0, "spmm_dual: width %d must be a multiple of 4 floats", W);
            const int W4 = k.W16 = W / 4;
            k.nnodes = p.nrows;
            if (W % 32 != 0 || ((long)p.x_rows * W * 4 <= SP_L2_RESIDENT_BYTES && W4 <= 512)) {
                // rows that are not whole 128-byte panels, or an X that lives in the L2s anyway: one lane group per row, whole rows
                // (no column passes here: nothing calls the merged operator on rows wider than 2048 floats that are not whole panels)
                REGT_CHECK_ARG(W4 <= 512, "spmm_dual: width %d is neither a multiple of 32 floats nor at most 2048", W);
                plan_csr(k, W4);
                break;
            }
            k.PL = panel_lanes(k.nnodes, W4 % 16 == 0);
            if (rows_ok(k.nnodes, p.x_rows, 4L * W, k.PL)) { plan_rows(k, p.x_rows, 4 * W); break; }
            plan_panel(k);
            REGT_CHECK_ARG(k.grid < (1L << 31), "spmm_dual: grid too large");
            break;
        }
        case SP_DUAL_BF16: {
            // always panels or row blocks: the bf16 rows exist for the large graphs of the bf16 arithmetic, there is no lane-group kernel
            REGT_CHECK_ARG(p.nrows > 0 && W > 0 && W % 64 == 0, "spmm_dual (bf16 rows): width %d must be a multiple of 64 elements", W);
            const long rowbytes = 2L * W;
            k.W16 = (int)(rowbytes / 16);
            k.nnodes = p.nrows;
            k.PL = panel_lanes(k.nnodes, rowbytes % 256 == 0);
            // the panel kernel gathers through a buffer descriptor too, so the bound on X holds for both kernels
            REGT_CHECK_ARG(p.x_rows * rowbytes < (1L << 32) - 4096, "spmm_dual (bf16 rows): X larger than 4 GB");
            // NOT rows_ok: whole panels follow from W % 64, X is bounded above, but nnodes * rowbytes < 4 GB -- which the row-block
            // kernel's output descriptors and 32-bit row offsets need -- is not asked here; rpg with the bf16 residency
            if (rows_wanted() && rows_fit(k.nnodes, k.PL, true)) { plan_rows(k, p.x_rows, (int)rowbytes); break; }
            plan_panel(k);
            k.x_bytes = (unsigned)(p.x_rows * rowbytes);
            REGT_CHECK_ARG(k.grid < (1L << 31), "spmm_dual (bf16 rows): grid too large");
            break;
        }
    }
    *plan = k;
    return REGT_OK;
}

static int pick_and_launch(const SpmmProblem& p, const SpmmPtrs& a, hipStream_t st) {
    SpmmPlan k;
    if (int rc = spmm_pick(p, &k)) return rc;
    return k.family == SP_PANEL || k.family == SP_ROWS ? spmm_launch_panel(k, a, st) : spmm_launch_csr(k, a, st);
}

int launch_spmm_csr(const int* rowptr, const int* col, const float* val, const float* X, float* Y, int nrows,
                    int nrows_x, int W, int nstack, hipStream_t st) {
    const bool aligned = ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) & 15) == 0;
    return pick_and_launch({SP_SINGLE, nrows, nstack, nrows_x, W, aligned}, {rowptr, col, val, nullptr, X, Y, nullptr}, st);
}

int launch_spmm_dual(const int* rowptr, const int* col, const float* val_a, const float* val_l, const float* X, float* YA,
                     float* YL, int nnodes, int W, hipStream_t st) {
    return launch_spmm_dual_x(rowptr, col, val_a, val_l, X, YA, YL, nnodes, nnodes, W, st);
}

int launch_spmm_dual_x(const int* rowptr, const int* col, const float* val_a, const float* val_l, const float* X, float* YA,
                       float* YL, int nnodes, int x_rows, int W, hipStream_t st) {
    return pick_and_launch({SP_DUAL, nnodes, 1, x_rows, W, true}, {rowptr, col, val_a, val_l, X, YA, YL}, st);
}

int launch_spmm_dual_bf16(const int* rowptr, const int* col, const float* val_a, const float* val_l, const void* X, void* YA, void* YL,
                          int nnodes, int x_rows, int W, hipStream_t st) {
    return pick_and_launch({SP_DUAL_BF16, nnodes, 1, x_rows, W, true}, {rowptr, col, val_a, val_l, X, YA, YL}, st);
}

}  // namespace regt
