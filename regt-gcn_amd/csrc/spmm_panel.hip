// Neighbour aggregation for graphs whose X does not live in the XCDs' L2s: the column-panel kernels (one operator, the merged
// two-weight operator on fp32 rows and on bf16 rows) and the row-block kernel.  Which one runs: spmm_pick (spmm_dispatch.hip).
#include "spmm_common.h"

namespace regt {

// ---- XCD-aware column-panel variant (large graphs) --------------------------------------------------
// The plain kernel above re-reads every neighbour row from the Infinity Cache: X (N*W*4 B, 154 MB at
// cfg-3) does not fit the 4 MiB L2 of an XCD, so the gather traffic is nnz*W*4 B (3.1 GB) and the
// kernel runs at the cache-fabric rate, not at the HBM rate.  Here the row is cut into 128-byte column
// panels (one cache line per neighbour per panel) and the work is laid out so that ALL workgroups
// resident on one XCD work on the same (node chunk, panel) at the same time: workgroup b lands on XCD
// b % 8 (round-robin dispatch -- used for speed only), XCD x owns the contiguous node chunk x (with
// region-contiguous node ids that is ~one region, whose neighbours are mostly inside the chunk) and
// walks panel 0, 1, ... over that chunk.  The live working set per XCD is chunk_nodes * 128 B
// (1.6 MB at cfg-3) and stays in L2, so each X line is fetched from HBM / MALL about once.
// Eight lanes own one (row, panel): 8 x 16 B = one 128-B line per neighbour; the 8 lanes pull 8
// (col, val) pairs with one coalesced load and broadcast them by shuffle, four gathers in flight.
template <int PL>     // lanes per row = panel width in float4: 8 = one 128-B line per neighbour, 16 = two (half the CSR re-reads)
__global__ __launch_bounds__(256) void spmm_panel_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                         const float* __restrict__ val, const float* __restrict__ X,
                                                         float* __restrict__ Y, int nnodes, int nstack, int W4,
                                                         int npanels, int nrb) {
    constexpr int ROWS = 256 / PL;
    const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3;
    const int per_panel = nstack * nrb;
    const int panel = li / per_panel;
    if (panel >= npanels) return;
    const int rem = li - panel * per_panel;
    const int s = rem / nrb, rb = rem - s * nrb;
    const SpChunk ch = sp_chunk(xcd, nnodes);
    const int c0 = ch.c0, csz = ch.csz;
    const int g = threadIdx.x / PL, gl = threadIdx.x % PL;
    if (rb * ROWS + g >= csz) return;                     // whole lane group leaves together
    const long row = (long)s * nnodes + c0 + rb * ROWS + g;
    const float4* X4 = reinterpret_cast<const float4*>(X) + panel * PL + gl;
    float4 acc = sp_zero4();
    const int beg = rowptr[row], end = rowptr[row + 1];
    for (int base = beg; base < end; base += PL) {
        const int n = end - base < PL ? end - base : PL;
        int myc = 0;
        float myv = 0.f;
        if (gl < n) { myc = col[base + gl]; myv = val[base + gl]; }
#pragma unroll
        for (int h = 0; h < PL / 4; ++h) {
            if (h * 4 < n) {
                float4 x[4];
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {               // lanes >= n carry (col 0, val 0): harmless
                    const int c = __shfl(myc, h * 4 + e, PL);
                    v[e] = __shfl(myv, h * 4 + e, PL);
                    x[e] = X4[(long)c * W4];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc.x = fmaf(v[e], x[e].x, acc.x); acc.y = fmaf(v[e], x[e].y, acc.y);
                    acc.z = fmaf(v[e], x[e].z, acc.z); acc.w = fmaf(v[e], x[e].w, acc.w);
                }
            }
        }
    }
    // streaming stores: the output is not read again here and must not evict the XCD's slice of X from its L2
    float4* py = reinterpret_cast<float4*>(Y) + row * W4 + panel * PL + gl;
    sp_store_nt(py, acc);
}

// ---- dual-operator panel variant ----------------------------------------------------------------------
// The regional Laplacian rows are (almost) a subset of the full-graph rows: the same neighbour row
// x[col] feeds both A_hat x and L~ x.  With a merged CSR that carries two weights per entry, one gather
// serves both outputs -- half the gather volume of the stacked operator.  Same XCD/panel schedule as above.
template <int PL, int IDX>              // PL lanes per row = panel width in float4 (8: one 128-B line per neighbour, 16: two);
                                        // IDX (<= PL) CSR entries fetched per index load
__global__ __launch_bounds__(256) void spmm_dual_panel_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                              const float* __restrict__ val_a, const float* __restrict__ val_l,
                                                              const float* __restrict__ X, float* __restrict__ YA,
                                                              float* __restrict__ YL, int nnodes, int W4, int npanels, int nrb) {
    static_assert(IDX % 8 == 0 && IDX <= PL, "index chunk is a multiple of the 8-gather round and fits the lane group");
    constexpr int ROWS = 256 / PL;
    const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3;
    const int panel = li / nrb;
    if (panel >= npanels) return;
    const int rb = li - panel * nrb;
    const SpChunk ch = sp_chunk(xcd, nnodes);
    const int c0 = ch.c0, csz = ch.csz;
    const int g = threadIdx.x / PL, gl = threadIdx.x % PL;
    if (rb * ROWS + g >= csz) return;
    const long row = c0 + rb * ROWS + g;
    const float4* X4 = reinterpret_cast<const float4*>(X) + panel * PL + gl;
    float4 aa = sp_zero4(), al = sp_zero4();
    const int beg = rowptr[row], end = rowptr[row + 1];
    for (int base = beg; base < end; base += IDX) {
        const int n = end - base < IDX ? end - base : IDX;
        int myc = 0;
        float mya = 0.f, myl = 0.f;
        if (gl < n) { myc = col[base + gl]; mya = val_a[base + gl]; myl = val_l[base + gl]; }
#pragma unroll
        for (int r = 0; r < IDX / 8; ++r) {
            if (r * 8 < n) {
                // all 8 gathers of the round in flight before the first FMA; entries >= n carry (col 0, weights 0)
                // (written out here and in the bf16 kernel: one sp_round8<BF, PL>(.., gather) moves both kernels' machine code)
                float4 x[8];
                float va[8], vl[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int c = __shfl(myc, r * 8 + e, PL);
                    va[e] = __shfl(mya, r * 8 + e, PL);
                    vl[e] = __shfl(myl, r * 8 + e, PL);
                    x[e] = r * 8 + e < n ? X4[(long)c * W4] : sp_zero4();
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    aa.x = fmaf(va[e], x[e].x, aa.x); aa.y = fmaf(va[e], x[e].y, aa.y);
                    aa.z = fmaf(va[e], x[e].z, aa.z); aa.w = fmaf(va[e], x[e].w, aa.w);
                    al.x = fmaf(vl[e], x[e].x, al.x); al.y = fmaf(vl[e], x[e].y, al.y);
                    al.z = fmaf(vl[e], x[e].z, al.z); al.w = fmaf(vl[e], x[e].w, al.w);
                }
            }
        }
    }
    float4* pa = reinterpret_cast<float4*>(YA) + row * W4 + panel * PL + gl;
    float4* pl = reinterpret_cast<float4*>(YL) + row * W4 + panel * PL + gl;
    {
        // the outputs are not read again by this kernel: streaming stores keep them from evicting the XCD's slice of X
        // from its L2 (cfg-3, X resident in the Infinity Cache: 186 -> 149 us, L2 hits 64 -> 70 %; inside a training
        // step, where X comes from HBM, 174 -> 167 us)
        sp_store_nt(pa, aa);
        sp_store_nt(pl, al);
    }
}

// The dual-operator panel kernel on bf16 rows (REGT_GEMM_MODE=bf16: x, A_hat x and L~ x only ever feed bf16 matrix-core operands):
// same schedule, a lane holds 8 elements of its 16 bytes, sums in fp32 in CSR order, outputs rounded once (nearest even).
template <int PL, int IDX>
__global__ __launch_bounds__(256, 5) void spmm_dual_panel_bf16_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                   const float* __restrict__ val_a, const float* __restrict__ val_l,
                                                                   const uint4* __restrict__ X, uint4* __restrict__ YA,
                                                                   uint4* __restrict__ YL, int nnodes, int W16, int npanels, int nrb,
                                                                   unsigned x_bytes) {
    static_assert(IDX % 8 == 0 && IDX <= PL, "index chunk is a multiple of the 8-gather round and fits the lane group");
    constexpr int ROWS = 256 / PL;
    // rows of X through a buffer descriptor: 32-bit byte offsets (host-checked), no 64-bit address arithmetic per gather
    const __amdgpu_buffer_rsrc_t sx = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(X), 0, x_bytes, 0x00020000);
    const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3;
    const int panel = li / nrb;
    if (panel >= npanels) return;
    const int rb = li - panel * nrb;
    const SpChunk ch = sp_chunk(xcd, nnodes);
    const int c0 = ch.c0, csz = ch.csz;
    const int g = threadIdx.x / PL, gl = threadIdx.x % PL;
    if (rb * ROWS + g >= csz) return;
    const long row = c0 + rb * ROWS + g;
    const unsigned lane_off = (unsigned)(panel * PL + gl) * 16u, rowbytes = (unsigned)W16 * 16u;
    SpAcc<true> aa, al;
#pragma unroll
    for (int i = 0; i < 8; ++i) { aa.v[i] = 0.f; al.v[i] = 0.f; }      // (written out: as a helper, sp_zero(SpAcc<BF>&), the reset moves this kernel's machine code)
    const int beg = rowptr[row], end = rowptr[row + 1];
    for (int base = beg; base < end; base += IDX) {
        const int n = end - base < IDX ? end - base : IDX;
        int myc = 0;
        float mya = 0.f, myl = 0.f;
        if (gl < n) { myc = col[base + gl]; mya = val_a[base + gl]; myl = val_l[base + gl]; }
#pragma unroll
        for (int r = 0; r < IDX / 8; ++r) {
            if (r * 8 < n) {
                u32x4_t x[8];
                float va[8], vl[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int c = __shfl(myc, r * 8 + e, PL);
                    va[e] = __shfl(mya, r * 8 + e, PL);
                    vl[e] = __shfl(myl, r * 8 + e, PL);
                    x[e] = r * 8 + e < n ? __builtin_amdgcn_raw_buffer_load_b128(sx, (unsigned)c * rowbytes + lane_off, 0, 0) : u32x4_t{0, 0, 0, 0};
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    sp_fma<true>(aa, va[e], x[e]);
                    sp_fma<true>(al, vl[e], x[e]);
                }
            }
        }
    }
    const u32x4_t pa = sp_pack<true>(aa), pl = sp_pack<true>(al);
    unsigned* oa = reinterpret_cast<unsigned*>(YA + row * W16 + panel * PL + gl);
    unsigned* ol = reinterpret_cast<unsigned*>(YL + row * W16 + panel * PL + gl);
    // (written out: an sp_store_nt of packed words moves this kernel's machine code)
    __builtin_nontemporal_store(pa.x, oa); __builtin_nontemporal_store(pa.y, oa + 1);
    __builtin_nontemporal_store(pa.z, oa + 2); __builtin_nontemporal_store(pa.w, oa + 3);
    __builtin_nontemporal_store(pl.x, ol); __builtin_nontemporal_store(pl.y, ol + 1);
    __builtin_nontemporal_store(pl.z, ol + 2); __builtin_nontemporal_store(pl.w, ol + 3);
}

// ---- row-block variant: the CSR entries of a workgroup's rows live in LDS, the workgroup walks ALL column panels ------------
// The panel kernels above read a row's (col, weight, weight) entries again for every panel: 6 x 13 MB at cfg-3, and those
// streams compete with the X slice for the XCD's 4 MiB L2.  Here a workgroup owns GROUPS x rpg consecutive-ish rows of its
// XCD's node chunk for the whole launch: it copies their entries to LDS once (one coalesced pass over the CSR: 13 MB in total)
// and then walks panel 0, 1, ... over them.  rpg is chosen on the host so that ALL workgroups of an XCD are resident at
// once (8 per CU): they start together and advance through the panels at about the same pace, so the live slice of X per
// XCD is still ~one panel wide (speed only -- nothing depends on the pacing).  A lane group of PL lanes owns one row at a time;
// it reads entries back with broadcast ds_read_b128 (no shuffles) and keeps 8 gathers in flight.  Rows of X / Y are addressed
// through buffer descriptors: 32-bit byte offsets, the panel offset is the instruction's scalar offset.
// BF: rows of X and of both outputs hold bf16 (16 bytes = 8 elements per lane), accumulation in fp32, one rounding at the end.
template <int PL, bool DUAL, bool BF>
__global__ __launch_bounds__(256, BF ? 5 : 8) void spmm_rows_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        const float* __restrict__ val_a, const float* __restrict__ val_l,
                                                        const void* __restrict__ X, void* __restrict__ YA, void* __restrict__ YL,
                                                        int nnodes, unsigned x_bytes, unsigned y_bytes, int rowbytes, int npanels, int rpg, int cap) {
    constexpr int GROUPS = 256 / PL;
    extern __shared__ __attribute__((aligned(16))) int sp_lds[];
    int* rp = sp_lds;
    SpEnt* ents = reinterpret_cast<SpEnt*>(sp_lds + 260);
    const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3;
    const SpChunk ch = sp_chunk(xcd, nnodes);
    const int c0 = ch.c0, csz = ch.csz;
    const int rows_wg = GROUPS * rpg;
    const int rb = li * rows_wg;                       // first row of the workgroup inside the chunk
    if (rb >= csz) return;
    const int nrows = csz - rb < rows_wg ? csz - rb : rows_wg;
    const int row0 = c0 + rb;
    const int tid = threadIdx.x, g = tid / PL, gl = tid % PL;
    const int first = rowptr[row0], last = rowptr[row0 + nrows];
    const int ntile = last - first;
    const bool in_lds = ntile <= cap;          // (workgroup-uniform) else: entries are read from global memory again per panel
    if (tid <= nrows) rp[tid] = rowptr[row0 + tid] - first;
    if (in_lds) {
        for (int i = tid; i < ntile; i += 256) {
            SpEnt e;
            e.col = col[first + i]; e.wa = val_a[first + i]; e.wl = DUAL ? val_l[first + i] : 0.f; e.pad = 0;
            ents[i] = e;
        }
    }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t sx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(X), 0, x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t sa = __builtin_amdgcn_make_buffer_rsrc(YA, 0, y_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t sl = __builtin_amdgcn_make_buffer_rsrc(DUAL ? YL : YA, 0, y_bytes, 0x00020000);
    for (int p = 0; p < npanels; ++p) {
        const int soff = p * PL * 16;
        for (int k = 0; k < rpg; ++k) {
            const int rl = g + GROUPS * k;
            if (rl >= nrows) break;                     // whole lane group leaves together
            const int beg = rp[rl], end = rp[rl + 1];
            SpAcc<BF> aa, al;
#pragma unroll
            for (int i = 0; i < (BF ? 8 : 4); ++i) { aa.v[i] = 0.f; al.v[i] = 0.f; }      // (written out: as a helper, sp_zero(SpAcc<BF>&), the reset moves this kernel's machine code)
            for (int e = beg; e < end; e += 8) {
                u32x4_t x[8];
                float wa[8], wl[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool ok = e + j < end;
                    SpEnt en{0, 0.f, 0.f, 0};
                    if (ok) {
                        if (in_lds) en = ents[e + j];
                        else { en.col = col[first + e + j]; en.wa = val_a[first + e + j]; en.wl = DUAL ? val_l[first + e + j] : 0.f; }
                    }
                    wa[j] = en.wa; wl[j] = en.wl;
                    x[j] = ok ? __builtin_amdgcn_raw_buffer_load_b128(sx, (unsigned)en.col * (unsigned)rowbytes + gl * 16, soff, 0) : u32x4_t{0, 0, 0, 0};
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    sp_fma<BF>(aa, wa[j], x[j]);
                    if (DUAL) sp_fma<BF>(al, wl[j], x[j]);
                }
            }
            // streaming stores: the outputs must not evict the XCD's slice of X from its L2 (aux bit 1 = nt)
            const unsigned yo = (unsigned)(row0 + rl) * (unsigned)rowbytes + gl * 16 + soff;
            __builtin_amdgcn_raw_buffer_store_b128(sp_pack<BF>(aa), sa, yo, 0, 2);
            if (DUAL) __builtin_amdgcn_raw_buffer_store_b128(sp_pack<BF>(al), sl, yo, 0, 2);
        }
    }
}

template <int PL, bool DUAL, bool BF>
static void launch_rows(const SpmmPlan& k, const SpmmPtrs& a, hipStream_t st) {
    hipLaunchKernelGGL((spmm_rows_kernel<PL, DUAL, BF>), dim3((unsigned)k.grid), dim3(256), k.lds, st, a.rowptr, a.col, a.val_a, a.val_l, a.X, a.YA, a.YL,
                       k.nnodes, k.x_bytes, k.y_bytes, k.rowbytes, k.npanels, k.rpg, k.cap);
}
template <int PL>
static void launch_panel(const SpmmPlan& k, const SpmmPtrs& a, hipStream_t st) {
    const dim3 grid((unsigned)k.grid);
    // (streaming output stores, 16-entry index chunks: the variants measured against them -- ordinary stores, 8-entry chunks,
    // non-temporal CSR loads, a padded X stride: profiles/r03_spmm_pmc_variants.txt, r04_spmm_ab.txt -- are gone)
    if (k.bf)
        hipLaunchKernelGGL((spmm_dual_panel_bf16_kernel<PL, PL>), grid, dim3(256), 0, st, a.rowptr, a.col, a.val_a, a.val_l, static_cast<const uint4*>(a.X),
                           static_cast<uint4*>(a.YA), static_cast<uint4*>(a.YL), k.nnodes, k.W16, k.npanels, k.nrb, k.x_bytes);
    else if (k.dual)
        hipLaunchKernelGGL((spmm_dual_panel_kernel<PL, PL>), grid, dim3(256), 0, st, a.rowptr, a.col, a.val_a, a.val_l, static_cast<const float*>(a.X),
                           static_cast<float*>(a.YA), static_cast<float*>(a.YL), k.nnodes, k.W16, k.npanels, k.nrb);
    else
        hipLaunchKernelGGL(spmm_panel_kernel<PL>, grid, dim3(256), 0, st, a.rowptr, a.col, a.val_a, static_cast<const float*>(a.X), static_cast<float*>(a.YA),
                           k.nnodes, k.nstack, k.W16, k.npanels, k.nrb);
}
template <int PL>
static void launch_pl(const SpmmPlan& k, const SpmmPtrs& a, hipStream_t st) {
    if (k.family == SP_PANEL) launch_panel<PL>(k, a, st);
    else if (k.bf) launch_rows<PL, true, true>(k, a, st);
    else if (k.dual) launch_rows<PL, true, false>(k, a, st);
    else launch_rows<PL, false, false>(k, a, st);
}

int spmm_launch_panel(const SpmmPlan& k, const SpmmPtrs& a, hipStream_t st) {
    if (k.PL == 16) launch_pl<16>(k, a, st);
    else launch_pl<8>(k, a, st);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace regt
