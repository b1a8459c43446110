// Weight gradients out[Nout x Nin] = P^T Q of the RegT-GCN cell (the transposes of models/utils.py:168-188 and of the regional embedding,
// models/RegionalTemporalGCN.py:136-148) on the fp32 MFMA: the two-workgroup kernel in its three column widths, the three-workgroup
// kernel and the scalar-guarded fallback, with the launcher that instantiates them.  Which one runs: wgrad_dispatch.hip.
// (Operands on the bf16 matrix pipe: wgrad_bf16.hip; the reduction of the row-chunk slabs: wgrad_reduce.hip.)
#include "wgrad_common.h"

namespace regt {

// ---- weight gradients: out[Nout x Nin] = P^T Q ----------------------------------------------------
// (tile and LDS layout: W_BK, W_LDP in wgrad_common.h)
// 64 (round 4): waves 4x1, each 1 x 2 MFMA tiles -- a 64-wide right-hand side ([x | L~ x] at F = 32) as ONE column tile: P crosses
// HBM / L2 once instead of once per 32 columns and a fragment of P feeds two MFMAs; the two-part right-hand side may split INSIDE it
template <int BNW, bool PBF = false>   // 128: waves 2x2, each 2x2 MFMA tiles;  32: waves 4x1, each one MFMA tile
__global__ __launch_bounds__(256, 2) void wgrad_kernel(WgradArgs a) {
    static_assert(BNW == 128 || BNW == 64 || BNW == 32, "column tile");
    constexpr int WM = BNW == 128 ? 2 : 1, WN = BNW == 32 ? 1 : 2;
    constexpr int LDQ = BNW + 4;
    constexpr int P_TILE = W_BK * W_LDP, Q_TILE = W_BK * LDQ;
    constexpr int QSLOTS = (W_BK * BNW / 4) / 256;          // float4 slots per thread for Q (4 or 1)
    using Core = FastCore<true, false>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int wr = BNW == 128 ? (wid >> 1) : wid, wc = BNW == 128 ? (wid & 1) : 0;
    const int tiles_i = (a.Nout + 127) / 128, tiles_j = (a.Nin + BNW - 1) / BNW;
    const int tpc = tiles_i * tiles_j;
    const WgradBlock blk = wgrad_block(a.nchunks, tpc);
    const int tile = blk.tile, chunk = blk.chunk;
    const int i0 = (tile / tiles_j) * 128, j0 = (tile % tiles_j) * BNW;
    const WgradRows rows = wgrad_chunk_rows(a, chunk);
    const long r0 = rows.r0, r1 = rows.r1;
    const int nrows = (int)(r1 - r0);

    f32x16 acc[WM][WN];      // (zero_acc, written out: through the helper the compiler scheduled this kernel differently)
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    f32x2 csum2 = {0.f, 0.f};

    // Both operands stream through wave-uniform buffer descriptors based at the chunk's first row
    // (vector path: ldp/ldq multiples of 4 and 16-B aligned bases, checked on the host).
    // PBF: P holds bf16 elements (REGT_GEMM_MODE=bf16: dhp, dzp|drp are rounded once by their producer): a 32 x 128 slab is
    // 8 KB = two 16-byte loads per thread (8 columns each), widened to fp32 on the way into LDS -- this kernel's arithmetic
    // stays the fp32 MFMA
    const bool second = a.Q2 != nullptr && j0 >= a.nin_split;          // this column tile reads the second operand
    // BNW = 64: the split may run through the tile -- columns past it come from Q2 through a second descriptor (both requested by
    // every lane with complementary out-of-range offsets, OR-ed: an out-of-range lane returns 0 without touching memory)
    const bool straddle = BNW == 64 && a.Q2 != nullptr && !second && j0 + BNW > a.nin_split;
    const int ldp = (int)a.ldp, ldq = second ? (int)a.ldq2 : (int)a.ldq;
    // Descriptors based at the chunk's first row with num_records = the chunk's bytes: a row past the chunk's end is out of
    // range (returns 0) without a per-load guard.  Per thread the offsets inside a 32-row slab are constants (a column past
    // Nout / Nin gets an out-of-range constant), the slab's first row goes into the instruction's scalar offset: no vector
    // instruction per load in the K loop (VALU work shares the SIMD's issue with the MFMAs, gemm_split.h).
    const char* pbase = reinterpret_cast<const char*>(a.P) + (PBF ? 2 : 4) * (r0 * a.ldp + i0);
    const float* qbase = second ? a.Q2 + r0 * a.ldq2 + (j0 - a.nin_split) : a.Q + r0 * a.ldq + j0;
    const long pbytes = (long)nrows * ldp * (PBF ? 2 : 4), qbytes = (long)nrows * ldq * 4;
    const __amdgpu_buffer_rsrc_t sp = wgrad_chunk_desc(pbase, pbytes);
    const __amdgpu_buffer_rsrc_t sq = wgrad_chunk_desc(qbase, qbytes);
    const long q2bytes = straddle ? (long)nrows * a.ldq2 * 4 : 0;
    const __amdgpu_buffer_rsrc_t sq2 = wgrad_chunk_desc(straddle ? a.Q2 + r0 * a.ldq2 : qbase, q2bytes);
    int vp[4], vq[QSLOTS], vq2[QSLOTS];
    if (PBF) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int idx = tid + 256 * s, i = 8 * (idx & 15);
            vp[s] = i0 + i < a.Nout ? 2 * ((idx >> 4) * ldp + i) : (int)Core::SRD_OOB;
        }
        vp[2] = vp[3] = 0;
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int slot = tid + 256 * s, i = 4 * (slot & 31);
            vp[s] = i0 + i < a.Nout ? 4 * ((slot >> 5) * ldp + i) : (int)Core::SRD_OOB;
        }
    }
#pragma unroll
    for (int s = 0; s < QSLOTS; ++s) {
        const int slot = tid + 256 * s, j = 4 * (slot % (BNW / 4));
        const bool in2 = straddle && j0 + j >= a.nin_split;
        vq[s] = j0 + j < a.Nin && !in2 ? 4 * ((slot / (BNW / 4)) * ldq + j) : (int)Core::SRD_OOB;
        vq2[s] = in2 && j0 + j < a.Nin ? 4 * ((slot / (BNW / 4)) * (int)a.ldq2 + (j0 + j - a.nin_split)) : (int)Core::SRD_OOB;
    }
    const int sp_step = ldp * (PBF ? 2 : 4), sq_step = ldq * 4, sq2_step = (int)a.ldq2 * 4;      // bytes per row

    auto load = [&](int k0, float4 (&rp)[4], float4 (&rq)[QSLOTS]) {
        const int sop = k0 * sp_step, soq = k0 * sq_step;
        if (PBF) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float4 raw = buf_ld4(sp, vp[s], sop);
                rp[2 * s] = widen_bf16x4(__float_as_uint(raw.x), __float_as_uint(raw.y));
                rp[2 * s + 1] = widen_bf16x4(__float_as_uint(raw.z), __float_as_uint(raw.w));
            }
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) rp[s] = buf_ld4(sp, vp[s], sop);
        }
#pragma unroll
        for (int s = 0; s < QSLOTS; ++s) rq[s] = buf_ld4(sq, vq[s], soq);
        if (BNW == 64) {        // unconditional (a tile that does not straddle the split has out-of-range offsets here): no branch around loads
#pragma unroll
            for (int s = 0; s < QSLOTS; ++s) {
                const float4 v = buf_ld4(sq2, vq2[s], k0 * sq2_step);
                rq[s] = or4(rq[s], v);
            }
        }
    };
    auto store = [&](int stage, const float4 (&rp)[4], float4 (&rq)[QSLOTS]) {
        float* lp = lds + stage * (P_TILE + Q_TILE);
        float* lq = lp + P_TILE;
        if (PBF) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int idx = tid + 256 * s;
                float* d = lp + (idx >> 4) * W_LDP + 8 * (idx & 15);
                *reinterpret_cast<float4*>(d) = rp[2 * s];
                *reinterpret_cast<float4*>(d + 4) = rp[2 * s + 1];
            }
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                int slot = tid + 256 * s;
                *reinterpret_cast<float4*>(lp + (slot >> 5) * W_LDP + 4 * (slot & 31)) = rp[s];
            }
        }
#pragma unroll
        for (int s = 0; s < QSLOTS; ++s) {
            int slot = tid + 256 * s;
            float4 v = rq[s];
            if (a.q_relu) v = relu4(v);
            *reinterpret_cast<float4*>(lq + (slot / (BNW / 4)) * LDQ + 4 * (slot % (BNW / 4))) = v;
        }
    };
    struct Frag { float a[WM][4], b[WN][4]; };
    auto read_frag = [&](int stage, int kg) {
        const float* lp = lds + stage * (P_TILE + Q_TILE);
        const float* lq = lp + P_TILE;
        Frag f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = kg * 8 + lh * 4 + j;
#pragma unroll
            for (int mi = 0; mi < WM; ++mi) f.a[mi][j] = lp[k * W_LDP + wr * (32 * WM) + mi * 32 + lr];
#pragma unroll
            for (int ni = 0; ni < WN; ++ni) f.b[ni][j] = lq[k * LDQ + wc * (32 * WN) + ni * 32 + lr];
        }
        return f;
    };
    auto mfma = [&](const Frag& f) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mi = 0; mi < WM; ++mi)
#pragma unroll
                for (int ni = 0; ni < WN; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[mi][j], f.b[ni][j], acc[mi][ni], 0, 0, 0);
    };
    auto colsum = [&](int stage) {
        if (a.colsum && (j0 == 0 || a.all_csum) && tid < 128) {      // (all_csum: same work in every column tile, launch_wgrad)
            const float* lp = lds + stage * (P_TILE + Q_TILE);
#pragma unroll
            for (int k = 0; k < W_BK; k += 2) {      // two partial sums (even / odd rows): one packed add per two rows
                const f32x2 v = {lp[k * W_LDP + tid], lp[(k + 1) * W_LDP + tid]};
                csum2 += v;
            }
        }
    };

    const int nit = (nrows + W_BK - 1) / W_BK;
    if (nit > 0) {
        float4 rp[4], rq[QSLOTS];
        load(0, rp, rq);
        store(0, rp, rq);
        __syncthreads();
        Frag cur = read_frag(0, 0);
        for (int it = 0; it + 1 < nit; ++it) {
            const int stage = it & 1;
            load((it + 1) * W_BK, rp, rq);
#pragma unroll
            for (int kg = 0; kg < 4; ++kg) {
                Frag nxt;
                if (kg < 3) nxt = read_frag(stage, kg + 1);
#pragma unroll
                for (int r = 0; r < 4 * WM * WN; ++r) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // DS read
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
                    __builtin_amdgcn_sched_group_barrier(0x006, 4, 0);   // VALU | SALU
                }
                mfma(cur);
                if (kg < 3) cur = nxt;
            }
            colsum(stage);
            store(stage ^ 1, rp, rq);
            __syncthreads();
            cur = read_frag(stage ^ 1, 0);
        }
        {
            const int stage = (nit - 1) & 1;
#pragma unroll
            for (int kg = 0; kg < 4; ++kg) {
                Frag nxt;
                if (kg < 3) nxt = read_frag(stage, kg + 1);
                mfma(cur);
                if (kg < 3) cur = nxt;
            }
            colsum(stage);
        }
    }
    const long stride = (long)a.Nout * a.Nin + (a.colsum ? a.Nout : 0);
    float* out = a.slab + (long)chunk * stride;
#pragma unroll
    for (int mi = 0; mi < WM; ++mi)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            int i = i0 + wr * (32 * WM) + mi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
            if (i < a.Nout) {
#pragma unroll
                for (int ni = 0; ni < WN; ++ni) {
                    int j = j0 + wc * (32 * WN) + ni * 32 + lr;
                    if (j < a.Nin) out[(long)i * a.Nin + j] = acc[mi][ni][reg];
                }
            }
        }
    if (a.colsum && j0 == 0 && tid < 128 && i0 + tid < a.Nout) out[(long)a.Nout * a.Nin + i0 + tid] = csum2[0] + csum2[1];
}

// fp32 weight gradients on THREE workgroups per CU: 16-row half slabs (two LDS stages of 16 x 132 floats per operand,
// 33,792 B), the half-step schedule of SplitCore::run_t (stage 0 / 1 = the halves of the current 32-row slab, the next slab
// in registers, its halves stored while the other half is multiplied), <= 168 VGPRs.  The two-workgroup kernel above
// reaches ~0.73 of the fp32 MFMA peak: one wave per SIMD and workgroup, every barrier and LDS round trip of a workgroup
// idles its share of the matrix pipe unless another workgroup fills in.  Same tiling, chunking, arithmetic order inside a
// chunk (k ascending, the same pairing of k to MFMA lanes) and output as wgrad_kernel<128, false>.
__global__ __launch_bounds__(256, 3) void wgrad3_kernel(WgradArgs a) {
    constexpr int HK = 16, LDT = 128 + 4, OP_T = HK * LDT, STAGE = 2 * OP_T;      // floats
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int wr = wid >> 1, wc = wid & 1;
    const int tiles_i = (a.Nout + 127) / 128, tiles_j = (a.Nin + 127) / 128;
    const int tpc = tiles_i * tiles_j;
    const WgradBlock blk = wgrad_block(a.nchunks, tpc);
    const int tile = blk.tile, chunk = blk.chunk;
    const int i0 = (tile / tiles_j) * 128, j0 = (tile % tiles_j) * 128;
    const WgradRows rows = wgrad_chunk_rows(a, chunk);
    const long r0 = rows.r0, r1 = rows.r1;
    const int nrows = (int)(r1 - r0);
    const int ldp = (int)a.ldp, ldq = (int)a.ldq;
    const long pbytes = (long)nrows * ldp * 4, qbytes = (long)nrows * ldq * 4;
    const __amdgpu_buffer_rsrc_t sp = wgrad_chunk_desc(a.P + r0 * a.ldp + i0, pbytes);
    const __amdgpu_buffer_rsrc_t sq = wgrad_chunk_desc(a.Q + r0 * a.ldq + j0, qbytes);
    // a half slab = 16 rows x 128 columns per operand = 512 float4: slots tid, tid + 256 -> row slot >> 5, column 4 (slot & 31)
    int vp[2], vq[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int slot = tid + 256 * s, c4 = 4 * (slot & 31);
        vp[s] = i0 + c4 < a.Nout ? 4 * ((slot >> 5) * ldp + c4) : (int)0x7FFFFFF8;
        vq[s] = j0 + c4 < a.Nin ? 4 * ((slot >> 5) * ldq + c4) : (int)0x7FFFFFF8;
    }
    const int sp_step = HK * ldp * 4, sq_step = HK * ldq * 4;        // bytes per half slab

    f32x16 acc[2][2];      // (zero_acc, written out: through the helper the compiler scheduled this kernel differently)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    f32x2 csum2 = {0.f, 0.f};
    const bool do_colsum = a.colsum && (j0 == 0 || a.all_csum) && tid < 128;      // stored by column tile 0 only
    const bool store_colsum = a.colsum && j0 == 0 && tid < 128;

    // registers of half h of a slab: rp[2 h + s], rq[2 h + s]
    auto load_half = [&](int g, int h, float4 (&rp)[4], float4 (&rq)[4]) {       // g = half-slab index (rows 16 g ..); past the end: zeros
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            rp[2 * h + s] = buf_ld4(sp, vp[s], g * sp_step);
            rq[2 * h + s] = buf_ld4(sq, vq[s], g * sq_step);
        }
    };
    auto store_half = [&](int h, const float4 (&rp)[4], const float4 (&rq)[4]) {
        float* lp = lds + h * STAGE;
        float* lq = lp + OP_T;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int slot = tid + 256 * s;
            float4 v = rq[2 * h + s];
            if (a.q_relu) v = relu4(v);
            *reinterpret_cast<float4*>(lp + (slot >> 5) * LDT + 4 * (slot & 31)) = rp[2 * h + s];
            *reinterpret_cast<float4*>(lq + (slot >> 5) * LDT + 4 * (slot & 31)) = v;
        }
    };
    struct Frag { float a[2][8], b[2][8]; };       // [32-row block][k slot]: lane half lh holds k = 8 kk + 4 lh + j at slot 4 kk + j
    auto read_frag = [&](int h) {
        const float* lp = lds + h * STAGE;
        const float* lq = lp + OP_T;
        Frag f;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = kk * 8 + lh * 4 + j;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    f.a[t][4 * kk + j] = lp[k * LDT + wr * 64 + t * 32 + lr];
                    f.b[t][4 * kk + j] = lq[k * LDT + wc * 64 + t * 32 + lr];
                }
            }
        return f;
    };
    auto mfma = [&](const Frag& f) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[mi][q], f.b[ni][q], acc[mi][ni], 0, 0, 0);
    };
    auto colsum = [&](int h) {
        if (do_colsum) {
            const float* lp = lds + h * STAGE;
#pragma unroll
            for (int k = 0; k < HK; k += 2) {
                const f32x2 v = {lp[k * LDT + tid], lp[(k + 1) * LDT + tid]};
                csum2 += v;
            }
        }
    };
    // multiply half hc (in LDS) while half hs of the next slab is stored and the same half of the slab after next requested
    auto fused = [&](int hs, int hc, int gnext, float4 (&rp)[4], float4 (&rq)[4]) {
        __builtin_amdgcn_sched_barrier(0);
        const Frag f = read_frag(hc);
        store_half(hs, rp, rq);
        mfma(f);
        load_half(gnext, hs, rp, rq);
        __builtin_amdgcn_sched_group_barrier(0x100, 32, 0);          // the fragment reads (ds_read_b32 / ds_read2)
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);       // MFMA
            __builtin_amdgcn_sched_group_barrier(0x006, 4, 0);       // VALU | SALU
            if (r < 4) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // DS write
            else __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);          // VMEM read
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    const int nslab = (nrows + 2 * HK - 1) / (2 * HK);
    if (nslab > 0) {
        float4 rp[4], rq[4];
        load_half(0, 0, rp, rq);
        load_half(1, 1, rp, rq);
        store_half(0, rp, rq);
        store_half(1, rp, rq);
        load_half(2, 0, rp, rq);          // slab 1 (zeros past the chunk's end)
        load_half(3, 1, rp, rq);
        __syncthreads();
        mfma(read_frag(0));
        colsum(0);
        for (int t = 0; t + 1 < nslab; ++t) {
            __syncthreads();
            fused(0, 1, 2 * t + 4, rp, rq);       // store half 2t+2 -> stage 0, multiply half 2t+1, request half 2t+4
            colsum(1);
            __syncthreads();
            fused(1, 0, 2 * t + 5, rp, rq);
            colsum(0);
        }
        __syncthreads();
        mfma(read_frag(1));
        colsum(1);
    }
    const long stride = (long)a.Nout * a.Nin + (a.colsum ? a.Nout : 0);
    float* out = a.slab + (long)chunk * stride;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int i = i0 + wr * 64 + mi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
            if (i < a.Nout) {
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const int j = j0 + wc * 64 + ni * 32 + lr;
                    if (j < a.Nin) out[(long)i * a.Nin + j] = acc[mi][ni][reg];
                }
            }
        }
    if (store_colsum && i0 + tid < a.Nout) out[(long)a.Nout * a.Nin + i0 + tid] = csum2[0] + csum2[1];
}

// fp32 weight gradients on ONE workgroup per CU, each wave owning a 128 x 128 block (Nin == 256, Nout % 256 == 0: wgrad_pick).
// A loop of v_mfma_f32_32x32x2_f32 holds 154 TFLOP/s with one wave per SIMD and ~100 with two (DESIGN_HISTORY section D): here a
// SIMD's one wave holds 4 x 4 MFMA tiles (256 accumulator registers), so a k step of 2 is 16 MFMAs against 4 + 4 fragment values --
// a quarter of the LDS and global traffic per MFMA of the 2 x 2 kernels above -- and no other wave competes for the matrix pipe.
// Two LDS stages of a 32-row slab of both operands (32 x 260 floats each, k-major as in HBM: 133,120 B); while slab t is multiplied
// the registers holding slab t + 1 go to the other stage and slab t + 2 is requested, one 16-byte store and one 16-byte load per
// operand slot between the MFMAs of a k step; one barrier per slab (16 k steps = 256 MFMAs per wave).
// Same chunking, arithmetic order inside a chunk (k ascending, the same pairing of k to MFMA lanes), column sums and slab layout as
// wgrad3_kernel / wgrad_kernel<128, false>: on the same row chunks the slabs agree bit for bit.
template <bool CSUM>      // CSUM: also the column sums of P (a template argument: a branch per k step would cut the schedule of the K loop)
__global__ __launch_bounds__(256, 1) void wgrad_wave_kernel(WgradArgs a) {
    constexpr int LDT = 256 + 4, OP_T = W_BK * LDT, STAGE = 2 * OP_T;      // floats (4 LDT = 16 mod 64 banks, as W_LDP)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int wr = wid >> 1, wc = wid & 1;
    const int tpc = a.Nout / 256;                                          // 256-row output tiles; one 256-column tile
    const WgradBlock blk = wgrad_block(a.nchunks, tpc);
    const int i0 = blk.tile * 256, chunk = blk.chunk;
    const WgradRows rows = wgrad_chunk_rows(a, chunk);
    const long r0 = rows.r0, r1 = rows.r1;
    const int nrows = (int)(r1 - r0);
    const int ldp = (int)a.ldp, ldq = (int)a.ldq;
    const long pbytes = (long)nrows * ldp * 4, qbytes = (long)nrows * ldq * 4;
    const __amdgpu_buffer_rsrc_t sp = wgrad_chunk_desc(a.P + r0 * a.ldp + i0, pbytes);
    const __amdgpu_buffer_rsrc_t sq = wgrad_chunk_desc(a.Q + r0 * a.ldq, qbytes);
    // a slab = 32 rows x 256 columns per operand = 2048 float4: slot tid + 256 s -> row (tid >> 6) + 4 s, column 4 (tid & 63).
    // One vector offset per operand; the slab's first row and the slot's 4 s rows go into the scalar offset.
    const int srow = tid >> 6, scol = 4 * (tid & 63);
    const int vp = 4 * (srow * ldp + scol), vq = 4 * (srow * ldq + scol);
    const int sp_row = ldp * 4, sq_row = ldq * 4;                          // bytes per row
    float* const st_base = lds + srow * LDT + scol;                        // + stage * STAGE (+ OP_T for Q) + 4 s LDT
    const float* const fa_base = lds + (4 * lh) * LDT + wr * 128 + lr;     // + stage * STAGE + k LDT + 32 mi
    const float* const fb_base = lds + OP_T + (4 * lh) * LDT + wc * 128 + lr;
    const float* const cs_base = lds + tid;                                // column tid of P

    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    f32x2 csum2 = {0.f, 0.f};

    float4 rp[8], rq[8];
    auto load_slot = [&](int t, int s) {         // slot s of slab t (rows past the chunk's end: zeros)
        rp[s] = buf_ld4(sp, vp, (32 * t + 4 * s) * sp_row);
        rq[s] = buf_ld4(sq, vq, (32 * t + 4 * s) * sq_row);
    };
    auto store_slot = [&](int stage, int s) {
        float* d = st_base + stage * STAGE + 4 * s * LDT;
        *reinterpret_cast<float4*>(d) = rp[s];
        *reinterpret_cast<float4*>(d + OP_T) = rq[s];
    };
    struct Frag { float a[4], b[4]; };
    // k step s of a slab (0..15): lane half lh holds k = 8 (s >> 2) + 4 lh + (s & 3)
    auto read_frag = [&](int stage, int s) {
        const int off = stage * STAGE + (8 * (s >> 2) + (s & 3)) * LDT;
        Frag f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f.a[t] = fa_base[off + 32 * t];
            f.b[t] = fb_base[off + 32 * t];
        }
        return f;
    };
    auto mfma = [&](const Frag& f) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[mi], f.b[ni], acc[mi][ni], 0, 0, 0);
    };
    // rows 2 s, 2 s + 1 of column tid of P: two partial sums (even / odd rows), one packed add per two rows
    auto read_csum = [&](int stage, int s) {
        f32x2 v = {0.f, 0.f};
        if (CSUM) {
            const float* c = cs_base + stage * STAGE + 2 * s * LDT;
            v[0] = c[0];
            v[1] = c[LDT];
        }
        return v;
    };

    const int nslab = (nrows + W_BK - 1) / W_BK;
    if (nslab > 0) {
#pragma unroll
        for (int s = 0; s < 8; ++s) load_slot(0, s);
#pragma unroll
        for (int s = 0; s < 8; ++s) store_slot(0, s);
#pragma unroll
        for (int s = 0; s < 8; ++s) load_slot(1, s);
        for (int t = 0; t < nslab; ++t) {
            const int stage = t & 1;
            __syncthreads();
            Frag cur = read_frag(stage, 0);
            f32x2 cv = read_csum(stage, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                Frag nxt;
                f32x2 cvn;
                if (s < 15) { nxt = read_frag(stage, s + 1); cvn = read_csum(stage, s + 1); }
                if (s < 8) {                       // slab t + 1 -> the other stage, slab t + 2 requested into the freed registers
                    store_slot(stage ^ 1, s);
                    load_slot(t + 2, s);
                }
                if (CSUM) csum2 += cv;             // (read one k step ahead, as the fragments: no wait in front of the add)
                mfma(cur);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                       // MFMA
                    if (r < (CSUM ? 6 : 4)) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read (4 fragment pairs, 2 column-sum rows)
                    else if (r >= 8 && r < 10) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);    // DS write
                    else if (r >= 10 && r < 12) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
                    __builtin_amdgcn_sched_group_barrier(0x006, 2, 0);                       // VALU | SALU
                }
                if (s < 15) { cur = nxt; cv = cvn; }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const long stride = (long)a.Nout * a.Nin + (CSUM ? a.Nout : 0);
    float* out = a.slab + (long)chunk * stride;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int i = i0 + wr * 128 + mi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) out[(long)i * a.Nin + wc * 128 + ni * 32 + lr] = acc[mi][ni][reg];
        }
    if (CSUM) out[(long)a.Nout * a.Nin + i0 + tid] = csum2[0] + csum2[1];
}

// Generic fallback (scalar-guarded loads) for operands that are not 16-byte tileable, e.g. the (N, O) head gradient.
template <int BNW>   // 128: waves 2x2, each 2x2 MFMA tiles;  32: waves 4x1, each one MFMA tile
__global__ __launch_bounds__(256, 2) void wgrad_kernel_generic(WgradArgs a) {
    constexpr int WM = BNW == 128 ? 2 : 1, WN = BNW == 128 ? 2 : 1;
    constexpr int LDQ = BNW + 4;
    constexpr int P_TILE = W_BK * W_LDP, Q_TILE = W_BK * LDQ;
    constexpr int QSLOTS = (W_BK * BNW / 4) / 256;          // float4 slots per thread for Q (4 or 1)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int wr = BNW == 128 ? (wid >> 1) : wid, wc = BNW == 128 ? (wid & 1) : 0;
    const int tiles_i = (a.Nout + 127) / 128, tiles_j = (a.Nin + BNW - 1) / BNW;
    const int tile = blockIdx.x % (tiles_i * tiles_j), chunk = blockIdx.x / (tiles_i * tiles_j);
    const int i0 = (tile / tiles_j) * 128, j0 = (tile % tiles_j) * BNW;
    const WgradRows rows = wgrad_chunk_rows(a, chunk);
    const long r0 = rows.r0, r1 = rows.r1;
    const bool vecP = (a.ldp % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.P) & 15) == 0);
    const bool vecQ = (a.ldq % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.Q) & 15) == 0);

    f32x16 acc[WM][WN];      // (zero_acc, written out: through the helper the compiler scheduled this kernel differently)
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float csum = 0.f;

    auto load = [&](long k0, float4 (&rp)[4], float4 (&rq)[QSLOTS]) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            int slot = tid + 256 * s;
            long m = k0 + (slot >> 5);
            int i = i0 + 4 * (slot & 31);
            rp[s] = (m < r1 && i < a.Nout) ? ld4_guard(a.P + m * a.ldp + i, a.Nout - i, vecP) : make_float4(0, 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < QSLOTS; ++s) {
            int slot = tid + 256 * s;
            long m = k0 + slot / (BNW / 4);
            int j = j0 + 4 * (slot % (BNW / 4));
            float4 v = (m < r1 && j < a.Nin) ? ld4_guard(a.Q + m * a.ldq + j, a.Nin - j, vecQ) : make_float4(0, 0, 0, 0);
            if (a.q_relu) v = relu4(v);
            rq[s] = v;
        }
    };
    auto store = [&](int stage, const float4 (&rp)[4], const float4 (&rq)[QSLOTS]) {
        float* lp = lds + stage * (P_TILE + Q_TILE);
        float* lq = lp + P_TILE;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            int slot = tid + 256 * s;
            *reinterpret_cast<float4*>(lp + (slot >> 5) * W_LDP + 4 * (slot & 31)) = rp[s];
        }
#pragma unroll
        for (int s = 0; s < QSLOTS; ++s) {
            int slot = tid + 256 * s;
            *reinterpret_cast<float4*>(lq + (slot / (BNW / 4)) * LDQ + 4 * (slot % (BNW / 4))) = rq[s];
        }
    };
    auto compute = [&](int stage) {
        const float* lp = lds + stage * (P_TILE + Q_TILE);
        const float* lq = lp + P_TILE;
#pragma unroll
        for (int kg = 0; kg < 4; ++kg) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = kg * 8 + lh * 4 + j;
                float av[WM], bv[WN];
#pragma unroll
                for (int mi = 0; mi < WM; ++mi) av[mi] = lp[k * W_LDP + wr * (32 * WM) + mi * 32 + lr];
#pragma unroll
                for (int ni = 0; ni < WN; ++ni) bv[ni] = lq[k * LDQ + wc * (32 * WN) + ni * 32 + lr];
#pragma unroll
                for (int mi = 0; mi < WM; ++mi)
#pragma unroll
                    for (int ni = 0; ni < WN; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
            }
        }
        if (a.colsum && j0 == 0 && tid < 128) {
#pragma unroll 8
            for (int k = 0; k < W_BK; ++k) csum += lp[k * W_LDP + tid];
        }
    };

    const long nit = (r1 - r0 + W_BK - 1) / W_BK;
    if (nit > 0) {
        float4 rp[4], rq[QSLOTS];
        load(r0, rp, rq);
        store(0, rp, rq);
        __syncthreads();
        for (long it = 0; it < nit; ++it) {
            const bool more = it + 1 < nit;
            if (more) load(r0 + (it + 1) * W_BK, rp, rq);
            compute((int)(it & 1));
            if (more) store((int)((it + 1) & 1), rp, rq);
            __syncthreads();
        }
    }
    const long stride = (long)a.Nout * a.Nin + (a.colsum ? a.Nout : 0);
    float* out = a.slab + (long)chunk * stride;
#pragma unroll
    for (int mi = 0; mi < WM; ++mi)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            int i = i0 + wr * (32 * WM) + mi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
            if (i < a.Nout) {
#pragma unroll
                for (int ni = 0; ni < WN; ++ni) {
                    int j = j0 + wc * (32 * WN) + ni * 32 + lr;
                    if (j < a.Nin) out[(long)i * a.Nin + j] = acc[mi][ni][reg];
                }
            }
        }
    if (a.colsum && j0 == 0 && tid < 128 && i0 + tid < a.Nout) out[(long)a.Nout * a.Nin + i0 + tid] = csum;
}

int launch_wgrad_fp32(const WgradPick& p, const WgradArgs& a, hipStream_t st) {
    switch (p.kernel) {
        case WG_SKINNY32: return wgrad_launch<&wgrad_kernel<32>>(p, a, st);
        case WG_SKINNY32_PBF: return wgrad_launch<&wgrad_kernel<32, true>>(p, a, st);
        case WG_MID64: return wgrad_launch<&wgrad_kernel<64>>(p, a, st);                   // 51 200 B of dynamic LDS
        case WG_WIDE128: return wgrad_launch<&wgrad_kernel<128>>(p, a, st);
        case WG_WIDE3: return wgrad_launch<&wgrad3_kernel>(p, a, st);
        case WG_GENERIC32: return wgrad_launch<&wgrad_kernel_generic<32>>(p, a, st);
        case WG_GENERIC128: return wgrad_launch<&wgrad_kernel_generic<128>>(p, a, st);
        case WG_WAVE:                                                                       // 133 120 B of dynamic LDS
            return a.colsum ? wgrad_launch<&wgrad_wave_kernel<true>>(p, a, st) : wgrad_launch<&wgrad_wave_kernel<false>>(p, a, st);
        default: REGT_CHECK_ARG(false, "wgrad: kernel %d is not an fp32-MFMA kernel", (int)p.kernel);
    }
    return REGT_OK;
}

}  // namespace regt
