// Weight gradients out[Nout x Nin] = P^T Q on the bf16 matrix pipe: the bf16-split kernels (exact three-way split, plain bf16 operands,
// operands stored as bf16) and the register-ring kernel for operands stored as bf16 rows, with the launcher that
// instantiates them.  Which one runs: wgrad_dispatch.hip.  (The fp32-MFMA kernels: wgrad_fp32.hip.)
#include "wgrad_common.h"

namespace regt {

// ---- weight gradients on the bf16 matrix pipe (opt-in bf16x3 split, gemm_split.h) ---------------------------
// Same tile (128 x 128), chunking, slab output and XCD mapping as wgrad_kernel<128>; the K loop follows SplitCore:
// P and Q rows are split exactly into three bf16 planes while they are staged, two 16-row half slabs double-buffer
// each other, six partial products per tile pair.  The operands lie k-major in HBM (row m contiguous along i) and are
// staged exactly so: a [16 m][128 i] bf16 image per plane with 256-byte rows whose 16-byte chunks are XOR-swizzled
// (image (b) of cdna_hip_programming.md T10) -- conflict-free for the ds_write_b64 of the staging pass and for
// ds_read_b64_tr_b16, the transposing LDS read that hands every lane 4 consecutive k of one column: two of them per
// plane make the 8-k operand of v_mfma_f32_32x32x16_bf16 without any shuffle.
// (WS_PLANE_B, one plane of one operand of one half slab: wgrad_common.h)
typedef short s16x4 __attribute__((ext_vector_type(4)));            // what the transposing LDS read returns
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
__device__ __forceinline__ int ws_off(int m, int ch) { return 256 * m + 16 * (ch ^ (((m & 3) << 2) | ((m >> 2) & 3))); }

// One 8-k operand of v_mfma_f32_32x32x16_bf16 for a lane: two transposing reads 4 rows apart in a plane (rows m0, m0 + 4, 16-byte
// chunk ch, byte `sub` inside it), joined
__device__ __forceinline__ bf16x8 ws_read_tr8(const char* plane, int m0, int ch, int sub) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(plane + ws_off(m0, ch) + sub));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(plane + ws_off(m0 + 4, ch) + sub));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// PBF / QBF (NP = 1 only): the operand is STORED as bf16 (dhp, dzp|drp, q: rounded once by their producers).  A half slab
// of such an operand is 16 rows x 128 columns x 2 B = 4 KB = one 16-byte load per thread (row tid >> 4, columns 8 (tid & 15)
// ..+7) that goes to LDS as it is: the chunk layout of ws_off already is 8 bf16 per 16 bytes.
template <int NP, bool PBF = false, bool QBF = false>   // NP 3: exact 3-way split; 1: plain bf16 operands (REGT_GEMM_MODE=bf16)
__global__ __launch_bounds__(256, 2) void wgrad_split_kernel(WgradArgs a) {
    static_assert(NP == 1 || (!PBF && !QBF), "bf16-stored operands only with the plain bf16 arithmetic");
    constexpr int WS_OPER_B = NP * WS_PLANE_B;       // 12288 / 4096
    constexpr int WS_STAGE_B = 2 * WS_OPER_B;        // P planes, then Q planes
    constexpr int WS_RED_B = 256 * 16;               // column-sum reduction image
    static_assert(2 * WS_STAGE_B >= WS_RED_B, "column-sum image fits the stages");
    using Core = FastCore<true, false>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    char* ldsb = reinterpret_cast<char*>(lds);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int wr = wid >> 1, wc = wid & 1;
    const int tiles_i = (a.Nout + 127) / 128, tiles_j = (a.Nin + 127) / 128;
    const int tpc = tiles_i * tiles_j;
    const WgradBlock blk = wgrad_block(a.nchunks, tpc);
    const int tile = blk.tile, chunk = blk.chunk;
    const int i0 = (tile / tiles_j) * 128, j0 = (tile % tiles_j) * 128;
    long r0, r1;      // (wgrad_chunk_rows, written out: through the helper the compiler scheduled this kernel differently)
    if (a.chunk_tab) { r0 = a.chunk_tab[2 * chunk]; r1 = a.chunk_tab[2 * chunk + 1]; }
    else { r0 = (long)chunk * a.kchunk; r1 = r0 + a.kchunk < a.M ? r0 + a.kchunk : a.M; }
    const int nrows = (int)(r1 - r0);

    f32x16 acc[2][2];
    zero_acc(acc);
    float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);      // column sums of the thread's 4 columns of P over its rows
    float4 csum2 = make_float4(0.f, 0.f, 0.f, 0.f);     // PBF: the thread owns 8 columns (csum: 0-3, csum2: 4-7)
    const bool do_csum = a.colsum && j0 == 0;

    const __amdgpu_buffer_rsrc_t sp = Core::make_srd(reinterpret_cast<const float*>(
        reinterpret_cast<const char*>(a.P) + (PBF ? 2 : 4) * (r0 * a.ldp + i0)));
    const __amdgpu_buffer_rsrc_t sq = Core::make_srd(reinterpret_cast<const float*>(
        reinterpret_cast<const char*>(a.Q) + (QBF ? 2 : 4) * (r0 * a.ldq + j0)));
    const int ldp = (int)a.ldp, ldq = (int)a.ldq;
    const int c4 = tid & 31;                             // fp32 operand: the thread's float4 column (4 i's)
    const int c8 = tid & 15;                             // bf16 operand: the thread's 16-byte chunk (8 i's)
    const bool okp = PBF ? i0 + 8 * c8 < a.Nout : i0 + 4 * c4 < a.Nout;
    // two-part right-hand side [Q | Q2] (fp32, columns >= nin_split come from Q2; the host admits it for Nin <= 128): a wave's
    // lanes straddle the split, so every slot is requested from both descriptors with complementary out-of-range masks
    // (an out-of-range lane returns 0 without touching memory) and the two results are OR-ed
    // (bf16-stored Q: the same with the thread's 8-column chunk; nin_split % 8 == 0, host-checked)
    const bool has_q2 = a.Q2 != nullptr;
    // which operand(s) this column tile reads: 1 = Q only, 2 = Q2 only, 3 = both (the split runs through the tile)
    const int q_tile = !has_q2 || j0 + 128 <= a.nin_split ? 1 : (j0 >= a.nin_split ? 2 : 3);
    const int qcol = QBF ? j0 + 8 * c8 : j0 + 4 * c4;        // first of the thread's columns of [Q | Q2]
    const bool in_q2 = has_q2 && qcol >= a.nin_split;
    const bool okq = qcol < a.Nin && !in_q2;
    const bool okq2 = in_q2 && qcol < a.Nin;
    const int ldq2 = (int)a.ldq2, cq2 = qcol - a.nin_split;
    const __amdgpu_buffer_rsrc_t sq2 = Core::make_srd(has_q2 ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.Q2) + (QBF ? 2 : 4) * (r0 * a.ldq2))
                                                             : a.Q);
    const float qfloor = a.q_relu ? 0.f : -__builtin_inff();

    // fp32 operand: slot s of a thread: half h = s & 1, row 16 h + (tid >> 5) + 8 (s >> 1) of the 32-row slab (registers
    // h and h + 2); bf16 operand: register h holds the 16 raw bytes of row 16 h + (tid >> 4)
    auto load_half = [&](int h, int k0, bool live, float4 (&rp)[4], float4 (&rq)[4]) {
        if (PBF) {
            const int m = k0 + 16 * h + (tid >> 4);
            rp[h] = Core::srd_load(sp, live && m < nrows && okp ? 2u * (unsigned)(m * ldp + 8 * c8) : Core::SRD_OOB);
        }
        if (QBF) {
            const int m = k0 + 16 * h + (tid >> 4);
            float4 q;
            if (q_tile == 2) {               // the whole column tile lies in the second operand: ONE load (workgroup-uniform)
                q = Core::srd_load(sq2, live && m < nrows && okq2 ? 2u * (unsigned)(m * ldq2 + cq2) : Core::SRD_OOB);
            } else {
                q = Core::srd_load(sq, live && m < nrows && okq ? 2u * (unsigned)(m * ldq + 8 * c8) : Core::SRD_OOB);
                if (q_tile == 3) {           // the tile straddles the split: both descriptors, complementary masks
                    const float4 q2 = Core::srd_load(sq2, live && m < nrows && okq2 ? 2u * (unsigned)(m * ldq2 + cq2) : Core::SRD_OOB);
                    q = or4(q, q2);
                }
            }
            rq[h] = q;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = k0 + 16 * h + (tid >> 5) + 8 * j;
            const bool ok = live && m < nrows;
            if (!PBF) rp[h + 2 * j] = Core::srd_load(sp, ok && okp ? 4u * (unsigned)(m * ldp + 4 * c4) : Core::SRD_OOB);
            if (!QBF) {
                float4 q = Core::srd_load(sq, ok && okq ? 4u * (unsigned)(m * ldq + 4 * c4) : Core::SRD_OOB);
                if (has_q2 && !QBF) {
                    const float4 q2 = Core::srd_load(sq2, ok && okq2 ? 4u * (unsigned)(m * ldq2 + cq2) : Core::SRD_OOB);
                    q = or4(q, q2);
                }
                rq[h + 2 * j] = q;
            }
        }
    };
    auto store_half = [&](int h, const float4 (&rp)[4], const float4 (&rq)[4]) {
        char* st = ldsb + h * WS_STAGE_B;
        if (PBF) {
            const float4 raw = rp[h];
            *reinterpret_cast<float4*>(st + ws_off(tid >> 4, c8)) = raw;
            const float4 lo = widen_bf16x4(__float_as_uint(raw.x), __float_as_uint(raw.y));
            const float4 hi = widen_bf16x4(__float_as_uint(raw.z), __float_as_uint(raw.w));
            csum.x += lo.x; csum.y += lo.y; csum.z += lo.z; csum.w += lo.w;
            csum2.x += hi.x; csum2.y += hi.y; csum2.z += hi.z; csum2.w += hi.w;
        }
        if (QBF) *reinterpret_cast<float4*>(st + WS_OPER_B + ws_off(tid >> 4, c8)) = rq[h];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int off = ws_off((tid >> 5) + 8 * j, c4 >> 1) + 8 * (c4 & 1);
            if (!PBF) {
                const float4 p = rp[h + 2 * j];
                csum.x += p.x; csum.y += p.y; csum.z += p.z; csum.w += p.w;
                SplitCore<false, NP>::split_store(st + off, p, WS_PLANE_B);
            }
            if (!QBF) {
                float4 q = rq[h + 2 * j];
                q.x = fmaxf(q.x, qfloor); q.y = fmaxf(q.y, qfloor); q.z = fmaxf(q.z, qfloor); q.w = fmaxf(q.w, qfloor);
                SplitCore<false, NP>::split_store(st + WS_OPER_B + off, q, WS_PLANE_B);
            }
        }
    };
    struct Frags { bf16x8 a[2][NP], b[2][NP]; };
    // lane 4q+p of a 16-lane group addresses block row q, columns 4p..4p+3; the group receives 4 k x 16 columns
    // transposed.  Groups 0,1 take columns 0-15 / 16-31 of the 32-column tile at k = 0..3, groups 2,3 the same
    // columns at k = 8..11; a second read 4 rows further down completes the 8-k operand.
    const int gq = (lane >> 2) & 3, gp = lane & 3, gg = lane >> 4;
    auto read_frags = [&](int h) {
        const char* st = ldsb + h * WS_STAGE_B;
        Frags f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int ca = (wr * 64 + t * 32 + 16 * (gg & 1) + 4 * gp) >> 3;      // 16-byte chunk of the lane's 4 columns
            const int cb = (wc * 64 + t * 32 + 16 * (gg & 1) + 4 * gp) >> 3;
            const int sub = 8 * (gp & 1);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int m0 = 8 * (gg >> 1) + gq;
                f.a[t][p] = ws_read_tr8(st + p * WS_PLANE_B, m0, ca, sub);
                f.b[t][p] = ws_read_tr8(st + WS_OPER_B + p * WS_PLANE_B, m0, cb, sub);
            }
        }
        return f;
    };
    auto mfmas = [&](const Frags& f) {
        constexpr int PA[6] = {NP == 3 ? 2 : 0, 1, 0, 1, 0, 0}, PB[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
        for (int q = 0; q < (NP == 3 ? 6 : 1); ++q)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[mi][PA[q]], f.b[ni][PB[q]], acc[mi][ni], 0, 0, 0);
    };
    auto fused = [&](int hs, int hc, int k_next, bool live, float4 (&rp)[4], float4 (&rq)[4]) {
        __builtin_amdgcn_sched_barrier(0);
        const Frags f = read_frags(hc);
        store_half(hs, rp, rq);
        mfmas(f);
        load_half(hs, k_next, live, rp, rq);
        if (NP == 3) {
            __builtin_amdgcn_sched_group_barrier(0x100, 24, 0);
#pragma unroll
            for (int r = 0; r < 24; ++r) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                if (r & 1) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                if (r >= 18 && r < 22) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            }
        } else {
            __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    const int nit = (nrows + 31) / 32;
    if (nit > 0) {
        float4 rp[4], rq[4];
        load_half(0, 0, true, rp, rq);
        load_half(1, 0, true, rp, rq);
        store_half(0, rp, rq);
        store_half(1, rp, rq);
        load_half(0, 32, nit > 1, rp, rq);
        load_half(1, 32, nit > 1, rp, rq);
        __syncthreads();
        mfmas(read_frags(0));
        for (int it = 0; it + 1 < nit; ++it) {
            const bool live = it + 2 < nit;
            __syncthreads();
            fused(0, 1, (it + 2) * 32, live, rp, rq);
            __syncthreads();
            fused(1, 0, (it + 2) * 32, live, rp, rq);
        }
        __syncthreads();
        mfmas(read_frags(1));
    }
    const long stride = (long)a.Nout * a.Nin + (a.colsum ? a.Nout : 0);
    float* out = a.slab + (long)chunk * stride;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            int i = i0 + wr * 64 + mi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
            if (i < a.Nout) {
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    int j = j0 + wc * 64 + ni * 32 + lr;
                    if (j < a.Nin) out[(long)i * a.Nin + j] = acc[mi][ni][reg];
                }
            }
        }
    if (do_csum && !PBF) {      // 8 threads (tid >> 5) hold partial sums of the same 4 columns: fixed-order reduction through LDS
        __syncthreads();
        reinterpret_cast<float4*>(lds)[tid] = csum;
        __syncthreads();
        if (tid < 128 && i0 + tid < a.Nout) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < 8; ++g) s += lds[(g * 32 + (tid >> 2)) * 4 + (tid & 3)];
            out[(long)a.Nout * a.Nin + i0 + tid] = s;
        }
    }
    if (do_csum && PBF) {       // 16 threads (tid >> 4) hold partial sums of the same 8 columns
        __syncthreads();
        reinterpret_cast<float4*>(lds)[2 * tid] = csum;
        reinterpret_cast<float4*>(lds)[2 * tid + 1] = csum2;
        __syncthreads();
        if (tid < 128 && i0 + tid < a.Nout) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) s += lds[(g * 16 + (tid >> 3)) * 8 + (tid & 7)];
            out[(long)a.Nout * a.Nin + i0 + tid] = s;
        }
    }
}

// ---- both operands STORED as bf16 (the bf16-row layout of the cfg-5 path): deep register ring --------------------------------
// Same tile, chunking, LDS image, MFMA and summation order as wgrad_split_kernel<1, true, true> (bit-identical slabs), but the rows
// are requested D half slabs ahead instead of one: a half slab of both operands is 8 KB per workgroup and the K loop consumes one per
// ~0.1 us, so with one half slab of lead every step waited out a full memory latency (wait_any 0.64, 4.1 TB/s).  D half slabs of
// lead keep D x 8 KB per workgroup in flight (Little: 8 TB/s x ~2 us / 256 CUs = 64 KB per CU).  The ring lives in registers
// (two float4 per slot), statically indexed: the K loop is unrolled D times.  A two-part right-hand side [Q | Q2] is taken when the
// split falls on a column-tile boundary (the tile reads one of the two).
// MI = 32-row MFMA tiles of a wave along the output rows: 2 = the 128 x 128 tile of wgrad_split_kernel; 4 = a 256 x 128 tile (the
// left operand's half slab is two 128-column images, wave row wr reads image wr): a column tile's rows of P cross L2 -> LDS once per
// 256 instead of once per 128 output rows (the paired gradients dhp^T [q | A_hat x], dzr^T [h | A_hat x]: 1088 / 2176 instead of
// 1536 / 3072 operand elements per row and chunk), twice the MFMA work per barrier.  Every output element still sums the same
// products in the same order: the slabs do not depend on MI.
template <int D, int MI>
__global__ __launch_bounds__(256, 2) void wgrad_bf16_ring_kernel(WgradArgs a) {
    static_assert(D >= 2 && D % 2 == 0, "ring depth: even (the LDS stage of a slot is static)");
    static_assert(MI == 2 || MI == 4, "128- or 256-row tile");
    constexpr int NPL = MI / 2;                          // 128-column images of P per half slab
    constexpr int TI = 64 * MI;                          // output rows of a tile
    constexpr int WS_Q_B = NPL * WS_PLANE_B, WS_STAGE_B = (NPL + 1) * WS_PLANE_B;
    using Core = FastCore<true, false>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    char* ldsb = reinterpret_cast<char*>(lds);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int wr = wid >> 1, wc = wid & 1;
    const int tiles_i = (a.Nout + TI - 1) / TI, tiles_j = (a.Nin + 127) / 128;
    const int tpc = tiles_i * tiles_j;
    const WgradBlock blk = wgrad_block(a.nchunks, tpc);
    const int tile = blk.tile, chunk = blk.chunk;
    const int i0 = (tile / tiles_j) * TI, j0 = (tile % tiles_j) * 128;
    long r0, r1;      // (wgrad_chunk_rows, written out: through the helper the compiler scheduled this kernel differently)
    if (a.chunk_tab) { r0 = a.chunk_tab[2 * chunk]; r1 = a.chunk_tab[2 * chunk + 1]; }
    else { r0 = (long)chunk * a.kchunk; r1 = r0 + a.kchunk < a.M ? r0 + a.kchunk : a.M; }
    const int nrows = (int)(r1 - r0);

    f32x16 acc[MI][2];
    zero_acc(acc);
    float4 csum[NPL][2];                                 // column sums of the thread's 8 columns of each image over its rows
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) csum[pl][0] = csum[pl][1] = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool do_csum = a.colsum && j0 == 0;

    const bool second = a.Q2 != nullptr && j0 >= a.nin_split;        // workgroup-uniform: this column tile lies in Q2
    const int ldp = (int)a.ldp, ldq = second ? (int)a.ldq2 : (int)a.ldq;
    // Descriptors that END with the chunk's last row: a row past the chunk is out of range by itself (the hardware returns zeros
    // without touching memory), so the K loop carries no row test -- one running byte offset per operand.  A thread whose columns
    // lie outside the matrix starts at 2^31: beyond every range the host admits (chunk rows x row bytes < 2^31), and the walk
    // ((rows + 32 + 16 D) x row bytes) cannot wrap it back into range.
    auto chunk_srd = [](const char* base, unsigned bytes) {
        const unsigned long long v = reinterpret_cast<unsigned long long>(base);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0,
                                                 (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t sp = chunk_srd(reinterpret_cast<const char*>(a.P) + 2 * (r0 * a.ldp + i0), 2u * (unsigned)nrows * (unsigned)ldp);
    const __amdgpu_buffer_rsrc_t sq = chunk_srd(second ? reinterpret_cast<const char*>(a.Q2) + 2 * (r0 * a.ldq2 + (j0 - a.nin_split))
                                                       : reinterpret_cast<const char*>(a.Q) + 2 * (r0 * a.ldq + j0), 2u * (unsigned)nrows * (unsigned)ldq);
    const int c8 = tid & 15, mrow = tid >> 4;            // the thread's 16-byte chunk (8 columns) and row of a half slab
    constexpr unsigned MASKED = 0x80000000u;
    // (MI = 4 is launched for Nout % 256 == 0 only: both images of P lie inside the matrix)
    unsigned vp = i0 + 8 * c8 < a.Nout ? 2u * (unsigned)(mrow * ldp + 8 * c8) : MASKED;      // running byte offsets: half slab g
    unsigned vq = j0 + 8 * c8 < a.Nin ? 2u * (unsigned)(mrow * ldq + 8 * c8) : MASKED;
    const unsigned stepp = 32u * (unsigned)ldp, stepq = 32u * (unsigned)ldq;                   // bytes per half slab (16 rows)

    float4 rp[D][NPL], rq[D];
    auto load = [&](int slot) {                          // the NEXT half slab of the chunk (requests are issued in row order)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) rp[slot][pl] = Core::srd_load(sp, vp + 256u * pl);
        rq[slot] = Core::srd_load(sq, vq);
        vp += stepp;
        vq += stepq;
        asm volatile("" : "+v"(vp), "+v"(vq));           // ONE running offset per operand (not one per unrolled slot)
    };
    const int lds_w = ws_off(mrow, c8);
    struct Frags { bf16x8 a[MI], b[2]; };
    const int gq = (lane >> 2) & 3, gp = lane & 3, gg = lane >> 4;
    auto read_frags = [&](int stage) {
        const char* st = ldsb + stage * WS_STAGE_B;
        Frags f;
        const int sub = 8 * (gp & 1);
        const int m0 = 8 * (gg >> 1) + gq;
#pragma unroll
        for (int t = 0; t < MI; ++t) {
            const int col = wr * (32 * MI) + t * 32;         // first column of the wave's tile t in the 64 MI-column left operand
            const int ca = ((col & 127) + 16 * (gg & 1) + 4 * gp) >> 3;
            const char* pl = st + (col >> 7) * WS_PLANE_B;
            f.a[t] = ws_read_tr8(pl, m0, ca, sub);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int cb = (wc * 64 + t * 32 + 16 * (gg & 1) + 4 * gp) >> 3;
            f.b[t] = ws_read_tr8(st + WS_Q_B, m0, cb, sub);
        }
        return f;
    };
    auto mfmas = [&](const Frags& f, int half) {             // half 0 / 1: the first / last MI / 2 row tiles
#pragma unroll
        for (int m = 0; m < MI / 2; ++m)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int mi = half * (MI / 2) + m;
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[mi], f.b[ni], acc[mi][ni], 0, 0, 0);
            }
    };

    const int G = 2 * ((nrows + 31) / 32);               // half slabs, the last one possibly all zero (as wgrad_split_kernel walks them)
    // The K loop exists twice: with the column sums of P (the workgroups of column tile 0 when a bias gradient is asked for) and
    // without -- 12 of a step's ~30 vector instructions, and the loop is bound by instruction issue once the ring hides the latency.
    auto k_loop = [&](auto cs_tag) {
        constexpr bool CS = decltype(cs_tag)::value;
        auto store = [&](int slot, int stage) {
            char* st = ldsb + stage * WS_STAGE_B;
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) {
                const float4 raw = rp[slot][pl];
                *reinterpret_cast<float4*>(st + pl * WS_PLANE_B + lds_w) = raw;
                if (CS) {
                    const float4 lo = widen_bf16x4(__float_as_uint(raw.x), __float_as_uint(raw.y));
                    const float4 hi = widen_bf16x4(__float_as_uint(raw.z), __float_as_uint(raw.w));
                    float4& c0 = csum[pl][0];
                    float4& c1 = csum[pl][1];
                    c0.x += lo.x; c0.y += lo.y; c0.z += lo.z; c0.w += lo.w;
                    c1.x += hi.x; c1.y += hi.y; c1.z += hi.z; c1.w += hi.w;
                    // pins the sums to this place (instruction selection otherwise sinks the whole chain to the end of the unrolled
                    // turn, keeping every slot's old rows alive past its reload)
                    asm volatile("" : "+v"(c0.x), "+v"(c0.y), "+v"(c0.z), "+v"(c0.w), "+v"(c1.x), "+v"(c1.y), "+v"(c1.z), "+v"(c1.w));
                }
            }
            *reinterpret_cast<float4*>(st + WS_Q_B + lds_w) = rq[slot];
        };
#pragma unroll
        for (int u = 0; u < D; ++u) load(u);
        store(0, 0);
        load(0);
        // step g: multiply half slab g (stage g & 1) while half slab g + 1 goes to the other stage and g + 1 + D is requested
        auto step = [&](int u) {
            const int sn = (u + 1) % D;
            __syncthreads();
            __builtin_amdgcn_sched_barrier(0);
            const Frags f = read_frags(u & 1);
            store(sn, (u + 1) & 1);
            mfmas(f, 0);
            // the slot's old contents are consumed (LDS write, column sums) before it is requested again: if the scheduler lets the two
            // live ranges overlap, the new rows land in other registers and are COPIED into the slot at the loop's back edge -- behind a
            // wait for the whole ring
            __builtin_amdgcn_sched_barrier(0);
            load(sn);
            mfmas(f, 1);
            __builtin_amdgcn_sched_barrier(0);
        };
        // whole turns of the ring as ONE basic block (a test per step gives every step a second predecessor, and the wait-count
        // insertion then assumes the slot's loads are the youngest: vmcnt(0) before every store); the last G % D steps test
        int gb = 0;
        for (; gb + D <= G; gb += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) step(u);
        }
#pragma unroll
        for (int u = 0; u < D - 1; ++u)
            if (gb + u < G) step(u);
    };
    if (G > 0) {
        if (do_csum || a.all_csum) k_loop(std::true_type{});
        else k_loop(std::false_type{});
    }
    const long stride = (long)a.Nout * a.Nin + (a.colsum ? a.Nout : 0);
    float* out = a.slab + (long)chunk * stride;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int i = i0 + wr * (32 * MI) + mi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
            if (i < a.Nout) {
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const int j = j0 + wc * 64 + ni * 32 + lr;
                    if (j < a.Nin) out[(long)i * a.Nin + j] = acc[mi][ni][reg];
                }
            }
        }
    if (do_csum) {       // 16 threads (tid >> 4) hold partial sums of the same 8 columns of an image: fixed-order sum through LDS
        __syncthreads();
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
            reinterpret_cast<float4*>(lds)[512 * pl + 2 * tid] = csum[pl][0];
            reinterpret_cast<float4*>(lds)[512 * pl + 2 * tid + 1] = csum[pl][1];
        }
        __syncthreads();
        if (tid < 128 * NPL && i0 + tid < a.Nout) {
            const int pl = tid >> 7, c = tid & 127;
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) s += lds[2048 * pl + (g * 16 + (c >> 3)) * 8 + (c & 7)];
            out[(long)a.Nout * a.Nin + i0 + tid] = s;
        }
    }
}

int launch_wgrad_bf16(const WgradPick& p, const WgradArgs& a, hipStream_t st) {
    switch (p.kernel) {
        case WG_SPLIT3: return wgrad_launch<&wgrad_split_kernel<3>>(p, a, st);
        case WG_SPLIT1: return wgrad_launch<&wgrad_split_kernel<1, false, false>>(p, a, st);
        case WG_SPLIT1_QBF: return wgrad_launch<&wgrad_split_kernel<1, false, true>>(p, a, st);
        case WG_SPLIT1_PBF: return wgrad_launch<&wgrad_split_kernel<1, true, false>>(p, a, st);
        case WG_SPLIT1_PBF_QBF: return wgrad_launch<&wgrad_split_kernel<1, true, true>>(p, a, st);
        case WG_RING_4_2: return wgrad_launch<&wgrad_bf16_ring_kernel<4, 2>>(p, a, st);
        case WG_RING_6_2: return wgrad_launch<&wgrad_bf16_ring_kernel<6, 2>>(p, a, st);
        case WG_RING_8_2: return wgrad_launch<&wgrad_bf16_ring_kernel<8, 2>>(p, a, st);
        case WG_RING_2_4: return wgrad_launch<&wgrad_bf16_ring_kernel<2, 4>>(p, a, st);
        case WG_RING_4_4: return wgrad_launch<&wgrad_bf16_ring_kernel<4, 4>>(p, a, st);
        default: REGT_CHECK_ARG(false, "wgrad: kernel %d is not a bf16-pipe kernel", (int)p.kernel);
    }
    return REGT_OK;
}

}  // namespace regt
