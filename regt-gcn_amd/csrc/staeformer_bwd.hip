// STAEformer training: the backward kernels between the dense layers.  Layout as in staeformer.hip: fp32 rows (b T + t) N + n, a
// sequence read through a row stride, head h owns columns [32 h, 32 h + 32), head width 32 only.
//
// Attention backward.  With scale = 1 / sqrt(32), LSE_i = log sum_j exp(scale q_i.k_j) from the training forward
// (stae_attention_kernel<true>) and delta_i = sum_d dO[i, d] O[i, d]:
//     P_ij = exp(scale q_i.k_j - LSE_i)    dP_ij = dO_i.v_j    dS_ij = P_ij (dP_ij - delta_i)
//     dQ_i = scale sum_j dS_ij k_j         dK_j = scale sum_i dS_ij q_i         dV_j = sum_i P_ij dO_i
// Two owner passes, each a wave per 32 rows of one (sequence, head) on v_mfma_f32_32x32x2_f32, no LDS, no barrier, no atomics, no
// score matrix in memory; every sum has a fixed order, two runs give the same bits.
//   stae_attention_dq_kernel: a wave owns 32 QUERIES and walks the key tiles.  As in the forward the products are formed
//   transposed, S^T = K Q^T and dP^T = V dO^T: a lane holds 16 keys (crow(i, lh)) of ONE query (lane & 31), so LSE and delta of that
//   query are lane scalars, and dS^T is already the B operand of dQ^T = K^T dS^T, with K read a second time in the accumulator's
//   key order (as V is in the forward).  delta is an in-lane sum over the lane's 16 columns plus one exchange with lane ^ 32; the
//   pass leaves it in the scratch (M x heads floats) for the second pass.
//   stae_attention_dkv_kernel: a wave owns 32 KEYS and walks the query tiles.  S = Q K^T and dP = dO V^T give 16 queries of one
//   key per lane; LSE and delta of those 16 queries are loaded per tile; P and dS are the B operands of dV^T = dO^T P and
//   dK^T = Q^T dS, with dO and Q read a second time in the accumulator's query order.
//   Ragged tiles.  A padding key has P forced to 0 and its K, V taken as 0 (never loaded), so dS = 0 (0 - delta) = 0 exactly.  A
//   padding query has Q, dO, LSE and delta taken as 0 (never loaded) and P forced to 0 in the key pass, so it adds exactly zero to
//   dK and dV; in the query pass its lanes compute exp(0 - 0) (0 - 0) = 0 and are never stored.  Nothing that was not loaded or
//   set reaches an exp or a product.
//   A sequence of ONE position (L = 1) has the constant softmax 1: dQ and dK are structurally zero and dV = dO.  Both passes take
//   P = 1 and dS = 0 as such there; rebuilt from lse and delta they would leave a rounding residue of 1e-7 where float64 has 0.
//
// Add+LayerNorm backward.  One wave per row recomputes z = residual + y, its mean and rstd with the forward's own code
// (ln_centre_row), x^ = (z - mean) rstd, g = dout gamma, and writes dz = rstd (g - mean(g) - x^ mean(g x^)), the gradient of both
// residual and y.  x^ comes from the inputs: nothing is divided by gamma.  dgamma = sum_rows dout x^ and dbeta = sum_rows dout: a
// wave carries its 16 consecutive rows in registers and writes one partial row of 2 D floats; slab_reduce_tree then sums each
// column's partials in 256 interleaved running sums combined pairwise (the split csrc/stnorm.hip's op_accumulate uses, for the
// same reason: one running sum over all M rows loses the bits a cancelling column needs).  The kernel is a template of stae_rows.h:
// its DROP instance also writes dy = keep dz s, the gradient of a branch that went through keep-bit dropout, in the same pass.  The
// column reduction (launch_stae_col_reduce) also serves the embedding and output-projection gradients of staeformer_train.hip.
#include "slab_reduce.h"
#include "stae_rows.h"

namespace regt {

namespace {

using namespace stae;

constexpr float SCALE = 0.17677669529663687f;                // 1 / sqrt(32)

struct AttnBwdArgs {
    const float *q, *k, *v, *out, *dout, *lse;
    float *dq, *dk, *dv, *delta;
    long ld, ldo, ldg, nwork;
    int T, N, H, axis, L, tiles;
};

// the wave's (tile, head, sequence): tile index returned, head and the sequence's first row / row step through the references
__device__ __forceinline__ int attn_work(const AttnBwdArgs& a, long w, int& h, long& row0, long& rstep) {
    const int tile = (int)(w % a.tiles);
    const long sh = w / a.tiles;
    h = (int)(sh % a.H);
    const long s = sh / a.H;
    if (a.axis == 1) {
        const long b = s / a.N;
        row0 = b * a.T * a.N + (s - b * a.N), rstep = a.N;
    } else {
        row0 = s * a.N, rstep = 1;
    }
    return tile;
}

// accumulator register i holds element (d = crow(i, lh), row lr) of a transposed 32 x 32 result: the row's columns 4 lh + 8 g + (0..3)
__device__ __forceinline__ void store_rows(float* p, const f32x16& o, float f) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(p + 8 * g) = make_float4(o[4 * g] * f, o[4 * g + 1] * f, o[4 * g + 2] * f, o[4 * g + 3] * f);
}

__global__ __launch_bounds__(THREADS) void stae_attention_dq_kernel(const AttnBwdArgs a) {
    const int lane = threadIdx.x & 63, lr = lane & 31, lh = lane >> 5;
    const long w = (long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (w >= a.nwork) return;                                // the waves share nothing: no barrier follows
    int h;
    long row0, rstep;
    const int qt = attn_work(a, w, h, row0, rstep);
    const int L = a.L, col = 32 * h;

    // this lane's slice of its query's rows: columns 16 lh .. 16 lh + 15 of Q, dO and O
    const int ql = qt * QT + lr;
    const bool qlive = ql < L;
    const long qrow = row0 + (long)ql * rstep;               // only used where qlive
    float qr[16], dor[16];
    float delta = 0.f, lse = 0.f;
    {
        float orow[16];
        load16(qr, a.q + qrow * a.ld + col + 16 * lh, qlive);
        load16(dor, a.dout + qrow * a.ldo + col + 16 * lh, qlive);
        load16(orow, a.out + qrow * a.ldo + col + 16 * lh, qlive);
#pragma unroll
        for (int j = 0; j < 16; ++j) delta = fmaf(dor[j], orow[j], delta);
        delta += __shfl_xor(delta, 32, 64);
        if (qlive) {
            lse = a.lse[qrow * a.H + h];
            if (lh == 0) a.delta[qrow * a.H + h] = delta;
        }
    }

    const bool single = L == 1;
    f32x16 acc;                                              // dQ^T: d = crow(i, lh), query = lr
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < L; k0 += QT) {
        const bool klive = k0 + lr < L;
        const long krow = row0 + (long)(k0 + lr) * rstep;
        float kr[16], vr[16];
        load16(kr, a.k + krow * a.ld + col + 16 * lh, klive);
        load16(vr, a.v + krow * a.ld + col + 16 * lh, klive);
        f32x16 st, dpt;                                      // S^T, dP^T: key = k0 + crow(i, lh), query = lr
#pragma unroll
        for (int i = 0; i < 16; ++i) st[i] = 0.f, dpt[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) st = mfma32(kr[j], qr[j], st);
#pragma unroll
        for (int j = 0; j < 16; ++j) dpt = mfma32(vr[j], dor[j], dpt);
        float kk[16];                                        // K[key crow(i, lh)][d = lr]: issued ahead of the softmax arithmetic
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = k0 + crow(i, lh);
            kk[i] = 0.f;
            if (key < L) kk[i] = a.k[(row0 + (long)key * rstep) * a.ld + col + lr];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float p = k0 + crow(i, lh) < L ? expf(st[i] * SCALE - lse) : 0.f;
            st[i] = single ? 0.f : p * (dpt[i] - delta);     // dS^T
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) acc = mfma32(kk[i], st[i], acc);
    }
    if (qlive) store_rows(a.dq + qrow * a.ldg + col + 4 * lh, acc, SCALE);
}

__global__ __launch_bounds__(THREADS) void stae_attention_dkv_kernel(const AttnBwdArgs a) {
    const int lane = threadIdx.x & 63, lr = lane & 31, lh = lane >> 5;
    const long w = (long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (w >= a.nwork) return;
    int h;
    long row0, rstep;
    const int kt = attn_work(a, w, h, row0, rstep);
    const int L = a.L, col = 32 * h;

    const int kl = kt * QT + lr;
    const bool klive = kl < L;
    const long krow = row0 + (long)kl * rstep;               // only used where klive
    float kr[16], vr[16];
    load16(kr, a.k + krow * a.ld + col + 16 * lh, klive);
    load16(vr, a.v + krow * a.ld + col + 16 * lh, klive);

    const bool single = L == 1;
    f32x16 dk, dv;                                           // dK^T, dV^T: d = crow(i, lh), key = lr
#pragma unroll
    for (int i = 0; i < 16; ++i) dk[i] = 0.f, dv[i] = 0.f;
    for (int q0 = 0; q0 < L; q0 += QT) {
        const bool qlive = q0 + lr < L;
        const long qrow = row0 + (long)(q0 + lr) * rstep;
        float qr[16], dor[16];
        load16(qr, a.q + qrow * a.ld + col + 16 * lh, qlive);
        load16(dor, a.dout + qrow * a.ldo + col + 16 * lh, qlive);
        f32x16 s, dp;                                        // S, dP: query = q0 + crow(i, lh), key = lr
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f, dp[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) s = mfma32(qr[j], kr[j], s);
#pragma unroll
        for (int j = 0; j < 16; ++j) dp = mfma32(dor[j], vr[j], dp);
        float qq[16], dd[16];                                // Q, dO [query crow(i, lh)][d = lr]
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int query = q0 + crow(i, lh);
            float lse = 0.f, delta = 0.f;
            qq[i] = 0.f, dd[i] = 0.f;
            if (query < L) {
                const long r = row0 + (long)query * rstep;
                qq[i] = a.q[r * a.ld + col + lr];
                dd[i] = a.dout[r * a.ldo + col + lr];
                lse = a.lse[r * a.H + h];
                delta = a.delta[r * a.H + h];
            }
            const float p = (query < L && klive) ? (single ? 1.0f : expf(s[i] * SCALE - lse)) : 0.f;
            s[i] = p;
            dp[i] = single ? 0.f : p * (dp[i] - delta);      // dS
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) dv = mfma32(dd[i], s[i], dv);
#pragma unroll
        for (int i = 0; i < 16; ++i) dk = mfma32(qq[i], dp[i], dk);
    }
    if (klive) {
        store_rows(a.dk + krow * a.ldg + col + 4 * lh, dk, SCALE);
        store_rows(a.dv + krow * a.ldg + col + 4 * lh, dv, 1.0f);
    }
}

}  // namespace

size_t stae_attention_bwd_scratch_floats(long M, int heads) { return (size_t)M * heads; }

size_t stae_add_layernorm_bwd_scratch_floats(long M, int D) { return (size_t)((M + LN_ROWS - 1) / LN_ROWS) * 2 * D; }

int launch_stae_attention_bwd(const float* q, const float* k, const float* v, long ld, const float* out, const float* dout, long ldo,
                              const float* lse, int B, int T, int N, int heads, int axis, float* dq, float* dk, float* dv, long ldg,
                              float* scratch, hipStream_t st) {
    AttnBwdArgs a{};
    a.q = q, a.k = k, a.v = v, a.out = out, a.dout = dout, a.lse = lse, a.dq = dq, a.dk = dk, a.dv = dv, a.delta = scratch;
    a.ld = ld, a.ldo = ldo, a.ldg = ldg;
    a.T = T, a.N = N, a.H = heads, a.axis = axis, a.L = axis == 1 ? T : N, a.tiles = cdiv(a.L, QT);
    a.nwork = (long)B * (axis == 1 ? N : T) * heads * a.tiles;
    const long blocks = (a.nwork + THREADS / 64 - 1) / (THREADS / 64);
    REGT_CHECK_ARG(blocks < (1L << 31), "stae attention backward: %ld workgroups exceed the grid", blocks);
    hipLaunchKernelGGL(stae_attention_dq_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);     // also writes delta
    REGT_CHECK_LAUNCH();
    hipLaunchKernelGGL(stae_attention_dkv_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

// one workgroup per column of the (nparts, width) partials, slab_reduce.h's interleaved-plus-tree order
int launch_stae_col_reduce(const float* partial, long nparts, long width, const SlabSegs& segs, hipStream_t st) {
    REGT_CHECK_ARG(width >= 1 && width < (1L << 31), "stae column reduction: %ld columns exceed the grid", width);
    hipLaunchKernelGGL(slab_reduce_tree<THREADS>, dim3((unsigned)width), dim3(THREADS), 0, st, partial, nparts, width, segs);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

// keep == nullptr: no dropout, dz is the gradient of both inputs and dy is not touched
int launch_stae_add_layernorm_bwd(const float* residual, const float* y, const float* gamma, const float* dout, float eps, long M, int D,
                                  float* dz, float* dgamma, float* dbeta, float* scratch, hipStream_t st, const uint32_t* keep, float s,
                                  float* dy) {
    const long nwaves = (M + LN_ROWS - 1) / LN_ROWS;
    const long blocks = (nwaves + THREADS / 64 - 1) / (THREADS / 64);
    if (keep)
        hipLaunchKernelGGL(stae_add_layernorm_bwd_kernel<true>, dim3((unsigned)blocks), dim3(THREADS), 0, st, residual, y, keep, s, gamma, dout,
                           eps, M, D, dz, dy, scratch);
    else
        hipLaunchKernelGGL(stae_add_layernorm_bwd_kernel<false>, dim3((unsigned)blocks), dim3(THREADS), 0, st, residual, y, nullptr, 1.0f, gamma,
                           dout, eps, M, D, dz, nullptr, scratch);
    REGT_CHECK_LAUNCH();
    SlabSegs segs{};
    add_seg(segs, dgamma, D);
    add_seg(segs, dbeta, D);
    return launch_stae_col_reduce(scratch, nwaves, 2 * D, segs, st);
}

}  // namespace regt
