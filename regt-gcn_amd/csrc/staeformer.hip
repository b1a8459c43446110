// STAEformer (models/STAEformer.py) inference: the kernels between the dense layers.  Activations are fp32 rows of D = model_dim
// floats in the reference's own order, (B, T, N, D) contiguous: row (b T + t) N + n, M = B T N rows.  Nothing is transposed in
// memory; the dense layers (FC_Q / FC_K / FC_V, out_proj, the two feed-forward linears) run on the GEMMs of gemm_fwd.hip and the
// launch sequence is stae_forward in api_baselines.hip.
//
// stae_attention_kernel: softmax(Q K^T / sqrt(32)) V per (sequence, head), Q / K / V read where the projection GEMMs wrote them
// through one row stride.  axis = 1 (temporal): a sequence is (b, n), L = T, position l is row (b T + l) N + n; axis = 2 (spatial):
// a sequence is (b, t), L = N, position l is row (b T + t) N + l.  Head h owns columns [32 h, 32 h + 32).
//   Mapping.  One wave owns 32 queries of one (sequence, head) and walks the keys in tiles of 32 with an online softmax; the four
//   waves of a workgroup are independent (no LDS, no barrier), consecutive waves take consecutive query tiles of one sequence so
//   that they stream the same K / V rows.  Both contractions run on v_mfma_f32_32x32x2_f32.  The scores are formed TRANSPOSED,
//   S^T = K Q^T: the accumulator then holds, per lane, 16 keys of ONE query (keys crow(i, lh), query lane & 31), so a query's
//   running maximum and sum are 16 in-lane steps and one exchange with lane ^ 32, and P^T is already laid out as the B operand of
//   O^T = V^T P^T -- the key order of that contraction is the accumulator's own, V is read to match, nothing passes through LDS.
//   Padding keys of a ragged last tile get the score -inf and their V is taken as 0 (never loaded); padding queries are computed
//   on zeros and never stored.  Every tile holds at least one real key, so the running maximum is finite from the first tile on.
//   Sums run in a fixed order: two runs give the same bits.  The SAVE_LSE instance is the training forward: the same out, plus
//   each (row, head)'s m + log(l), from which staeformer_bwd.hip rebuilds the probabilities.
//
// stae_add_layernorm_kernel: out = LayerNorm(residual + y) gamma + beta over D (biased variance, as nn.LayerNorm), one wave per
// row, the row held in registers (mean first, then the centred squares); the kernel is the DROP = false instance of the template in
// stae_rows.h, whose DROP = true instance (staeformer_train.hip) applies keep-bit dropout to y; out may alias residual.
//
// stae_embed_kernel: layer 0's input, columns in the reference's concatenation order (models/STAEformer.py:203-229):
// input_proj(x[..., :input_dim]) | tod_embedding[(x[..., 1] steps_per_day).long()] | dow_embedding[x[..., 2].long()] | node_emb |
// adaptive_embedding[t, n]; a block of width 0 is absent.  .long() truncates toward zero; the index is then CLAMPED into its
// table (negative or NaN -> row 0, too large -> the last row), where the reference would raise: nothing outside a table is read.
//
// stae_output_proj_kernel: the use_mixed_proj tail (:237-245), out[b, o, n, c] = sum_{t, d} x[b, t, n, d] W[o output_dim + c, t D + d]
// + bias; one wave per (b, n) reads the node's T pieces at stride N D.
//
// Limits (checked by regt_stae_* before any launch): head width 32; D % 32 == 0, D <= 256.
#include "stae_rows.h"

namespace regt {

namespace {

using namespace stae;

struct AttnArgs {
    const float *q, *k, *v;
    float *out, *lse;                     // lse: (M, H) row statistics m + log(l), written by the SAVE_LSE instance only
    long ld, ldo, nwork;
    int T, N, H, axis, L, qtiles;
};

// SAVE_LSE: the training forward.  Same arithmetic and the same out, bit for bit; each query's log-sum-exp of its scaled scores
// is stored besides, which is all the backward needs to rebuild the probabilities.
template <bool SAVE_LSE>
__global__ __launch_bounds__(THREADS) void stae_attention_kernel(const AttnArgs a) {
    const int lane = threadIdx.x & 63, lr = lane & 31, lh = lane >> 5;
    const long w = (long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (w >= a.nwork) return;                                // the waves share nothing: no barrier follows
    const int qt = (int)(w % a.qtiles);
    const long sh = w / a.qtiles;
    const int h = (int)(sh % a.H);
    const long s = sh / a.H;
    long row0, rstep;                                        // position l of the sequence is row row0 + l * rstep
    if (a.axis == 1) {
        const long b = s / a.N;
        row0 = b * a.T * a.N + (s - b * a.N), rstep = a.N;
    } else {
        row0 = s * a.N, rstep = 1;
    }
    const int L = a.L, col = 32 * h;
    const float scale = 0.17677669529663687f;                // 1 / sqrt(32)

    // this lane's operand slice of its query: columns 16 lh .. 16 lh + 15 (the contraction over d runs in that order on both sides)
    const int ql = qt * QT + lr;
    float qr[16];
    load16(qr, a.q + (row0 + (long)ql * rstep) * a.ld + col + 16 * lh, ql < L);

    f32x16 o;                                                // O^T: d = crow(i, lh), query = lr
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < L; k0 += QT) {
        float kr[16];
        load16(kr, a.k + (row0 + (long)(k0 + lr) * rstep) * a.ld + col + 16 * lh, k0 + lr < L);
        f32x16 st;                                           // S^T: key = k0 + crow(i, lh), query = lr
#pragma unroll
        for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) st = mfma32(kr[j], qr[j], st);
        float vv[16];                                        // V[key crow(i, lh)][d = lr]: issued ahead of the softmax arithmetic
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = k0 + crow(i, lh);
            vv[i] = 0.f;
            if (key < L) vv[i] = a.v[(row0 + (long)key * rstep) * a.ld + col + lr];
        }
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            st[i] = k0 + crow(i, lh) < L ? st[i] * scale : -INFINITY;
            mx = fmaxf(mx, st[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);                       // finite: the tile has a real key
        const float alpha = expf(m - mn);                    // 0 on the first tile
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            st[i] = expf(st[i] - mn);
            sum += st[i];
        }
        sum += __shfl_xor(sum, 32, 64);
        l = l * alpha + sum;
        m = mn;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] *= alpha;
#pragma unroll
        for (int i = 0; i < 16; ++i) o = mfma32(vv[i], st[i], o);
    }
    if (ql < L) {
        const float inv = 1.0f / l;
        float* op = a.out + (row0 + (long)ql * rstep) * a.ldo + col + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(op + 8 * g) = make_float4(o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv);
        if constexpr (SAVE_LSE)
            if (lh == 0) a.lse[(row0 + (long)ql * rstep) * a.H + h] = m + logf(l);
    }
}

struct EmbedArgs {
    const float *x, *w_in, *b_in, *tod, *dow, *node, *adp;
    float* out;
    long total;
    int T, N, F, Cin, e_in, e_tod, e_dow, e_sp, e_adp, D, spd, dpw;
};

__global__ __launch_bounds__(THREADS) void stae_embed_kernel(const EmbedArgs a) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= a.total) return;
    const long mrow = e / a.D;
    int c = (int)(e - mrow * a.D);
    const int n = (int)(mrow % a.N), t = (int)((mrow / a.N) % a.T);
    const float* xr = a.x + mrow * a.F;
    float r;
    if (c < a.e_in) {
        r = 0.f;
        for (int i = 0; i < a.Cin; ++i) r = fmaf(xr[i], a.w_in[c * a.Cin + i], r);
        r += a.b_in[c];
    } else if ((c -= a.e_in) < a.e_tod) {
        r = a.tod[(long)table_index(xr[1] * (float)a.spd, a.spd) * a.e_tod + c];
    } else if ((c -= a.e_tod) < a.e_dow) {
        r = a.dow[(long)table_index(xr[2], a.dpw) * a.e_dow + c];
    } else if ((c -= a.e_dow) < a.e_sp) {
        r = a.node[(long)n * a.e_sp + c];
    } else {
        c -= a.e_sp;
        r = a.adp[((long)t * a.N + n) * a.e_adp + c];
    }
    a.out[e] = r;
}

__global__ __launch_bounds__(THREADS) void stae_output_proj_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                   const float* __restrict__ bias, float* __restrict__ out, int B, int T,
                                                                   int N, int D, int O, int OD) {
    const int lane = threadIdx.x & 63;
    const long node = (long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);       // b N + n
    if (node >= (long)B * N) return;
    const long b = node / N, n = node - b * N;
    const float* xb = x + (b * T * N + n) * D;                                       // piece t at + t N D
    const long tstep = (long)N * D, K = (long)T * D;
    for (int j = 0; j < O * OD; ++j) {
        const float* wj = w + j * K;
        float acc = 0.f;
        for (int t = 0; t < T; ++t)
            for (int d = lane; d < D; d += 64) acc = fmaf(xb[t * tstep + d], wj[t * D + d], acc);
        acc = wave_sum(acc);
        if (lane == 0) out[((b * O + j / OD) * N + n) * OD + j % OD] = acc + bias[j];
    }
}

}  // namespace

// lse == nullptr: the inference instance
int launch_stae_attention(const float* q, const float* k, const float* v, long ld, int B, int T, int N, int heads, int axis, float* out,
                          long ldo, hipStream_t st, float* lse) {
    AttnArgs a{};
    a.q = q, a.k = k, a.v = v, a.out = out, a.lse = lse, a.ld = ld, a.ldo = ldo;
    a.T = T, a.N = N, a.H = heads, a.axis = axis, a.L = axis == 1 ? T : N, a.qtiles = cdiv(a.L, QT);
    a.nwork = (long)B * (axis == 1 ? N : T) * heads * a.qtiles;
    const long blocks = (a.nwork + THREADS / 64 - 1) / (THREADS / 64);
    REGT_CHECK_ARG(blocks < (1L << 31), "stae attention: %ld workgroups exceed the grid", blocks);
    if (lse)
        hipLaunchKernelGGL(stae_attention_kernel<true>, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(stae_attention_kernel<false>, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

int launch_stae_add_layernorm(const float* residual, const float* y, const float* gamma, const float* beta, float eps, long M, int D,
                              float* out, hipStream_t st) {
    const long blocks = (M + THREADS / 64 - 1) / (THREADS / 64);
    REGT_CHECK_ARG(blocks < (1L << 31), "stae add_layernorm: %ld workgroups exceed the grid", blocks);
    hipLaunchKernelGGL(stae_add_layernorm_kernel<false>, dim3((unsigned)blocks), dim3(THREADS), 0, st, residual, y, nullptr, 1.0f, gamma, beta, eps,
                       M, D, out);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

int launch_stae_embed(const StaeDims& s, const float* x, const float* const* P, float* out, hipStream_t st) {
    EmbedArgs a{};
    a.x = x, a.node = P[0], a.adp = P[1], a.w_in = P[2], a.b_in = P[3], a.tod = P[4], a.dow = P[5], a.out = out;
    a.T = s.in_steps, a.N = s.num_nodes, a.F = s.in_features, a.Cin = s.input_dim;
    a.e_in = s.e_in, a.e_tod = s.e_tod, a.e_dow = s.e_dow, a.e_sp = s.e_sp, a.e_adp = s.e_adp, a.D = stae_model_dim(s);
    a.spd = s.steps_per_day, a.dpw = s.days_per_week;
    a.total = (long)s.batch * s.in_steps * s.num_nodes * a.D;
    const long blocks = (a.total + THREADS - 1) / THREADS;
    REGT_CHECK_ARG(blocks < (1L << 31), "stae embed: %ld workgroups exceed the grid", blocks);
    hipLaunchKernelGGL(stae_embed_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, a);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

int launch_stae_output_proj(const StaeDims& s, const float* x, const float* w, const float* bias, float* out, hipStream_t st) {
    const long nodes = (long)s.batch * s.num_nodes;
    hipLaunchKernelGGL(stae_output_proj_kernel, dim3((unsigned)((nodes + THREADS / 64 - 1) / (THREADS / 64))), dim3(THREADS), 0, st, x, w, bias,
                       out, s.batch, s.in_steps, s.num_nodes, stae_model_dim(s), s.out_steps, s.output_dim);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace regt
