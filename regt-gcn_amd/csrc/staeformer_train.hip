// STAEformer whole-model training: what the trainable layer (staeformer_bwd.hip) leaves open.  Layout as in staeformer.hip: fp32 rows
// (b T + t) N + n of D = model_dim floats, M = B T N rows.  All three pieces are bandwidth-bound; no float atomics, every sum has a
// fixed order (two runs give the same bits), nothing outside the documented windows is written.
//
// Dropout folded into add+LayerNorm (models/STAEformer.py:98-104: dropout on the branch just before ln(residual + out)).  keep is
// (M, D / 32) words, bit j of word w keeps column 32 w + j (the STID / SpatialGCN convention), s = 1 / (1 - p):
//     forward   out = LayerNorm(residual + keep y s) gamma + beta
//     backward  dz (gradient of residual), dgamma, dbeta as without dropout, and dy = keep dz s as a second M x D store of the same
//               pass: it feeds the data-gradient GEMM of out_proj / feed_forward.2, so it has to exist in memory; dz is not re-read.
// Both are the DROP instances of the templates in stae_rows.h, whose other instances are the kernels without dropout.
// Byte floor: forward 3 M D + M D / 32 floats (plain: 3 M D), backward 5 M D + M D / 32 (plain: 4 M D).
//
// Embedding backward (stae_embed_kernel's transpose), given x (B, T, N, F) and dX0 (M, D); no gradient for x.
//   stae_embed_bwd_chunk_kernel: input_proj weight / bias and the two tables.  A workgroup owns R consecutive rows and one thread
//   per column of the first three blocks; the thread walks its rows IN ROW ORDER and adds into cells of an LDS image
//   [w (E, input_dim) | b (E) | tod (steps_per_day, e_tod) | dow (days_per_week, e_dow)] that only it touches.  A table row's cell
//   is chosen by table_index, the forward's own clamp (negative or NaN -> row 0, too large -> the last row); cells nobody hits stay
//   exactly 0.  The image goes out as one partial row of P floats; launch_stae_col_reduce sums the partials in a fixed order.
//   P <= STAE_EMBED_BWD_MAX_LDS (the image must fit the LDS); R is a multiple of 64 with P <= R D / 4, so the partials cost at most
//   a quarter of the floats read.
//   stae_embed_bwd_owner_kernel: node_emb (N, S) = sum over (b, t) and adaptive_embedding (T, N, A) = sum over b, one thread per
//   output element, which adds its column of dX0 in (b, t) order.
//   Byte floor: x and dX0 read once (M (F + D) floats); the outputs are small.
//
// Output projection backward (use_mixed_proj), J = out_steps * output_dim <= 64, K = T D, dout[b, j, n] read through strides:
//     dX[b, t, n, d] = sum_j dout[b, j, n] W[j, t D + d]    dW[j, t D + d] = sum_{b, n} dout[b, j, n] X[b, t, n, d]    db[j] = sum dout
//   stae_output_proj_bwd_kernel: a workgroup owns (chunk of NCH (b, n) pairs, t) and one thread per column d.  The thread holds
//   W[:, t D + d] and its J running sums of dW in registers; per (b, n) it reads X once, writes dX once and takes the pair's J dout
//   values from an LDS tile (64 pairs at a time).  Partials (nchunks, J K + J) go through launch_stae_col_reduce: 256 interleaved
//   running sums combined pairwise, because one running sum over all B N pairs loses the bits a cancelling column needs.  NCH = 64
//   ceil(J / 16): the partials cost at most an eighth of the floats moved.
//   Byte floor: X read once, dX written once (2 M D floats), W and dW touched once (2 J K).
#include "slab_reduce.h"
#include "stae_rows.h"

namespace regt {

namespace {

using namespace stae;

struct EmbedBwdArgs {
    const float *x, *dx0;
    float* partial;
    long M;
    int F, Cin, e_in, e_tod, e_dow, D, spd, dpw, R, P;
};

__global__ __launch_bounds__(THREADS) void stae_embed_bwd_chunk_kernel(const EmbedBwdArgs a) {
    extern __shared__ float image[];                         // [w | b | tod | dow], P floats
    for (int i = threadIdx.x; i < a.P; i += blockDim.x) image[i] = 0.f;
    __syncthreads();
    float* lw = image;
    float* lb = lw + a.e_in * a.Cin;
    float* ltod = lb + a.e_in;
    float* ldow = ltod + a.spd * a.e_tod;
    int c = threadIdx.x;
    const long r0 = (long)blockIdx.x * a.R, r1 = r0 + a.R < a.M ? r0 + a.R : a.M;
    if (c < a.e_in) {
        for (long row = r0; row < r1; ++row) {
            const float* xr = a.x + row * a.F;
            const float g = a.dx0[row * a.D + c];
            lb[c] += g;
            for (int i = 0; i < a.Cin; ++i) lw[c * a.Cin + i] = fmaf(g, xr[i], lw[c * a.Cin + i]);
        }
    } else if (c < a.e_in + a.e_tod) {
        const int col = c - a.e_in;
        for (long row = r0; row < r1; ++row)
            ltod[table_index(a.x[row * a.F + 1] * (float)a.spd, a.spd) * a.e_tod + col] += a.dx0[row * a.D + c];
    } else if (c < a.e_in + a.e_tod + a.e_dow) {
        const int col = c - a.e_in - a.e_tod;
        for (long row = r0; row < r1; ++row) ldow[table_index(a.x[row * a.F + 2], a.dpw) * a.e_dow + col] += a.dx0[row * a.D + c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.P; i += blockDim.x) a.partial[(long)blockIdx.x * a.P + i] = image[i];
}

// element e < N S: node_emb[n, c]; then adaptive_embedding[t, n, c]
__global__ __launch_bounds__(THREADS) void stae_embed_bwd_owner_kernel(const float* __restrict__ dx0, int B, int T, int N, int D, int e_sp,
                                                                       int e_adp, int off_sp, float* __restrict__ dnode,
                                                                       float* __restrict__ dadp) {
    long e = (long)blockIdx.x * THREADS + threadIdx.x;
    const long n_sp = (long)N * e_sp, n_adp = (long)T * N * e_adp;
    if (e < n_sp) {
        const long n = e / e_sp;
        const int c = (int)(e - n * e_sp);
        float s = 0.f;
        for (long bt = 0; bt < (long)B * T; ++bt) s += dx0[(bt * N + n) * D + off_sp + c];
        dnode[e] = s;
    } else if ((e -= n_sp) < n_adp) {
        const long tn = e / e_adp;                           // t N + n
        const int c = (int)(e - tn * e_adp);
        float s = 0.f;
        for (long b = 0; b < B; ++b) s += dx0[(b * T * N + tn) * D + off_sp + e_sp + c];
        dadp[e] = s;
    }
}

constexpr int OP_SUB = 64;                                   // (b, n) pairs per LDS tile of dout

struct OutProjBwdArgs {
    const float *x, *w, *dout;
    float *dx, *partial;
    long sb, so, sn, sc, nodes, PW;
    int T, N, D, J, OD, NCH;
};

template <int JT>
__global__ __launch_bounds__(THREADS) void stae_output_proj_bwd_kernel(const OutProjBwdArgs a) {
    __shared__ float sd[OP_SUB * JT];                        // dout[pair][j], zeros past J
    const int tid = threadIdx.x, d = tid, t = blockIdx.y;
    const bool live = d < a.D;
    const long K = (long)a.T * a.D;
    const long node0 = (long)blockIdx.x * a.NCH, node1 = node0 + a.NCH < a.nodes ? node0 + a.NCH : a.nodes;
    float w[JT], acc[JT];
#pragma unroll
    for (int j = 0; j < JT; ++j) {
        w[j] = (live && j < a.J) ? a.w[j * K + (long)t * a.D + d] : 0.f;
        acc[j] = 0.f;
    }
    float dbacc = 0.f;
    for (long s0 = node0; s0 < node1; s0 += OP_SUB) {
        const int ns = (int)(node1 - s0 < OP_SUB ? node1 - s0 : OP_SUB);
        __syncthreads();                                     // the previous tile has been read
        for (int i = tid; i < ns * JT; i += blockDim.x) {
            const int j = i / ns, ln = i - j * ns;           // consecutive threads take consecutive pairs of one j
            float g = 0.f;
            if (j < a.J) {
                const long node = s0 + ln, b = node / a.N, n = node - b * a.N;
                g = a.dout[b * a.sb + (j / a.OD) * a.so + n * a.sn + (j % a.OD) * a.sc];
            }
            sd[ln * JT + j] = g;
        }
        __syncthreads();
        if (t == 0 && tid < a.J)
            for (int ln = 0; ln < ns; ++ln) dbacc += sd[ln * JT + tid];
        if (live) {
            for (int ln = 0; ln < ns; ++ln) {
                const long node = s0 + ln, b = node / a.N, n = node - b * a.N;
                const long e = ((b * a.T + t) * a.N + n) * a.D + d;
                const float xv = a.x[e];
                float dxv = 0.f;
#pragma unroll
                for (int j = 0; j < JT; ++j) {
                    const float g = sd[ln * JT + j];
                    acc[j] = fmaf(g, xv, acc[j]);
                    dxv = fmaf(g, w[j], dxv);
                }
                if (a.dx) a.dx[e] = dxv;
            }
        }
    }
    float* part = a.partial + (long)blockIdx.x * a.PW;
    if (live) {
#pragma unroll
        for (int j = 0; j < JT; ++j)
            if (j < a.J) part[j * K + (long)t * a.D + d] = acc[j];
    }
    if (t == 0 && tid < a.J) part[a.J * K + tid] = dbacc;
}

inline int out_proj_chunk(int J) { return OP_SUB * ((J + 15) / 16); }

inline int embed_chunk_rows(long P, int D) {
    const long r = (4 * P + 64L * D - 1) / (64L * D);
    return (int)(64 * (r < 1 ? 1 : r));
}

}  // namespace

int launch_stae_drop_add_layernorm(const float* residual, const float* y, const uint32_t* keep, float s, const float* gamma, const float* beta,
                                   float eps, long M, int D, float* out, hipStream_t st) {
    const long blocks = (M + THREADS / 64 - 1) / (THREADS / 64);
    REGT_CHECK_ARG(blocks < (1L << 31), "stae drop_add_layernorm: %ld workgroups exceed the grid", blocks);
    hipLaunchKernelGGL(stae_add_layernorm_kernel<true>, dim3((unsigned)blocks), dim3(THREADS), 0, st, residual, y, keep, s, gamma, beta, eps, M,
                       D, out);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

long stae_embed_bwd_partial_floats(const StaeDims& s) {
    return (long)s.e_in * s.input_dim + s.e_in + (long)s.steps_per_day * s.e_tod + (long)s.days_per_week * s.e_dow;
}

size_t stae_embed_bwd_scratch_floats(const StaeDims& s) {
    const long P = stae_embed_bwd_partial_floats(s), M = (long)s.batch * s.in_steps * s.num_nodes;
    const int R = embed_chunk_rows(P, stae_model_dim(s));
    return (size_t)((M + R - 1) / R) * P;
}

int launch_stae_embed_bwd(const StaeDims& s, const float* x, const float* dx0, float* const* G, float* scratch, hipStream_t st) {
    const int D = stae_model_dim(s);
    EmbedBwdArgs a{};
    a.x = x, a.dx0 = dx0, a.partial = scratch;
    a.M = (long)s.batch * s.in_steps * s.num_nodes;
    a.F = s.in_features, a.Cin = s.input_dim, a.e_in = s.e_in, a.e_tod = s.e_tod, a.e_dow = s.e_dow, a.D = D;
    a.spd = s.steps_per_day, a.dpw = s.days_per_week;
    const long P = stae_embed_bwd_partial_floats(s);
    REGT_CHECK_ARG(P <= STAE_EMBED_BWD_MAX_LDS,
                   "stae embed backward: input_embedding_dim * (input_dim + 1) + steps_per_day * tod_embedding_dim + days_per_week * "
                   "dow_embedding_dim = %ld floats exceed the %d an LDS image holds",
                   P, STAE_EMBED_BWD_MAX_LDS);
    a.P = (int)P, a.R = embed_chunk_rows(P, D);
    const long nchunks = (a.M + a.R - 1) / a.R;
    const int threads = 64 * ((s.e_in + s.e_tod + s.e_dow + 63) / 64);                // <= THREADS: the three widths sum to at most D <= 256
    hipLaunchKernelGGL(stae_embed_bwd_chunk_kernel, dim3((unsigned)nchunks), dim3(threads), (size_t)P * sizeof(float), st, a);
    REGT_CHECK_LAUNCH();
    SlabSegs segs{};
    add_seg(segs, G[2], (long)s.e_in * s.input_dim);
    add_seg(segs, G[3], s.e_in);
    add_seg(segs, G[4], (long)s.steps_per_day * s.e_tod);      // empty (and G[4] NULL) where the width is 0
    add_seg(segs, G[5], (long)s.days_per_week * s.e_dow);
    if (int rc = launch_stae_col_reduce(scratch, nchunks, P, segs, st)) return rc;
    const long owners = (long)s.num_nodes * s.e_sp + (long)s.in_steps * s.num_nodes * s.e_adp;
    if (owners > 0) {
        hipLaunchKernelGGL(stae_embed_bwd_owner_kernel, dim3((unsigned)((owners + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, dx0, s.batch,
                           s.in_steps, s.num_nodes, D, s.e_sp, s.e_adp, s.e_in + s.e_tod + s.e_dow, G[0], G[1]);
        REGT_CHECK_LAUNCH();
    }
    return REGT_OK;
}

size_t stae_output_proj_bwd_scratch_floats(const StaeDims& s) {
    const long J = (long)s.out_steps * s.output_dim, K = (long)s.in_steps * stae_model_dim(s), nodes = (long)s.batch * s.num_nodes;
    const int NCH = out_proj_chunk((int)J);
    return (size_t)((nodes + NCH - 1) / NCH) * (J * K + J);
}

int launch_stae_output_proj_bwd(const StaeDims& s, const float* x, const float* w, const float* dout, long sb, long so, long sn, long sc,
                                float* dx, float* dw, float* db, float* scratch, hipStream_t st) {
    OutProjBwdArgs a{};
    a.x = x, a.w = w, a.dout = dout, a.dx = dx, a.partial = scratch;
    a.sb = sb, a.so = so, a.sn = sn, a.sc = sc;
    a.T = s.in_steps, a.N = s.num_nodes, a.D = stae_model_dim(s), a.J = s.out_steps * s.output_dim, a.OD = s.output_dim;
    a.nodes = (long)s.batch * s.num_nodes, a.NCH = out_proj_chunk(a.J);
    const long K = (long)a.T * a.D;
    a.PW = a.J * K + a.J;
    const long nchunks = (a.nodes + a.NCH - 1) / a.NCH;
    const dim3 grid((unsigned)nchunks, (unsigned)a.T), block(64 * ((a.D + 63) / 64));
    if (a.J <= 4)
        hipLaunchKernelGGL(stae_output_proj_bwd_kernel<4>, grid, block, 0, st, a);
    else if (a.J <= 16)
        hipLaunchKernelGGL(stae_output_proj_bwd_kernel<16>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(stae_output_proj_bwd_kernel<64>, grid, block, 0, st, a);
    REGT_CHECK_LAUNCH();
    SlabSegs segs{};
    add_seg(segs, dw, a.J * K);
    add_seg(segs, db, a.J);
    return launch_stae_col_reduce(scratch, nchunks, a.PW, segs, st);
}

}  // namespace regt
