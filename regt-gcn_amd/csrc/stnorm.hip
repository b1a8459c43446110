// The reference's STNorm (models/STNorm.py): a WaveNet stack of gated dilated convolutions whose input is [x, TNorm(x), SNorm(x)].
//
//   x_0     = start_conv(left-pad(input))                                  (1x1 conv C_in -> 16; padded columns hold the bias)
//   layer i (dilation d = 2^(i % layers)):
//     z     = [x_i | TNorm_i(x_i) | SNorm_i(x_i)]                            (16 * NZ channels, NZ = 1 + tnorm + snorm)
//     h     = tanh(Wf0 z[t] + Wf1 z[t+d] + bf) * sigmoid(Wg0 z[t] + Wg1 z[t+d] + bg)
//     skip  = Wsk h + bsk + skip                                             (last L_out columns only)
//     x_i+1 = Wr h + br + x_i[t + d]
//   out     = end_conv_2(relu(end_conv_1(relu(skip))))
//
// TNorm: per (channel, node) statistics over a group of consecutive batch elements and all columns (biased variance; running
// buffers in eval mode, updated group by group in training mode).  SNorm: per (batch, channel, column) statistics over ALL nodes
// (unbiased variance), so every layer seam is a launch boundary: each layer launch writes per-wave (count, mean, M2) partials of
// its output, st_sn_final combines them with Chan's formula in a fixed order, and the next launch reads the finished mean / rstd.
//
// Mapping: one thread owns one node for every batch element and column; a workgroup is one wave of 64 consecutive nodes.
// Activations are stored (B, L, 16, N) -- [b][t][c][n] -- so the lanes of a wave read and write consecutive addresses.
// The backward runs the layers in reverse.  It recomputes z, the convolutions and the gate from the saved layer inputs, keeps the
// node-local TNorm backward in the same launch and defers SNorm's (which needs sums over all nodes of dsn and dsn * x^) to the next
// launch through a second seam.  Weight gradients: each wave stages its 64 rows in LDS and accumulates the outer products into its
// own slab row (each lane owns fixed entries, rows summed in order); the slab rows are then reduced in a fixed order.  No float
// atomics anywhere: the gradients are bit-reproducible.
#include "lane_helpers.h"
#include "slab_reduce.h"

namespace regt {

namespace {

constexpr int SC = 16;                 // channels (models/STNorm.py default)
constexpr int WV = 64;                 // nodes per workgroup (one wave)
constexpr float ST_EPS = 1e-5f;
constexpr float ST_MOM = 0.1f;
constexpr int RED_CHUNK = 32;

// (na, ma, Ma) <- (na, ma, Ma) + (nb, mb, Mb): Chan et al.'s pairwise update of count, mean and sum of squared deviations
__device__ __forceinline__ void chan(float& na, float& ma, float& Ma, float nb, float mb, float Mb) {
    if (nb == 0.f) return;
    if (na == 0.f) { na = nb; ma = mb; Ma = Mb; return; }
    const float n = na + nb, delta = mb - ma, fb = nb / n;
    ma = ma + delta * fb;
    Ma = Ma + Mb + delta * delta * na * fb;
    na = n;
}

__device__ __forceinline__ void chan_wave(float& n, float& m, float& M) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float n2 = __shfl_xor(n, off), m2 = __shfl_xor(m, off), M2 = __shfl_xor(M, off);
        chan(n, m, M, n2, m2, M2);
    }
}

struct Dims {
    int N, B, gs, G, L, Cin, O, nl, layers, tn, sn, train, L0, Lout, nw;
};

struct LayerP {                        // one layer's parameters / buffers (tn, sn pointers NULL when off)
    const float *fw, *fb, *gw, *gb, *rw, *rb, *kw, *kb, *tg, *tb, *sg, *sb;
    float *rm, *rv;
};

// outer-product blocks of a weight-gradient slab row: entry (i, j) of block k = sum over rows of row[a + i] * row[b + j]
struct OpBlocks {
    int a[8], na[8], b[8], nb[8];
    int nblk, E;
};

// Each lane owns entries lane, lane + 64, ... of the wave's slab row and adds rows [0, nvalid) of the staged LDS rows in a fixed
// order: four interleaved partial sums over the rows, combined pairwise, then added to the entry.  One running sum through every
// row of every column instead is a chain of B * L * 64 additions, and where a normalisation's 1 / sqrt(var + eps) makes the
// terms large and cancelling (start_conv.bias under left padding) its rounding grows with that length.
__device__ void op_accumulate(const float* rows, int stride, int nvalid, const OpBlocks& ob, float* slab_row) {
    const int lane = threadIdx.x;
    for (int e = lane; e < ob.E; e += WV) {
        int k = 0, base = 0;
        while (e >= base + ob.na[k] * ob.nb[k]) { base += ob.na[k] * ob.nb[k]; ++k; }
        const int loc = e - base, i = loc / ob.nb[k], j = loc - (loc / ob.nb[k]) * ob.nb[k];
        const float* pa = rows + ob.a[k] + i;
        const float* pb = rows + ob.b[k] + j;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int r = 0;
        for (; r + 4 <= nvalid; r += 4) {
            s0 = fmaf(pa[r * stride], pb[r * stride], s0);
            s1 = fmaf(pa[(r + 1) * stride], pb[(r + 1) * stride], s1);
            s2 = fmaf(pa[(r + 2) * stride], pb[(r + 2) * stride], s2);
            s3 = fmaf(pa[(r + 3) * stride], pb[(r + 3) * stride], s3);
        }
        for (; r < nvalid; ++r) s0 = fmaf(pa[r * stride], pb[r * stride], s0);
        slab_row[e] += (s0 + s1) + (s2 + s3);
    }
}

__device__ void slab_zero(float* slab_row, int E) {
    for (int e = threadIdx.x; e < E; e += WV) slab_row[e] = 0.f;
}

// TNorm statistics of node n over group g (batch elements g*gs .. g*gs+gs-1, columns 0..Li-1): two passes, biased variance
__device__ void tnorm_batch_stats(const float* __restrict__ x, const Dims& d, int Li, int g, long n, float (&mean)[SC], float (&var)[SC]) {
    const long plane = (long)SC * d.N;
    const float cnt = (float)(d.gs * Li);
#pragma unroll
    for (int c = 0; c < SC; ++c) mean[c] = 0.f, var[c] = 0.f;
    for (int b = g * d.gs; b < (g + 1) * d.gs; ++b)
        for (int t = 0; t < Li; ++t) {
            const float* col = x + ((long)b * Li + t) * plane + n;
#pragma unroll
            for (int c = 0; c < SC; ++c) mean[c] += col[(long)c * d.N];
        }
#pragma unroll
    for (int c = 0; c < SC; ++c) mean[c] /= cnt;
    for (int b = g * d.gs; b < (g + 1) * d.gs; ++b)
        for (int t = 0; t < Li; ++t) {
            const float* col = x + ((long)b * Li + t) * plane + n;
#pragma unroll
            for (int c = 0; c < SC; ++c) {
                const float v = col[(long)c * d.N] - mean[c];
                var[c] = fmaf(v, v, var[c]);
            }
        }
#pragma unroll
    for (int c = 0; c < SC; ++c) var[c] /= cnt;
}

// the normalisation in use for node n, group g: batch statistics (training; running buffers updated when `update`) or running ones
__device__ void tnorm_stats(const float* __restrict__ x, const Dims& d, const LayerP& p, int Li, int g, long n, bool live, bool update,
                            float (&mean)[SC], float (&rstd)[SC]) {
    if (d.train) {
        float var[SC];
        tnorm_batch_stats(x, d, Li, g, n, mean, var);
        const float cnt = (float)(d.gs * Li);
#pragma unroll
        for (int c = 0; c < SC; ++c) {
            rstd[c] = 1.f / sqrtf(var[c] + ST_EPS);
            if (update && live) {
                const long k = (long)c * d.N + n;
                p.rm[k] = ST_MOM * mean[c] + (1.f - ST_MOM) * p.rm[k];
                p.rv[k] = ST_MOM * var[c] * cnt / (cnt - 1.f) + (1.f - ST_MOM) * p.rv[k];
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < SC; ++c) {
            const long k = (long)c * d.N + n;
            mean[c] = p.rm[k];
            rstd[c] = 1.f / sqrtf(p.rv[k] + ST_EPS);
        }
    }
}

// z at column t: [x | tnorm | snorm]
template <bool TN, bool SN, int NZ = 1 + TN + SN>
__device__ __forceinline__ void build_z(const float* __restrict__ x, const Dims& d, const LayerP& p, int Li, int b, int t, long n,
                                        const float (&tm)[SC], const float (&tr)[SC], const float (&tg)[SC], const float (&tb)[SC],
                                        const float* __restrict__ sstat, float (&z)[NZ * SC]) {
    const float* col = x + ((long)b * Li + t) * SC * d.N + n;
#pragma unroll
    for (int c = 0; c < SC; ++c) {
        const float v = col[(long)c * d.N];
        z[c] = v;
        if constexpr (TN) z[SC + c] = (v - tm[c]) * tr[c] * tg[c] + tb[c];
        if constexpr (SN) {
            const float* ss = sstat + (((long)b * Li + t) * SC + c) * 2;
            z[(TN ? 2 : 1) * SC + c] = (v - ss[0]) * ss[1] * p.sg[c] + p.sb[c];
        }
    }
}

// filter / gate convolutions and the gate at one column: h = tanh(f) * sigmoid(g)
template <int NZ>
__device__ __forceinline__ void gate(const LayerP& p, const float (&z0)[NZ * SC], const float (&z1)[NZ * SC], float (&f)[SC],
                                     float (&g)[SC]) {
    constexpr int K = NZ * SC;
    for (int o = 0; o < SC; ++o) {
        float a = p.fb[o], bb = p.gb[o];
        const float* wf = p.fw + o * 2 * K;
        const float* wg = p.gw + o * 2 * K;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            a = fmaf(wf[2 * k], z0[k], a);
            a = fmaf(wf[2 * k + 1], z1[k], a);
            bb = fmaf(wg[2 * k], z0[k], bb);
            bb = fmaf(wg[2 * k + 1], z1[k], bb);
        }
        f[o] = a;
        g[o] = bb;
    }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------

struct StartArgs {
    Dims d;
    const float *x, *w, *b;            // input (B, L, N, Cin); start_conv weight (16, Cin), bias (16)
    float *x0, *pm, *pM;               // x_0 (B, L0, 16, N); SNorm partials of x_0 (row (b*L0 + t)*16 + c, column wave)
};

__global__ __launch_bounds__(WV) void st_start_fwd(StartArgs a) {
    const Dims& d = a.d;
    const long n = (long)blockIdx.x * WV + threadIdx.x;
    const bool live = n < d.N;
    const long nn = live ? n : 0;
    const int pad = d.L0 - d.L;
    for (int b = 0; b < d.B; ++b)
        for (int t = 0; t < d.L0; ++t) {
            float acc[SC];
#pragma unroll
            for (int c = 0; c < SC; ++c) acc[c] = a.b[c];
            const int ti = t - pad;
            if (ti >= 0) {
                const float* xr = a.x + (((long)b * d.L + ti) * d.N + nn) * d.Cin;
                for (int ci = 0; ci < d.Cin; ++ci) {
                    const float v = xr[ci];
#pragma unroll
                    for (int c = 0; c < SC; ++c) acc[c] = fmaf(a.w[c * d.Cin + ci], v, acc[c]);
                }
            }
            float* col = a.x0 + ((long)b * d.L0 + t) * SC * d.N;
#pragma unroll
            for (int c = 0; c < SC; ++c) {
                if (live) col[(long)c * d.N + n] = acc[c];
                if (d.sn) {
                    float cn = live ? 1.f : 0.f, m = live ? acc[c] : 0.f, M = 0.f;
                    chan_wave(cn, m, M);
                    if (threadIdx.x == 0) {
                        const long row = ((long)b * d.L0 + t) * SC + c;
                        a.pm[row * d.nw + blockIdx.x] = m;
                        a.pM[row * d.nw + blockIdx.x] = M;
                    }
                }
            }
        }
}

// mean / rstd per (b, t, c) of one layer input from the per-wave partials (one wave per row, waves combined in a fixed order)
__global__ __launch_bounds__(WV) void st_sn_final(const float* __restrict__ pm, const float* __restrict__ pM, int N, int nw,
                                                  float* __restrict__ sstat) {
    const long row = blockIdx.x;
    float cn = 0.f, m = 0.f, M = 0.f;
    for (int w = threadIdx.x; w < nw; w += WV) chan(cn, m, M, (float)min(WV, N - w * WV), pm[row * nw + w], pM[row * nw + w]);
    chan_wave(cn, m, M);
    if (threadIdx.x == 0) {
        sstat[row * 2] = m;
        sstat[row * 2 + 1] = 1.f / sqrtf(M / (float)(N - 1) + ST_EPS);
    }
}

struct LayerFwdArgs {
    Dims d;
    LayerP p;
    int Li, Ln, dil, first, update;
    const float* x;                    // (B, Li, 16, N)
    const float* sstat;                // (B, Li, 16, 2)
    float* xn;                         // (B, Ln, 16, N) (not for the last layer)
    float *pm, *pM;                    // SNorm partials of xn
    float* skip;                       // (B, Lout, 16, N)
    const float *e1w, *e1b, *e2w, *e2b;  // head (last layer)
    float* out;                        // (B, O, N, Lout)
};

template <bool TN, bool SN, bool LAST>
__global__ __launch_bounds__(WV) void st_layer_fwd(LayerFwdArgs a) {
    constexpr int NZ = 1 + TN + SN, K = NZ * SC;
    const Dims& d = a.d;
    const LayerP& p = a.p;
    const long n = (long)blockIdx.x * WV + threadIdx.x;
    const bool live = n < d.N;
    const long nn = live ? n : 0;
    const long plane = (long)SC * d.N;
    float tg[SC], tb[SC], tm[SC], tr[SC];
#pragma unroll
    for (int c = 0; c < SC; ++c) {
        tg[c] = d.tn ? p.tg[(long)c * d.N + nn] : 0.f;
        tb[c] = d.tn ? p.tb[(long)c * d.N + nn] : 0.f;
        tm[c] = 0.f, tr[c] = 0.f;
    }
    for (int g = 0; g < d.G; ++g) {
        if (TN) tnorm_stats(a.x, d, p, a.Li, g, nn, live, a.update, tm, tr);
        for (int b = g * d.gs; b < (g + 1) * d.gs; ++b)
            for (int t = 0; t < a.Ln; ++t) {
                float z0[K], z1[K], f[SC], gg[SC], h[SC];
                build_z<TN, SN>(a.x, d, p, a.Li, b, t, nn, tm, tr, tg, tb, a.sstat, z0);
                build_z<TN, SN>(a.x, d, p, a.Li, b, t + a.dil, nn, tm, tr, tg, tb, a.sstat, z1);
                gate<NZ>(p, z0, z1, f, gg);
#pragma unroll
                for (int o = 0; o < SC; ++o) h[o] = tanhf(f[o]) * sigm(gg[o]);
                const int ts = t - (a.Ln - d.Lout);
                float sk[SC];
                if (ts >= 0) {
                    float* scol = a.skip + ((long)b * d.Lout + ts) * plane + nn;
                    for (int o = 0; o < SC; ++o) {
                        float s = p.kb[o];
#pragma unroll
                        for (int c = 0; c < SC; ++c) s = fmaf(p.kw[o * SC + c], h[c], s);
                        if (!a.first) s = s + scol[(long)o * d.N];
                        sk[o] = s;
                        if (live) scol[(long)o * d.N] = s;
                    }
                }
                if (LAST) {
                    if (ts >= 0) {                                      // (always: the last layer's columns are the last L_out)
                        float r[SC];
                        for (int o = 0; o < SC; ++o) {
                            float s = a.e1b[o];
#pragma unroll
                            for (int c = 0; c < SC; ++c) s = fmaf(a.e1w[o * SC + c], fmaxf(sk[c], 0.f), s);
                            r[o] = fmaxf(s, 0.f);
                        }
                        for (int o = 0; o < d.O; ++o) {
                            float s = a.e2b[o];
#pragma unroll
                            for (int c = 0; c < SC; ++c) s = fmaf(a.e2w[o * SC + c], r[c], s);
                            if (live) a.out[(((long)b * d.O + o) * d.N + n) * d.Lout + ts] = s;
                        }
                    }
                } else {
                    const float* res = a.x + ((long)b * a.Li + t + a.dil) * plane + nn;
                    float* xcol = a.xn + ((long)b * a.Ln + t) * plane;
                    for (int o = 0; o < SC; ++o) {
                        float s = p.rb[o];
#pragma unroll
                        for (int c = 0; c < SC; ++c) s = fmaf(p.rw[o * SC + c], h[c], s);
                        s = s + res[(long)o * d.N];
                        if (live) xcol[(long)o * d.N + n] = s;
                        if (d.sn) {
                            float cn = live ? 1.f : 0.f, m = live ? s : 0.f, M = 0.f;
                            chan_wave(cn, m, M);
                            if (threadIdx.x == 0) {
                                const long row = ((long)b * a.Ln + t) * SC + o;
                                a.pm[row * d.nw + blockIdx.x] = m;
                                a.pM[row * d.nw + blockIdx.x] = M;
                            }
                        }
                    }
                }
            }
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------

struct HeadBwdArgs {
    Dims d;
    const float *skip, *dout, *e1w, *e1b, *e2w;
    float* dskip;                      // (B, Lout, 16, N)
    float* slab;                       // per wave: [dE2 (O,16) | de2b (O) | dE1 (16,16) | de1b (16)]
    OpBlocks ob;
    int stride;
};

__global__ __launch_bounds__(WV) void st_head_bwd(HeadBwdArgs a) {
    extern __shared__ float rows[];    // [dout (O) | rr (16) | dr1 (16) | a1 (16) | 1]
    const Dims& d = a.d;
    const long n = (long)blockIdx.x * WV + threadIdx.x;
    const bool live = n < d.N;
    const long nn = live ? n : 0;
    const int nvalid = (int)min((long)WV, d.N - (long)blockIdx.x * WV);
    float* slab_row = a.slab + (long)blockIdx.x * a.ob.E;
    slab_zero(slab_row, a.ob.E);
    float* row = rows + threadIdx.x * a.stride;
    const long plane = (long)SC * d.N;
    for (int b = 0; b < d.B; ++b)
        for (int ts = 0; ts < d.Lout; ++ts) {
            float sk[SC], a1[SC], r1[SC], dr1[SC];
            const float* scol = a.skip + ((long)b * d.Lout + ts) * plane + nn;
#pragma unroll
            for (int c = 0; c < SC; ++c) sk[c] = scol[(long)c * d.N], a1[c] = fmaxf(sk[c], 0.f);
            for (int o = 0; o < SC; ++o) {
                float s = a.e1b[o];
#pragma unroll
                for (int c = 0; c < SC; ++c) s = fmaf(a.e1w[o * SC + c], a1[c], s);
                r1[o] = s;
                dr1[o] = 0.f;
            }
            for (int o = 0; o < d.O; ++o) {
                const float g = live ? a.dout[(((long)b * d.O + o) * d.N + n) * d.Lout + ts] : 0.f;
                row[o] = g;
#pragma unroll
                for (int c = 0; c < SC; ++c) dr1[c] = fmaf(a.e2w[o * SC + c], g, dr1[c]);
            }
#pragma unroll
            for (int c = 0; c < SC; ++c) {
                dr1[c] = r1[c] > 0.f ? dr1[c] : 0.f;
                row[d.O + c] = fmaxf(r1[c], 0.f);
                row[d.O + SC + c] = dr1[c];
                row[d.O + 2 * SC + c] = a1[c];
            }
            row[d.O + 3 * SC] = 1.f;
            float* dcol = a.dskip + ((long)b * d.Lout + ts) * plane;
            for (int c = 0; c < SC; ++c) {
                float s = 0.f;
#pragma unroll
                for (int o = 0; o < SC; ++o) s = fmaf(a.e1w[o * SC + c], dr1[o], s);
                if (live) dcol[(long)c * d.N + n] = sk[c] > 0.f ? s : 0.f;
            }
            __syncthreads();
            op_accumulate(rows, a.stride, nvalid, a.ob, slab_row);
            __syncthreads();
        }
}

struct LayerBwdArgs {
    Dims d;
    LayerP p;
    int Li, Ln, dil;
    const float *x, *sstat;            // layer input (B, Li, 16, N) and its SNorm mean / rstd
    // gradient w.r.t. the layer output x_{i+1} = dxr_next + SNorm_{i+1} backward (has_next; else 0)
    int has_next;
    const float *xnext, *sstat_next, *ssum_next, *dxr_next, *dsn_next, *sg_next;
    const float* dskip;                // (B, Lout, 16, N)
    float *dxr, *dsn, *dtn, *dfg;      // outputs / scratch of this layer
    float *pp1, *pp2;                  // per-wave sums of dsn and dsn * x^ (rows (b*Li + t)*16 + c)
    float *dtg, *dtb;                  // TNorm gamma / beta gradients (16, N), written directly
    float* slab;
    OpBlocks ob;
    int stride;
};

// dL/dx_{i+1} at (b, t, c, node n)
__device__ __forceinline__ float load_dx(const LayerBwdArgs& a, int b, int t, int c, long n) {
    if (!a.has_next) return 0.f;
    const Dims& d = a.d;
    const long k = (((long)b * a.Ln + t) * SC + c) * d.N + n;
    float v = a.dxr_next[k];
    if (d.sn) {
        const long r = ((long)b * a.Ln + t) * SC + c;
        const float m = a.sstat_next[2 * r], rs = a.sstat_next[2 * r + 1];
        const float s1 = a.ssum_next[2 * r], s2 = a.ssum_next[2 * r + 1];
        const float gm = a.sg_next[c];
        const float xh = (a.xnext[k] - m) * rs;
        v += rs * (gm * a.dsn_next[k] - gm * s1 / (float)d.N - xh * gm * s2 / (float)(d.N - 1));
    }
    return v;
}

template <bool TN, bool SN>
__global__ __launch_bounds__(WV) void st_layer_bwd(LayerBwdArgs a) {
    constexpr int NZ = 1 + TN + SN, K = NZ * SC;
    extern __shared__ float rows[];    // [zz (2K, interleaved k*2 + tap) | df | dg | h | dxo | dsk | 1]
    const Dims& d = a.d;
    const LayerP& p = a.p;
    const long n = (long)blockIdx.x * WV + threadIdx.x;
    const bool live = n < d.N;
    const long nn = live ? n : 0;
    const int nvalid = (int)min((long)WV, d.N - (long)blockIdx.x * WV);
    const long plane = (long)SC * d.N;
    float* slab_row = a.slab + (long)blockIdx.x * a.ob.E;
    slab_zero(slab_row, a.ob.E);
    float* row = rows + threadIdx.x * a.stride;
    float tg[SC], tb[SC], tm[SC], tr[SC], dtg[SC], dtb[SC];
#pragma unroll
    for (int c = 0; c < SC; ++c) {
        tg[c] = d.tn ? p.tg[(long)c * d.N + nn] : 0.f;
        tb[c] = d.tn ? p.tb[(long)c * d.N + nn] : 0.f;
        tm[c] = 0.f, tr[c] = 0.f, dtg[c] = 0.f, dtb[c] = 0.f;
    }
    constexpr int tsn = TN ? 2 * SC : SC;     // offset of the SNorm slice in z
    for (int g = 0; g < d.G; ++g) {
        if (TN) tnorm_stats(a.x, d, p, a.Li, g, nn, live, false, tm, tr);
        // 1: recompute the gate per output column, df / dg, weight gradients
        for (int b = g * d.gs; b < (g + 1) * d.gs; ++b)
            for (int t = 0; t < a.Ln; ++t) {
                float z0[K], z1[K], f[SC], gg[SC], h[SC], dh[SC], dxo[SC], dsk[SC];
                build_z<TN, SN>(a.x, d, p, a.Li, b, t, nn, tm, tr, tg, tb, a.sstat, z0);
                build_z<TN, SN>(a.x, d, p, a.Li, b, t + a.dil, nn, tm, tr, tg, tb, a.sstat, z1);
                gate<NZ>(p, z0, z1, f, gg);
                const int ts = t - (a.Ln - d.Lout);
#pragma unroll
                for (int c = 0; c < SC; ++c) {
                    h[c] = tanhf(f[c]) * sigm(gg[c]);
                    dxo[c] = live ? load_dx(a, b, t, c, n) : 0.f;
                    dsk[c] = (ts >= 0 && live) ? a.dskip[((long)b * d.Lout + ts) * plane + (long)c * d.N + n] : 0.f;
                    dh[c] = 0.f;
                }
                for (int o = 0; o < SC; ++o)
#pragma unroll
                    for (int c = 0; c < SC; ++c) dh[c] = fmaf(p.rw[o * SC + c], dxo[o], fmaf(p.kw[o * SC + c], dsk[o], dh[c]));
                float* fgcol = a.dfg + ((long)b * a.Ln + t) * 2 * plane;
#pragma unroll
                for (int c = 0; c < SC; ++c) {
                    const float th = tanhf(f[c]), sg = sigm(gg[c]);
                    const float df = dh[c] * sg * (1.f - th * th);
                    const float dg = dh[c] * th * sg * (1.f - sg);
                    if (live) fgcol[(long)c * d.N + n] = df, fgcol[(long)(SC + c) * d.N + n] = dg;
                    row[2 * K + c] = df;
                    row[2 * K + SC + c] = dg;
                    row[2 * K + 2 * SC + c] = h[c];
                    row[2 * K + 3 * SC + c] = dxo[c];
                    row[2 * K + 4 * SC + c] = dsk[c];
                }
#pragma unroll
                for (int k = 0; k < K; ++k) row[2 * k] = z0[k], row[2 * k + 1] = z1[k];
                row[2 * K + 5 * SC] = 1.f;
                __syncthreads();
                op_accumulate(rows, a.stride, nvalid, a.ob, slab_row);
                __syncthreads();
            }
        // 2: dz per input column -> dx (direct + residual), dtn, dsn
        float A1[SC], A2[SC];
#pragma unroll
        for (int c = 0; c < SC; ++c) A1[c] = 0.f, A2[c] = 0.f;
        for (int b = g * d.gs; b < (g + 1) * d.gs; ++b)
            for (int t = 0; t < a.Li; ++t) {
                float dz[K];
#pragma unroll
                for (int k = 0; k < K; ++k) dz[k] = 0.f;
                for (int tap = 0; tap < 2; ++tap) {
                    const int to = t - tap * a.dil;          // the output column that read column t through this tap
                    if (to < 0 || to >= a.Ln) continue;
                    const float* fgcol = a.dfg + ((long)b * a.Ln + to) * 2 * plane + nn;
                    for (int o = 0; o < SC; ++o) {
                        const float df = fgcol[(long)o * d.N], dg = fgcol[(long)(SC + o) * d.N];
                        const float* wf = p.fw + o * 2 * K + tap;
                        const float* wg = p.gw + o * 2 * K + tap;
#pragma unroll
                        for (int k = 0; k < K; ++k) dz[k] = fmaf(wf[2 * k], df, fmaf(wg[2 * k], dg, dz[k]));
                    }
                }
                const long cb = ((long)b * a.Li + t) * plane;
                const float* xcol = a.x + cb + nn;
#pragma unroll
                for (int c = 0; c < SC; ++c) {
                    float v = dz[c];
                    if (t >= a.dil && live) v += load_dx(a, b, t - a.dil, c, n);
                    const float xv = xcol[(long)c * d.N];
                    if constexpr (TN) {
                        const float dt = dz[SC + c];
                        const float xh = (xv - tm[c]) * tr[c];
                        dtg[c] = fmaf(dt, xh, dtg[c]);
                        dtb[c] += dt;
                        if (d.train) {
                            A1[c] += dt * tg[c];
                            A2[c] = fmaf(dt * tg[c], xh, A2[c]);
                            if (live) a.dtn[cb + (long)c * d.N + n] = dt;
                        } else {
                            v = fmaf(dt * tg[c], tr[c], v);
                        }
                    }
                    if (live) a.dxr[cb + (long)c * d.N + n] = v;
                    if constexpr (SN) {
                        const float ds = live ? dz[tsn + c] : 0.f;
                        if (live) a.dsn[cb + (long)c * d.N + n] = ds;
                        const float* ss = a.sstat + (((long)b * a.Li + t) * SC + c) * 2;
                        const float xh = (xv - ss[0]) * ss[1];
                        const float s1 = wave_sum(ds), s2 = wave_sum(ds * xh);
                        if (threadIdx.x == 0) {
                            const long r = ((long)b * a.Li + t) * SC + c;
                            a.pp1[r * d.nw + blockIdx.x] = s1;
                            a.pp2[r * d.nw + blockIdx.x] = s2;
                        }
                    }
                }
            }
        // 3: TNorm backward through the batch statistics (training)
        if (d.tn && d.train && live) {
            const float cnt = (float)(d.gs * a.Li);
            for (int b = g * d.gs; b < (g + 1) * d.gs; ++b)
                for (int t = 0; t < a.Li; ++t) {
                    const long cb = ((long)b * a.Li + t) * plane + n;
#pragma unroll
                    for (int c = 0; c < SC; ++c) {
                        const long k = cb + (long)c * d.N;
                        const float xh = (a.x[k] - tm[c]) * tr[c];
                        a.dxr[k] += tr[c] * (a.dtn[k] * tg[c] - A1[c] / cnt - xh * A2[c] / cnt);
                    }
                }
        }
    }
    if (d.tn && live) {
#pragma unroll
        for (int c = 0; c < SC; ++c) a.dtg[(long)c * d.N + n] = dtg[c], a.dtb[(long)c * d.N + n] = dtb[c];
    }
}

// sums over all nodes of dsn and dsn * x^ per (b, t, c), waves in a fixed order
__global__ __launch_bounds__(WV) void st_sn_bwd_final(const float* __restrict__ pp1, const float* __restrict__ pp2, int nw,
                                                      float* __restrict__ ssum) {
    const long row = blockIdx.x;
    float s1 = 0.f, s2 = 0.f;
    for (int w = threadIdx.x; w < nw; w += WV) s1 += pp1[row * nw + w], s2 += pp2[row * nw + w];
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (threadIdx.x == 0) ssum[2 * row] = s1, ssum[2 * row + 1] = s2;
}

// SNorm gamma / beta gradients: dgamma[c] = sum_{b,t} S2, dbeta[c] = sum_{b,t} S1
__global__ __launch_bounds__(WV) void st_sn_param_grad(const float* __restrict__ ssum, int rows_bt, float* __restrict__ dg,
                                                       float* __restrict__ db) {
    const int c = threadIdx.x;
    if (c >= SC) return;
    float s1 = 0.f, s2 = 0.f;
    for (int r = 0; r < rows_bt; ++r) s1 += ssum[2 * ((long)r * SC + c)], s2 += ssum[2 * ((long)r * SC + c) + 1];
    dg[c] = s2;
    db[c] = s1;
}

struct StartBwdArgs {
    Dims d;
    LayerBwdArgs dx;                   // load_dx over layer 0 (Ln = L0)
    const float* x;
    float* slab;
    OpBlocks ob;
    int stride;
};

__global__ __launch_bounds__(WV) void st_start_bwd(StartBwdArgs a) {
    extern __shared__ float rows[];    // [dx0 (16) | x (Cin) | 1]
    const Dims& d = a.d;
    const long n = (long)blockIdx.x * WV + threadIdx.x;
    const bool live = n < d.N;
    const long nn = live ? n : 0;
    const int nvalid = (int)min((long)WV, d.N - (long)blockIdx.x * WV);
    float* slab_row = a.slab + (long)blockIdx.x * a.ob.E;
    slab_zero(slab_row, a.ob.E);
    float* row = rows + threadIdx.x * a.stride;
    const int pad = d.L0 - d.L;
    for (int b = 0; b < d.B; ++b)
        for (int t = 0; t < d.L0; ++t) {
#pragma unroll
            for (int c = 0; c < SC; ++c) row[c] = live ? load_dx(a.dx, b, t, c, n) : 0.f;
            const int ti = t - pad;
            const float* xr = a.x + (((long)b * d.L + (ti >= 0 ? ti : 0)) * d.N + nn) * d.Cin;
            for (int ci = 0; ci < d.Cin; ++ci) row[SC + ci] = ti >= 0 ? xr[ci] : 0.f;
            row[SC + d.Cin] = 1.f;
            __syncthreads();
            op_accumulate(rows, a.stride, nvalid, a.ob, slab_row);
            __syncthreads();
        }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------

struct Plan {
    Dims d;
    int K, NZ;
    long Lsum;                         // sum of the layer input lengths
    int Li[64], dil[64];
    long xoff[64], soff[64];           // workspace offsets of the saved layer inputs and SNorm stats
    long skip_off, pm_off, pM_off, ws_floats;   // pm / pM: the forward's per-wave SNorm partials
    long col;                          // floats of one (B, L0, 16, N) activation
    int Emax, nchunks;
    long sc_dxr[2], sc_dsn[2], sc_dtn, sc_dfg, sc_dskip, sc_pp1, sc_pp2, sc_ssum[2], sc_slab, sc_part, scratch_floats;
};

int layer_E(int K) { return 2 * (SC * 2 * K) + 2 * SC * SC + 4 * SC; }

bool make_plan(const StnDims& s, Plan& pl) {
    Dims& d = pl.d;
    d.N = s.num_nodes, d.B = s.batch, d.gs = s.tnorm_group, d.L = s.seq_len, d.Cin = s.in_dim, d.O = s.out_dim;
    d.layers = s.layers, d.tn = s.tnorm ? 1 : 0, d.sn = s.snorm ? 1 : 0, d.train = s.training ? 1 : 0;
    if (d.N < 2 || d.B < 1 || d.gs < 1 || d.B % d.gs || d.L < 1 || d.Cin < 1 || d.Cin > ST_MAX_CH || d.O < 1 || d.O > ST_MAX_CH ||
        s.blocks < 1 || d.layers < 1 || d.layers > 8 || (long)s.blocks * d.layers > 64)
        return false;
    d.G = d.B / d.gs;
    d.nl = s.blocks * d.layers;
    const int rf = 1 + s.blocks * ((1 << d.layers) - 1);
    d.L0 = d.L > rf ? d.L : rf;
    d.Lout = d.L0 - (rf - 1);
    d.nw = cdiv(d.N, WV);
    pl.NZ = 1 + d.tn + d.sn;
    pl.K = pl.NZ * SC;
    const long cols1 = (long)d.B * SC * d.N;  // floats of one column of all batch elements
    long off = 0, soff = 0, L = d.L0;
    pl.Lsum = 0;
    for (int i = 0; i < d.nl; ++i) {
        pl.Li[i] = (int)L;
        pl.dil[i] = 1 << (i % d.layers);
        pl.xoff[i] = off;
        off += L * cols1;
        pl.Lsum += L;
        L -= pl.dil[i];
    }
    pl.skip_off = off;
    off += (long)d.Lout * cols1;
    for (int i = 0; i < d.nl; ++i) {
        pl.soff[i] = off + soff;
        soff += d.sn ? (long)d.B * pl.Li[i] * SC * 2 : 0;
    }
    off += soff;
    const long prow = (long)d.B * d.L0 * SC * d.nw;   // partial rows x waves
    pl.pm_off = off, off += d.sn ? prow : 0;
    pl.pM_off = off, off += d.sn ? prow : 0;
    pl.ws_floats = off;
    pl.col = (long)d.L0 * cols1;
    pl.Emax = layer_E(pl.K);
    pl.Emax = pl.Emax > SC * d.Cin + SC ? pl.Emax : SC * d.Cin + SC;
    pl.Emax = pl.Emax > d.O * SC + d.O + SC * SC + SC ? pl.Emax : d.O * SC + d.O + SC * SC + SC;
    pl.nchunks = cdiv(d.nw, RED_CHUNK);
    long o2 = 0;
    for (int k = 0; k < 2; ++k) pl.sc_dxr[k] = o2, o2 += pl.col;
    for (int k = 0; k < 2; ++k) pl.sc_dsn[k] = o2, o2 += pl.col;
    pl.sc_dtn = o2, o2 += pl.col;
    pl.sc_dfg = o2, o2 += 2 * pl.col;
    pl.sc_dskip = o2, o2 += (long)d.Lout * cols1;
    pl.sc_pp1 = o2, o2 += prow;
    pl.sc_pp2 = o2, o2 += prow;
    for (int k = 0; k < 2; ++k) pl.sc_ssum[k] = o2, o2 += (long)d.B * d.L0 * SC * 2;
    pl.sc_slab = o2, o2 += (long)d.nw * pl.Emax;
    pl.sc_part = o2, o2 += (long)pl.nchunks * pl.Emax;
    pl.scratch_floats = o2;
    return true;
}

LayerP layer_params(const Plan& pl, const float* const* P, float* const* run, int i) {
    const float* const* q = P + ST_HEAD_PARAMS + ST_LAYER_PARAMS * i;
    LayerP p;
    p.fw = q[0], p.fb = q[1], p.gw = q[2], p.gb = q[3], p.rw = q[4], p.rb = q[5], p.kw = q[6], p.kb = q[7];
    p.tg = q[8], p.tb = q[9], p.sg = q[10], p.sb = q[11];
    p.rm = pl.d.tn ? run[2 * i] : nullptr;
    p.rv = pl.d.tn ? run[2 * i + 1] : nullptr;
    return p;
}

// slab reduction in a fixed order: stage 1 sums RED_CHUNK wave rows, stage 2 the chunks, scattered to the gradient tensors
int reduce_slab(const Plan& pl, float* slab, float* part, int E, const SlabSegs& sg, hipStream_t st) {
    return launch_slab_reduce_chunked<RED_CHUNK>(slab, pl.d.nw, E, part, sg, st);
}

void add_block(OpBlocks& ob, int a, int na, int b, int nb) {
    ob.a[ob.nblk] = a, ob.na[ob.nblk] = na, ob.b[ob.nblk] = b, ob.nb[ob.nblk] = nb;
    ++ob.nblk;
    ob.E += na * nb;
}

// LDS rows of the head / start-conv backward grow with out_dim / in_dim: past 64 KB the kernel's limit is raised to what ST_MAX_CH needs
constexpr int HEAD_LDS_MAX = WV * (ST_MAX_CH + 3 * SC + 1) * (int)sizeof(float);
constexpr int START_LDS_MAX = WV * (SC + ST_MAX_CH + 1) * (int)sizeof(float);
static_assert(HEAD_LDS_MAX <= 160 * 1024 && START_LDS_MAX <= 160 * 1024, "LDS rows exceed the CU's 160 KB");
static_assert(WV * (2 * 3 * SC + 5 * SC + 1) * (int)sizeof(float) <= 64 * 1024, "st_layer_bwd rows exceed 64 KB");

template <bool TN, bool SN>
int layer_fwd_nz(const LayerFwdArgs& a, bool last, hipStream_t st) {
    if (last) hipLaunchKernelGGL((st_layer_fwd<TN, SN, true>), dim3(a.d.nw), dim3(WV), 0, st, a);
    else hipLaunchKernelGGL((st_layer_fwd<TN, SN, false>), dim3(a.d.nw), dim3(WV), 0, st, a);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

template <bool TN, bool SN>
int layer_bwd_nz(const LayerBwdArgs& a, hipStream_t st) {
    const int bytes = WV * a.stride * (int)sizeof(float);
    hipLaunchKernelGGL((st_layer_bwd<TN, SN>), dim3(a.d.nw), dim3(WV), bytes, st, a);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace

bool stnorm_sizes(const StnDims& s, size_t* ws_floats, size_t* scratch_floats) {
    Plan pl;
    if (!make_plan(s, pl)) return false;
    if (ws_floats) *ws_floats = (size_t)pl.ws_floats;
    if (scratch_floats) *scratch_floats = (size_t)pl.scratch_floats;
    return true;
}

int launch_stnorm_fwd(const StnDims& s, const float* x, const float* const* P, float* const* run, float* out, float* ws,
                      hipStream_t st) {
    Plan pl;
    if (!make_plan(s, pl)) return REGT_ERR_ARG;
    const Dims& d = pl.d;
    float* pm = ws + pl.pm_off;
    float* pM = ws + pl.pM_off;
    StartArgs sa{d, x, P[0], P[1], ws + pl.xoff[0], pm, pM};
    hipLaunchKernelGGL(st_start_fwd, dim3(d.nw), dim3(WV), 0, st, sa);
    REGT_CHECK_LAUNCH();
    if (d.sn) {
        hipLaunchKernelGGL(st_sn_final, dim3(d.B * pl.Li[0] * SC), dim3(WV), 0, st, pm, pM, d.N, d.nw, ws + pl.soff[0]);
        REGT_CHECK_LAUNCH();
    }
    for (int i = 0; i < d.nl; ++i) {
        const bool last = i == d.nl - 1;
        LayerFwdArgs a{};
        a.d = d;
        a.p = layer_params(pl, P, run, i);
        a.Li = pl.Li[i], a.dil = pl.dil[i], a.Ln = pl.Li[i] - pl.dil[i];
        a.first = i == 0;
        a.update = d.train;
        a.x = ws + pl.xoff[i];
        a.sstat = ws + pl.soff[i];
        a.xn = last ? nullptr : ws + pl.xoff[i + 1];
        a.pm = pm, a.pM = pM;
        a.skip = ws + pl.skip_off;
        a.e1w = P[2], a.e1b = P[3], a.e2w = P[4], a.e2b = P[5];
        a.out = out;
        int rc;
        switch (d.tn * 2 + d.sn) {
            case 0: rc = layer_fwd_nz<false, false>(a, last, st); break;
            case 1: rc = layer_fwd_nz<false, true>(a, last, st); break;
            case 2: rc = layer_fwd_nz<true, false>(a, last, st); break;
            default: rc = layer_fwd_nz<true, true>(a, last, st); break;
        }
        if (rc) return rc;
        if (d.sn && !last) {
            hipLaunchKernelGGL(st_sn_final, dim3(d.B * pl.Li[i + 1] * SC), dim3(WV), 0, st, pm, pM, d.N, d.nw, ws + pl.soff[i + 1]);
            REGT_CHECK_LAUNCH();
        }
    }
    return REGT_OK;
}

int launch_stnorm_bwd(const StnDims& s, const float* x, const float* const* P, float* const* run, const float* dout, float* const* Gr,
                      const float* ws, float* sc, hipStream_t st) {
    Plan pl;
    if (!make_plan(s, pl)) return REGT_ERR_ARG;
    const Dims& d = pl.d;
    float* slab = sc + pl.sc_slab;
    float* part = sc + pl.sc_part;
    float* dskip = sc + pl.sc_dskip;
    // head
    {
        HeadBwdArgs h{};
        h.d = d;
        h.skip = ws + pl.skip_off, h.dout = dout, h.e1w = P[2], h.e1b = P[3], h.e2w = P[4];
        h.dskip = dskip, h.slab = slab;
        const int O = d.O;
        add_block(h.ob, 0, O, O, SC);                  // dE2 = dout x relu(r1)
        add_block(h.ob, 0, O, O + 3 * SC, 1);          // de2b
        add_block(h.ob, O + SC, SC, O + 2 * SC, SC);   // dE1 = dr1 x relu(skip)
        add_block(h.ob, O + SC, SC, O + 3 * SC, 1);    // de1b
        h.stride = O + 3 * SC + 1;
        const int bytes = WV * h.stride * (int)sizeof(float);
        if (bytes > 64 * 1024)
            if (int rc = want_dynamic_lds<&st_head_bwd>(HEAD_LDS_MAX)) return rc;
        hipLaunchKernelGGL(st_head_bwd, dim3(d.nw), dim3(WV), bytes, st, h);
        REGT_CHECK_LAUNCH();
        SlabSegs sg{};
        add_seg(sg, Gr[4], O * SC);
        add_seg(sg, Gr[5], O);
        add_seg(sg, Gr[2], SC * SC);
        add_seg(sg, Gr[3], SC);
        if (int rc = reduce_slab(pl, slab, part, h.ob.E, sg, st)) return rc;
    }
    const int K = pl.K;
    LayerBwdArgs prev{};                               // the last launched layer (i + 1), read by layer i
    for (int i = d.nl - 1; i >= 0; --i) {
        LayerBwdArgs a{};
        a.d = d;
        a.p = layer_params(pl, P, run, i);
        a.Li = pl.Li[i], a.dil = pl.dil[i], a.Ln = pl.Li[i] - pl.dil[i];
        a.x = ws + pl.xoff[i];
        a.sstat = ws + pl.soff[i];
        a.has_next = i < d.nl - 1;
        if (a.has_next) {
            a.xnext = prev.x, a.sstat_next = prev.sstat, a.ssum_next = sc + pl.sc_ssum[(i + 1) & 1];
            a.dxr_next = prev.dxr, a.dsn_next = prev.dsn, a.sg_next = prev.p.sg;
        }
        a.dskip = dskip;
        a.dxr = sc + pl.sc_dxr[i & 1], a.dsn = sc + pl.sc_dsn[i & 1], a.dtn = sc + pl.sc_dtn, a.dfg = sc + pl.sc_dfg;
        a.pp1 = sc + pl.sc_pp1, a.pp2 = sc + pl.sc_pp2;
        float* const* g = Gr + ST_HEAD_PARAMS + ST_LAYER_PARAMS * i;
        a.dtg = g[8], a.dtb = g[9];
        a.slab = slab;
        const int zz = 0, df = 2 * K, dg = df + SC, hh = dg + SC, dxo = hh + SC, dsk = dxo + SC, one = dsk + SC;
        add_block(a.ob, df, SC, zz, 2 * K);            // filter weight (16, K, 1, 2): entry o * 2K + k * 2 + tap
        add_block(a.ob, dg, SC, zz, 2 * K);            // gate weight
        add_block(a.ob, dxo, SC, hh, SC);              // residual weight
        add_block(a.ob, dsk, SC, hh, SC);              // skip weight
        add_block(a.ob, df, SC, one, 1);
        add_block(a.ob, dg, SC, one, 1);
        add_block(a.ob, dxo, SC, one, 1);
        add_block(a.ob, dsk, SC, one, 1);
        a.stride = one + 1;
        int rc;
        switch (d.tn * 2 + d.sn) {
            case 0: rc = layer_bwd_nz<false, false>(a, st); break;
            case 1: rc = layer_bwd_nz<false, true>(a, st); break;
            case 2: rc = layer_bwd_nz<true, false>(a, st); break;
            default: rc = layer_bwd_nz<true, true>(a, st); break;
        }
        if (rc) return rc;
        SlabSegs sg{};
        add_seg(sg, g[0], SC * 2 * K);
        add_seg(sg, g[2], SC * 2 * K);
        add_seg(sg, g[4], SC * SC);
        add_seg(sg, g[6], SC * SC);
        add_seg(sg, g[1], SC);
        add_seg(sg, g[3], SC);
        add_seg(sg, g[5], SC);
        add_seg(sg, g[7], SC);
        if ((rc = reduce_slab(pl, slab, part, a.ob.E, sg, st))) return rc;
        if (d.sn) {
            float* ssum = sc + pl.sc_ssum[i & 1];
            hipLaunchKernelGGL(st_sn_bwd_final, dim3(d.B * pl.Li[i] * SC), dim3(WV), 0, st, a.pp1, a.pp2, d.nw, ssum);
            REGT_CHECK_LAUNCH();
            hipLaunchKernelGGL(st_sn_param_grad, dim3(1), dim3(WV), 0, st, ssum, d.B * pl.Li[i], g[10], g[11]);
            REGT_CHECK_LAUNCH();
        }
        prev = a;
    }
    // start conv: dW = dx_0 x padded input
    StartBwdArgs sb{};
    sb.d = d;
    sb.dx = prev;                                      // layer 0 as "next": load_dx reads dx_0 with its SNorm backward
    sb.dx.has_next = 1;
    sb.dx.Ln = pl.Li[0];
    sb.dx.xnext = prev.x, sb.dx.sstat_next = prev.sstat, sb.dx.ssum_next = sc + pl.sc_ssum[0];
    sb.dx.dxr_next = prev.dxr, sb.dx.dsn_next = prev.dsn, sb.dx.sg_next = prev.p.sg;
    sb.x = x;
    sb.slab = slab;
    add_block(sb.ob, 0, SC, SC, d.Cin);
    add_block(sb.ob, 0, SC, SC + d.Cin, 1);
    sb.stride = SC + d.Cin + 1;
    const int bytes = WV * sb.stride * (int)sizeof(float);
    if (bytes > 64 * 1024)
        if (int rc = want_dynamic_lds<&st_start_bwd>(START_LDS_MAX)) return rc;
    hipLaunchKernelGGL(st_start_bwd, dim3(d.nw), dim3(WV), bytes, st, sb);
    REGT_CHECK_LAUNCH();
    SlabSegs sg{};
    add_seg(sg, Gr[0], SC * d.Cin);
    add_seg(sg, Gr[1], SC);
    return reduce_slab(pl, slab, part, sb.ob.E, sg, st);
}

}  // namespace regt
