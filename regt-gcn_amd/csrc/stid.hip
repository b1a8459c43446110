// STID (models/STID.py) as run.py builds it (if_time_in_day = if_day_in_week = False): a per-node network
//
//   E   = X We^T + be                    X (node, input_len * input_dim): column l * input_dim + c is feature c of time step l
//   H_0 = [E | node_emb]                 (hidden = embed_dim + node_dim * if_node = 64 or 32)
//   A_l = keep_l * relu(H_l W1_l^T + b1_l) / (1 - p)         (keep = NULL: eval, no dropout, no scaling)
//   H_{l+1} = A_l W2_l^T + b2_l + H_l    l = 0 .. num_layer - 1
//   out = H_L Wr^T + br                  (B, output_len, N, 1)
//
// Mapping.  Persistent workgroups (grid = min(tiles, STID_MAX_WGS)), 256 threads, one per CU; a tile is 64 nodes of one batch
// element and workgroup g takes tiles g, g + grid, ...  The weights are staged in LDS once per workgroup (transposed and padded
// for the forward, as stored for the backward); the layers that do not fit in the 160 KiB (num_layer > 3 at hidden 64) are
// read from global memory instead.  Every contraction runs on v_mfma_f32_32x32x2_f32: the four waves own the 2 x 2 quadrants
// (node half, channel half) of the 64 x 64 result, the activations cross from the accumulator layout to the A-operand
// layout through one LDS tile, and the residual stays in registers.  x is gathered from (B, L, N, C) by the lanes themselves.
//
// Training.  The forward writes H_0 .. H_L and A_0 .. A_{L-1} of every node to a workspace ((2L + 1) * hidden floats per
// node); the backward reads them back rather than recomputing.  The backward is one launch: per
// tile it walks the layers in reverse, and every weight gradient (a sum over all nodes and batch elements) is accumulated in
// the workgroup's own slab, tile by tile in tile order; a second kernel sums the slabs in workgroup order and the per-batch
// node-embedding rows in batch order.  No float atomics: two runs give the same bits.
//
// Keep bits: int32 (num_layer, B, N, hidden / 32), bit j of word w keeps channel 32 w + j.
//
// Limits (checked by regt_stid_* before any launch): embed_dim == node_dim == 32; 1 <= num_layer <= 8; 1 <= input_len <= 255;
// 1 <= input_dim <= in_features <= 256; input_dim * input_len <= 192; 1 <= output_len <= 64; num_nodes, batch >= 1.
#include "lane_helpers.h"
#include "slab_reduce.h"

namespace regt {

namespace {

constexpr int TILE = 64;                  // nodes per tile
constexpr int LD = TILE + 1;              // row stride of an LDS activation tile (conflict-free column walks)
constexpr int LDS_BYTES = 160 * 1024;
constexpr int THREADS = 256;

struct Args {
    int N, B, L, C, D, Kin, hd, NL, O, OP, lds_layers, tpb, ntiles, P;
    float scale;
    const float *x, *node_emb, *we, *be, *wr, *br;
    const float *w1[STID_MAX_LAYERS], *b1[STID_MAX_LAYERS], *w2[STID_MAX_LAYERS], *b2[STID_MAX_LAYERS];
    const unsigned* keep;
    float* out;
    float* ws;
    const float* dout;
    float* slab;
    float* dnode;
};

// acc (32 x 32) += A (32 x K) B (K x 32); fa(k) / fb(k) give this lane's A[lane & 31][k] / B[k][lane & 31]; K even
template <class FA, class FB>
__device__ __forceinline__ f32x16 gemm(f32x16 acc, int K, int lh, FA fa, FB fb) {
    int k0 = 0;
    for (; k0 + 8 <= K; k0 += 8) {             // four steps a round: the operand loads of a round issue ahead of its MFMAs
        const int k = k0 + lh;
        const float a0 = fa(k), a1 = fa(k + 2), a2 = fa(k + 4), a3 = fa(k + 6);
        const float b0 = fb(k), b1 = fb(k + 2), b2 = fb(k + 4), b3 = fb(k + 6);
        acc = mfma32(a0, b0, acc);
        acc = mfma32(a1, b1, acc);
        acc = mfma32(a2, b2, acc);
        acc = mfma32(a3, b3, acc);
    }
    for (; k0 < K; k0 += 2) acc = mfma32(fa(k0 + lh), fb(k0 + lh), acc);
    return acc;
}

__device__ __forceinline__ f32x16 splat(float v) {
    f32x16 r;
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = v;
    return r;
}

// accumulator quadrant -> LDS tile
__device__ __forceinline__ void put_tile(float* s, const f32x16& v, int mh, int nh, int lr, int lh) {
#pragma unroll
    for (int i = 0; i < 16; ++i) s[(mh * 32 + crow(i, lh)) * LD + nh * 32 + lr] = v[i];
}

// accumulator quadrant -> workspace slot (rows of hd floats per node)
__device__ __forceinline__ void put_ws(float* ws, long slot_row0, int hd, const f32x16& v, int nvalid, int mh, int nh, int lr, int lh) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = mh * 32 + crow(i, lh);
        if (r < nvalid) ws[(slot_row0 + r) * hd + nh * 32 + lr] = v[i];
    }
}

// workspace slot -> LDS tile (zero rows beyond the last node)
__device__ __forceinline__ void get_ws(float* s, const float* ws, long slot_row0, int hd, int nvalid, int tid) {
    for (int i = tid; i < TILE * hd; i += THREADS) {
        const int r = i / hd, c = i - r * hd;
        s[r * LD + c] = r < nvalid ? ws[(slot_row0 + r) * hd + c] : 0.f;
    }
}

__global__ __launch_bounds__(THREADS) void stid_fwd_kernel(const Args a) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5, mh = wave & 1, nh = wave >> 1;
    const int hd = a.hd, WLD = hd + 1, WSZ = hd * WLD, Kin = a.Kin, KinP = (Kin + 1) & ~1, OLD = a.OP + 1;
    float* sWe = smem;                        // [KinP][32]   We^T
    float* sB = sWe + KinP * 32;              // be[32], then b1_l[64], b2_l[64] per layer
    float* sWr = sB + 32 + a.NL * 128;        // [hd][OP + 1] Wr^T
    float* sBr = sWr + hd * OLD;              // [64]
    float* sS = sBr + 64;                     // [64][LD]     activation tile
    float* sW = sS + TILE * LD;               // lds_layers x {W1^T, W2^T} [hd][hd + 1]
    for (int i = tid; i < KinP * 32; i += THREADS) {
        const int o = i / KinP, k = i - o * KinP;
        sWe[k * 32 + o] = k < Kin ? a.we[o * Kin + k] : 0.f;
    }
    if (tid < 32) sB[tid] = a.be[tid];
    for (int i = tid; i < a.NL * 128; i += THREADS) {
        const int l = i >> 7, j = i & 127, c = j & 63;
        sB[32 + i] = c < hd ? ((j >> 6) ? a.b2[l] : a.b1[l])[c] : 0.f;
    }
    for (int i = tid; i < hd * a.OP; i += THREADS) {
        const int o = i / hd, k = i - o * hd;
        sWr[k * OLD + o] = o < a.O ? a.wr[o * hd + k] : 0.f;
    }
    if (tid < 64) sBr[tid] = tid < a.O ? a.br[tid] : 0.f;
    for (int l = 0; l < a.lds_layers; ++l)
        for (int i = tid; i < hd * hd; i += THREADS) {
            const int o = i / hd, k = i - o * hd;
            sW[(2 * l) * WSZ + k * WLD + o] = a.w1[l][i];
            sW[(2 * l + 1) * WSZ + k * WLD + o] = a.w2[l][i];
        }
    __syncthreads();

    const bool act = nh * 32 < hd;            // hidden 32: the waves of the upper channel half only keep the barriers
    const int col = nh * 32 + lr;
    const long BN = (long)a.B * a.N;
    const float* sArow = sS + (mh * 32 + lr) * LD;
    for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int b = t / a.tpb, n0 = (t - b * a.tpb) * TILE, nvalid = min(TILE, a.N - n0);
        const long row0 = (long)b * a.N + n0;
        f32x16 h = splat(0.f);
        if (nh == 0) {                         // E = X We^T + be, x gathered from (B, L, N, C)
            const int node = n0 + mh * 32 + lr;
            const bool live = node < a.N;
            const float* xb = a.x + ((long)b * a.L * a.N + (live ? node : 0)) * a.C;
            const long lstride = (long)a.N * a.C;
            h = gemm(splat(sB[lr]), KinP, lh,
                     [&](int k) {
                         const int l = k / a.D, c = k - l * a.D;
                         return live && k < Kin ? xb[l * lstride + c] : 0.f;
                     },
                     [&](int k) { return sWe[k * 32 + lr]; });
        } else if (act) {                      // the node's embedding row
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = mh * 32 + crow(i, lh);
                h[i] = r < nvalid ? a.node_emb[(long)(n0 + r) * 32 + lr] : 0.f;
            }
        }
        if (act) {
            put_tile(sS, h, mh, nh, lr, lh);
            if (a.ws) put_ws(a.ws, row0, hd, h, nvalid, mh, nh, lr, lh);
        }
        __syncthreads();
        for (int l = 0; l < a.NL; ++l) {
            f32x16 y = splat(0.f);
            if (act) {
                y = splat(sB[32 + l * 128 + col]);
                if (l < a.lds_layers) {
                    const float* w = sW + (2 * l) * WSZ + col;
                    y = gemm(y, hd, lh, [&](int k) { return sArow[k]; }, [&](int k) { return w[k * WLD]; });
                } else {
                    const float* w = a.w1[l] + col * hd;
                    y = gemm(y, hd, lh, [&](int k) { return sArow[k]; }, [&](int k) { return w[k]; });
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int r = mh * 32 + crow(i, lh);
                    float v = fmaxf(y[i], 0.f);
                    if (a.keep) {
                        const unsigned word = r < nvalid ? a.keep[(((long)l * BN) + row0 + r) * (hd >> 5) + nh] : 0u;
                        v = ((word >> lr) & 1u) ? v * a.scale : 0.f;
                    }
                    y[i] = v;
                }
            }
            __syncthreads();                   // every wave has read H_l
            if (act) {
                put_tile(sS, y, mh, nh, lr, lh);
                if (a.ws) put_ws(a.ws, (a.NL + 1 + l) * BN + row0, hd, y, nvalid, mh, nh, lr, lh);
            }
            __syncthreads();
            if (act) {
                const float bias = sB[32 + l * 128 + 64 + col];
#pragma unroll
                for (int i = 0; i < 16; ++i) h[i] += bias;
                if (l < a.lds_layers) {
                    const float* w = sW + (2 * l + 1) * WSZ + col;
                    h = gemm(h, hd, lh, [&](int k) { return sArow[k]; }, [&](int k) { return w[k * WLD]; });
                } else {
                    const float* w = a.w2[l] + col * hd;
                    h = gemm(h, hd, lh, [&](int k) { return sArow[k]; }, [&](int k) { return w[k]; });
                }
            }
            __syncthreads();                   // every wave has read A_l
            if (act) {
                put_tile(sS, h, mh, nh, lr, lh);
                if (a.ws) put_ws(a.ws, (l + 1) * BN + row0, hd, h, nvalid, mh, nh, lr, lh);
            }
            __syncthreads();
        }
        f32x16 o = splat(0.f);
        const bool oact = nh * 32 < a.OP;
        if (oact) {
            const float* w = sWr + col;
            o = gemm(splat(sBr[col]), hd, lh, [&](int k) { return sArow[k]; }, [&](int k) { return w[k * OLD]; });
        }
        __syncthreads();                       // every wave has read H_L
        if (oact) put_tile(sS, o, mh, nh, lr, lh);
        __syncthreads();
        for (int i = tid; i < a.O * TILE; i += THREADS) {    // (B, O, N, 1): lanes along the nodes
            const int oc = i >> 6, r = i & 63;
            if (r < nvalid) a.out[((long)b * a.O + oc) * a.N + n0 + r] = sS[r * LD + oc];
        }
        __syncthreads();
    }
}

// slab quadrant helpers: rows x cols block at `p` with row stride ld, this wave's 32 x 32 part (mh, nh)
__device__ __forceinline__ f32x16 slab_get(const float* p, int ld, int rows, int cols, bool first, int mh, int nh, int lr, int lh) {
    f32x16 v = splat(0.f);
    if (first) return v;
    const int c = nh * 32 + lr;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = mh * 32 + crow(i, lh);
        if (r < rows && c < cols) v[i] = p[r * ld + c];
    }
    return v;
}

__device__ __forceinline__ void slab_put(float* p, int ld, int rows, int cols, const f32x16& v, int mh, int nh, int lr, int lh) {
    const int c = nh * 32 + lr;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = mh * 32 + crow(i, lh);
        if (r < rows && c < cols) p[r * ld + c] = v[i];
    }
}

// column sums of an LDS tile (rows in order) accumulated into a slab vector
__device__ __forceinline__ void slab_colsum(float* p, const float* s, int cols, bool first, int tid) {
    if (tid < cols) {
        float v = 0.f;
        for (int r = 0; r < TILE; ++r) v += s[r * LD + tid];
        p[tid] = first ? v : p[tid] + v;
    }
}

__global__ __launch_bounds__(THREADS) void stid_bwd_kernel(const Args a) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5, mh = wave & 1, nh = wave >> 1;
    const int hd = a.hd, WSZ = hd * hd, Kin = a.Kin, O = a.O;
    float* sA = smem;                          // [64][LD] saved activation tile
    float* sG = sA + TILE * LD;                // [64][LD] gradient tile
    float* sWr = sG + TILE * LD;               // [OP][hd] Wr (zero rows beyond O)
    float* sW = sWr + a.OP * hd;               // lds_layers x {W1, W2} [hd][hd]
    for (int i = tid; i < a.OP * hd; i += THREADS) sWr[i] = i < O * hd ? a.wr[i] : 0.f;
    for (int l = 0; l < a.lds_layers; ++l)
        for (int i = tid; i < WSZ; i += THREADS) {
            sW[(2 * l) * WSZ + i] = a.w1[l][i];
            sW[(2 * l + 1) * WSZ + i] = a.w2[l][i];
        }
    __syncthreads();

    const bool act = nh * 32 < hd;
    const int col = nh * 32 + lr, arow = mh * 32 + lr;
    const long BN = (long)a.B * a.N;
    float* slab = a.slab + (long)blockIdx.x * a.P;
    float* gWe = slab;                         // (32, Kin)
    float* gbe = gWe + 32 * Kin;
    float* glay = gbe + 32;                    // per layer: dW1 (hd, hd), db1, dW2, db2
    const int LSZ = 2 * WSZ + 2 * hd;
    float* gWr = glay + a.NL * LSZ;            // (O, hd)
    float* gbr = gWr + O * hd;
    const float* sGrow = sG + arow * LD;
    // weight gradient dW (rows = out, cols = in) += G^T Act over the tile's nodes
    auto wgrad = [&](float* g, int rows, bool first) {
        if (!(act && mh * 32 < rows)) return;
        f32x16 c = slab_get(g, hd, rows, hd, first, mh, nh, lr, lh);
        c = gemm(c, TILE, lh, [&](int k) { return sG[k * LD + arow]; }, [&](int k) { return sA[k * LD + col]; });
        slab_put(g, hd, rows, hd, c, mh, nh, lr, lh);
    };
    bool first = true;
    for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x, first = false) {
        const int b = t / a.tpb, n0 = (t - b * a.tpb) * TILE, nvalid = min(TILE, a.N - n0);
        const long row0 = (long)b * a.N + n0;
        for (int i = tid; i < a.OP * TILE; i += THREADS) {   // dout (B, O, N, 1) -> sG[node][o]
            const int oc = i >> 6, r = i & 63;
            sG[r * LD + oc] = oc < O && r < nvalid ? a.dout[((long)b * O + oc) * a.N + n0 + r] : 0.f;
        }
        get_ws(sA, a.ws, a.NL * BN + row0, hd, nvalid, tid);  // H_L
        __syncthreads();
        wgrad(gWr, O, first);
        slab_colsum(gbr, sG, O, first, tid);
        f32x16 g = splat(0.f);                 // dL/dH_{l+1}, this wave's quadrant
        if (act) {
            const float* w = sWr + col;
            g = gemm(g, (O + 1) & ~1, lh, [&](int k) { return sGrow[k]; }, [&](int k) { return w[k * hd]; });
        }
        __syncthreads();
        if (act) put_tile(sG, g, mh, nh, lr, lh);
        for (int l = a.NL - 1; l >= 0; --l) {
            float* gl = glay + l * LSZ;
            get_ws(sA, a.ws, (a.NL + 1 + l) * BN + row0, hd, nvalid, tid);   // A_l
            __syncthreads();
            wgrad(gl + WSZ + hd, hd, first);                                 // dW2
            slab_colsum(gl + 2 * WSZ + hd, sG, hd, first, tid);              // db2
            f32x16 dy = splat(0.f);
            if (act) {
                if (l < a.lds_layers) {
                    const float* w = sW + (2 * l + 1) * WSZ + col;
                    dy = gemm(dy, hd, lh, [&](int k) { return sGrow[k]; }, [&](int k) { return w[k * hd]; });
                } else {
                    const float* w = a.w2[l] + col;
                    dy = gemm(dy, hd, lh, [&](int k) { return sGrow[k]; }, [&](int k) { return w[k * hd]; });
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {                               // relu and keep gates of A_l
                    const int r = mh * 32 + crow(i, lh);
                    bool on = sA[r * LD + col] > 0.f;
                    if (a.keep && r < nvalid) on = on && ((a.keep[(((long)l * BN) + row0 + r) * (hd >> 5) + nh] >> lr) & 1u);
                    dy[i] = on ? dy[i] * a.scale : 0.f;
                }
            }
            __syncthreads();                   // every wave has read dH_{l+1} and A_l
            if (act) put_tile(sG, dy, mh, nh, lr, lh);
            get_ws(sA, a.ws, l * BN + row0, hd, nvalid, tid);                // H_l
            __syncthreads();
            wgrad(gl, hd, first);                                            // dW1
            slab_colsum(gl + WSZ, sG, hd, first, tid);                       // db1
            if (act) {                                                       // dH_l = dY W1 + dH_{l+1}
                if (l < a.lds_layers) {
                    const float* w = sW + (2 * l) * WSZ + col;
                    g = gemm(g, hd, lh, [&](int k) { return sGrow[k]; }, [&](int k) { return w[k * hd]; });
                } else {
                    const float* w = a.w1[l] + col;
                    g = gemm(g, hd, lh, [&](int k) { return sGrow[k]; }, [&](int k) { return w[k * hd]; });
                }
            }
            __syncthreads();
            if (act) put_tile(sG, g, mh, nh, lr, lh);
        }
        __syncthreads();                       // sG = dH_0
        // dWe (32, Kin) += dE^T X, column blocks of 32 over the waves; X from global
        for (int kb = wave; kb * 32 < Kin; kb += 4) {
            const int kc = kb * 32 + lr;
            const int l = kc / a.D, c = kc - l * a.D;
            const float* xk = a.x + (((long)b * a.L + l) * a.N + n0) * a.C + c;
            const bool kok = kc < Kin;
            f32x16 cw = splat(0.f);
            if (!first) {
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (kok) cw[i] = gWe[crow(i, lh) * Kin + kc];
            }
            cw = gemm(cw, TILE, lh, [&](int k) { return sG[k * LD + lr]; },
                      [&](int k) { return kok && k < nvalid ? xk[(long)k * a.C] : 0.f; });
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (kok) gWe[crow(i, lh) * Kin + kc] = cw[i];
        }
        slab_colsum(gbe, sG, 32, first, tid);
        if (hd == 64)                          // node-embedding rows of this batch element
            for (int i = tid; i < TILE * 32; i += THREADS) {
                const int r = i >> 5, j = i & 31;
                if (r < nvalid) a.dnode[(row0 + r) * 32 + j] = sG[r * LD + 32 + j];
            }
        __syncthreads();
    }
}

// grads = the slabs summed in workgroup order; dnode_emb = the per-batch rows summed in batch order, in the same launch
__global__ __launch_bounds__(256) void stid_reduce_kernel(const float* __restrict__ slab, int G, int P, const SlabSegs sg,
                                                          const float* __restrict__ dnode, int B, long N32, float* __restrict__ gnode) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < P) slab_scatter(sg, e, slab_col_sum<false>(slab, G, P, e));
    else if (gnode && e - P < N32) gnode[e - P] = slab_col_sum<false>(dnode, B, N32, e - P);
}

int hidden(const StidDims& s) { return s.embed_dim + (s.if_node ? s.node_dim : 0); }
long param_floats(const StidDims& s) {
    const int hd = hidden(s);
    return 32L * s.input_dim * s.input_len + 32 + (long)s.num_layer * (2 * hd * hd + 2 * hd) + (long)s.output_len * hd + s.output_len;
}
int tiles(const StidDims& s) { return s.batch * cdiv(s.num_nodes, TILE); }

void fill(Args& a, const StidDims& s, const float* const* P) {
    a.N = s.num_nodes, a.B = s.batch, a.L = s.input_len, a.C = s.in_features, a.D = s.input_dim, a.Kin = s.input_dim * s.input_len;
    a.hd = hidden(s), a.NL = s.num_layer, a.O = s.output_len, a.OP = s.output_len <= 32 ? 32 : 64;
    a.tpb = cdiv(s.num_nodes, TILE), a.ntiles = tiles(s), a.P = (int)param_floats(s);
    a.node_emb = P[0], a.we = P[1], a.be = P[2];
    for (int l = 0; l < s.num_layer; ++l) a.w1[l] = P[3 + 4 * l], a.b1[l] = P[4 + 4 * l], a.w2[l] = P[5 + 4 * l], a.b2[l] = P[6 + 4 * l];
    a.wr = P[3 + 4 * s.num_layer], a.br = P[4 + 4 * s.num_layer];
}

}  // namespace

bool stid_sizes(const StidDims& s, size_t* ws_floats, size_t* scratch_floats) {
    const size_t bn = (size_t)s.batch * s.num_nodes;
    if (ws_floats) *ws_floats = (size_t)(2 * s.num_layer + 1) * bn * hidden(s);
    if (scratch_floats) *scratch_floats = (size_t)min(tiles(s), STID_MAX_WGS) * param_floats(s) + (s.if_node ? bn * 32 : 0);
    return true;
}

int launch_stid_fwd(const StidDims& s, const float* x, const float* const* P, const uint32_t* keep, float* out, float* ws, hipStream_t st) {
    Args a{};
    fill(a, s, P);
    a.x = x, a.keep = keep, a.out = out, a.ws = ws;
    a.scale = keep ? 1.f / (1.f - s.dropout_p) : 1.f;
    const int hd = a.hd, KinP = (a.Kin + 1) & ~1;
    const int fixed = KinP * 32 + 32 + a.NL * 128 + hd * (a.OP + 1) + 64 + TILE * LD, per_layer = 2 * hd * (hd + 1);
    a.lds_layers = min(a.NL, (LDS_BYTES / 4 - fixed) / per_layer);
    const int bytes = (fixed + a.lds_layers * per_layer) * 4;
    if (bytes > 64 * 1024)
        if (int rc = want_dynamic_lds<&stid_fwd_kernel>(LDS_BYTES)) return rc;
    hipLaunchKernelGGL(stid_fwd_kernel, dim3(min(a.ntiles, STID_MAX_WGS)), dim3(THREADS), bytes, st, a);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

int launch_stid_bwd(const StidDims& s, const float* x, const float* const* P, const uint32_t* keep, const float* dout, float* const* G,
                    const float* ws, float* scratch, hipStream_t st) {
    Args a{};
    fill(a, s, P);
    const int grid = min(a.ntiles, STID_MAX_WGS);
    a.x = x, a.keep = keep, a.dout = dout, a.ws = const_cast<float*>(ws);
    a.scale = keep ? 1.f / (1.f - s.dropout_p) : 1.f;
    a.slab = scratch, a.dnode = scratch + (size_t)grid * a.P;
    const int hd = a.hd;
    const int fixed = 2 * TILE * LD + a.OP * hd, per_layer = 2 * hd * hd;
    a.lds_layers = min(a.NL, (LDS_BYTES / 4 - fixed) / per_layer);
    const int bytes = (fixed + a.lds_layers * per_layer) * 4;
    if (bytes > 64 * 1024)
        if (int rc = want_dynamic_lds<&stid_bwd_kernel>(LDS_BYTES)) return rc;
    hipLaunchKernelGGL(stid_bwd_kernel, dim3(grid), dim3(THREADS), bytes, st, a);
    REGT_CHECK_LAUNCH();
    SlabSegs sg{};
    add_seg(sg, G[1], 32 * a.Kin);
    add_seg(sg, G[2], 32);
    for (int l = 0; l < a.NL; ++l) {
        add_seg(sg, G[3 + 4 * l], hd * hd);
        add_seg(sg, G[4 + 4 * l], hd);
        add_seg(sg, G[5 + 4 * l], hd * hd);
        add_seg(sg, G[6 + 4 * l], hd);
    }
    add_seg(sg, G[3 + 4 * a.NL], a.O * hd);
    add_seg(sg, G[4 + 4 * a.NL], a.O);
    const long n32 = s.if_node ? (long)a.N * 32 : 0;
    hipLaunchKernelGGL(stid_reduce_kernel, dim3(cdiv(a.P + n32, 256)), dim3(256), 0, st, a.slab, grid, a.P, sg, a.dnode, a.B, n32,
                       s.if_node ? G[0] : nullptr);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace regt
