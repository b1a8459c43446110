// One torch.nn.GRU layer (hidden 256, gates stacked r, z, n) over a whole sequence in one persistent launch per direction.
//
// A workgroup owns a tile of GRU_RT = 8 batch rows from the first step to the last; it never waits for another workgroup.  The
// hidden state stays in LDS between steps.  W_hh (768 x 256 fp32, 786 KB) fits neither LDS nor the registers of a CU: it is
// streamed from L2 every step, from a copy repacked once per call as [k / 4][column][4] so that a wave reads 1 KB contiguous per
// load.  The contraction runs on the packed-FMA VALU (two batch rows per lane operand): 1024 threads split K four ways, leave
// their partial sums in LDS and every thread finishes two (row, unit) pairs in a fixed order.  The input projection (K = T <= 255)
// is part of the step.  The backward is the same shape run in reverse; the weight gradients are contractions over all steps and
// rows, formed afterwards per row chunk and summed in chunk order: no float atomics anywhere, two runs give the same bits.
#include "lane_helpers.h"
#include "slab_reduce.h"

namespace regt {

namespace {

constexpr int H = GRU_HIDDEN, G = 3 * GRU_HIDDEN, RT = GRU_RT, KS = 4, THREADS = H * KS;
constexpr int FWD_LDS_FLOATS = KS * 4 * RT * H + RT * H + RT * 256;       // partial sums, h, x (T padded to <= 256)
constexpr int BWD_LDS_FLOATS = G * RT + KS * RT * H;
static_assert(RT == 2 * KS, "every thread finishes RT / KS = 2 rows of its hidden unit");

typedef float f32x2 __attribute__((ext_vector_type(2)));

// dst[(k4 * ncol + col) * 4 + kk] = src[col * s_col + (4 k4 + kk) * s_k], zero for 4 k4 + kk >= K
__global__ void gru_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int ncol, int K, long s_col, long s_k) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)((K + 3) / 4) * ncol * 4;
    if (i >= total) return;
    const int kk = (int)(i & 3), col = (int)((i >> 2) % ncol), k = (int)((i >> 2) / ncol) * 4 + kk;
    dst[i] = k < K ? src[col * s_col + k * s_k] : 0.f;
}

struct FwdArgs {
    int seq, rows, T, T4, training;
    long sx_seq, sx_row, sx_t;
    const float *x, *whhp, *wihp, *b_ih, *b_hh, *h0;
    float *out, *h_last, *hs, *gates;
};

// acc[p] += lds[k][2p .. 2p+1] * w for the RT rows of one k (rows are the minor index of the LDS tile)
__device__ __forceinline__ void load_rows(const float* p, f32x2 (&v)[RT / 2]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = f32x2{a.x, a.y}; v[1] = f32x2{a.z, a.w}; v[2] = f32x2{b.x, b.y}; v[3] = f32x2{b.z, b.w};
}

__global__ __launch_bounds__(THREADS) void gru_fwd_kernel(const FwdArgs a) {
    extern __shared__ float smem[];
    float* part = smem;                          // [KS][4][RT][H]
    float* h_s = part + KS * 4 * RT * H;         // [H][RT]
    float* x_s = h_s + RT * H;                   // [T4][RT]
    const int tid = threadIdx.x, j = tid & (H - 1), q = tid >> 8;
    const int row0 = blockIdx.x * RT, nrow = min(RT, a.rows - row0);
    const f32x4* whh = reinterpret_cast<const f32x4*>(a.whhp);
    const f32x4* wih = reinterpret_cast<const f32x4*>(a.wihp);
    const float bi_r = a.b_ih[j] + a.b_hh[j], bi_z = a.b_ih[H + j] + a.b_hh[H + j], b_in = a.b_ih[2 * H + j], b_hn = a.b_hh[2 * H + j];
    const int nx = a.T4 * RT;

    // x elements of this thread: e -> (k = e / RT, r = e % RT); zero outside the input and the tile
    auto load_x = [&](int t, float (&xv)[2]) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + u * THREADS, k = e / RT, r = e % RT;
            xv[u] = (e < nx && k < a.T && r < nrow) ? a.x[t * a.sx_seq + (long)(row0 + r) * a.sx_row + k * a.sx_t] : 0.f;
        }
    };
    auto store_x = [&](const float (&xv)[2]) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + u * THREADS;
            if (e < nx) x_s[e] = xv[u];
        }
    };

    for (int e = tid; e < RT * H; e += THREADS) {
        const int k = e / RT, r = e % RT;
        const float v = (a.h0 && r < nrow) ? a.h0[(long)(row0 + r) * H + k] : 0.f;
        h_s[e] = v;
        if (a.training && r < nrow) a.hs[(long)(row0 + r) * H + k] = v;
    }
    float xv[2];
    load_x(0, xv);
    store_x(xv);
    __syncthreads();

    for (int t = 0; t < a.seq; ++t) {
        if (t + 1 < a.seq) load_x(t + 1, xv);                    // in flight across the contraction
        f32x2 acc[4][RT / 2];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int p = 0; p < RT / 2; ++p) acc[g][p] = f32x2{0.f, 0.f};
        // hidden part: k in [64 q, 64 q + 64)
#pragma unroll 2
        for (int k4 = q * (H / 4 / KS); k4 < (q + 1) * (H / 4 / KS); ++k4) {
            const f32x4 w0 = whh[k4 * G + j], w1 = whh[k4 * G + H + j], w2 = whh[k4 * G + 2 * H + j];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                f32x2 hv[RT / 2];
                load_rows(h_s + (4 * k4 + kk) * RT, hv);
#pragma unroll
                for (int p = 0; p < RT / 2; ++p) {
                    acc[0][p] += hv[p] * w0[kk];
                    acc[1][p] += hv[p] * w1[kk];
                    acc[2][p] += hv[p] * w2[kk];
                }
            }
        }
        // input part: k4 = q, q + KS, ...
        for (int k4 = q; k4 < a.T4 / 4; k4 += KS) {
            const f32x4 w0 = wih[k4 * G + j], w1 = wih[k4 * G + H + j], w2 = wih[k4 * G + 2 * H + j];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                f32x2 v[RT / 2];
                load_rows(x_s + (4 * k4 + kk) * RT, v);
#pragma unroll
                for (int p = 0; p < RT / 2; ++p) {
                    acc[0][p] += v[p] * w0[kk];
                    acc[1][p] += v[p] * w1[kk];
                    acc[3][p] += v[p] * w2[kk];
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int p = 0; p < RT / 2; ++p) {
                part[((q * 4 + g) * RT + 2 * p) * H + j] = acc[g][p].x;
                part[((q * 4 + g) * RT + 2 * p + 1) * H + j] = acc[g][p].y;
            }
        __syncthreads();
        // finish rows 2 q and 2 q + 1 of hidden unit j: the KS partial sums in a fixed order
#pragma unroll
        for (int rr = 0; rr < RT / KS; ++rr) {
            const int r = q * (RT / KS) + rr;
            float s[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float v = part[((0 * 4 + g) * RT + r) * H + j];
#pragma unroll
                for (int qq = 1; qq < KS; ++qq) v += part[((qq * 4 + g) * RT + r) * H + j];
                s[g] = v;
            }
            const float rg = sigm(s[0] + bi_r), zg = sigm(s[1] + bi_z), hn = s[2] + b_hn;
            const float ng = tanhf(s[3] + b_in + rg * hn);
            const float hp = h_s[j * RT + r], hnew = (1.f - zg) * ng + zg * hp;
            h_s[j * RT + r] = hnew;
            if (r < nrow) {
                const long m = (long)t * a.rows + row0 + r;
                if (a.out) a.out[m * H + j] = hnew;
                if (a.training) {
                    a.hs[(m + a.rows) * H + j] = hnew;
                    float* gp = a.gates + m * 4 * H + j;
                    gp[0] = rg; gp[H] = zg; gp[2 * H] = ng; gp[3 * H] = hn;
                }
                if (a.h_last && t == a.seq - 1) a.h_last[(long)(row0 + r) * H + j] = hnew;
            }
        }
        if (t + 1 < a.seq) store_x(xv);
        __syncthreads();
    }
}

struct BwdArgs {
    int seq, rows;
    const float *whhq, *hs, *gates, *dout, *dh_last;
    float *dgi, *dghn, *dh0;
};

__global__ __launch_bounds__(THREADS) void gru_bwd_kernel(const BwdArgs a) {
    extern __shared__ float smem[];
    float* dg_s = smem;                  // [G][RT]: dr, dz, dn * r (what W_hh carries back)
    float* part = dg_s + G * RT;         // [KS][RT][H]
    const int tid = threadIdx.x, j = tid & (H - 1), q = tid >> 8;
    const int row0 = blockIdx.x * RT, nrow = min(RT, a.rows - row0);
    const f32x4* whh = reinterpret_cast<const f32x4*>(a.whhq);
    constexpr int RP = RT / KS;
    float dh[RP], sv[RP][6];             // saved r, z, n, hn, h_prev and the upstream gradient of the step being loaded

    auto load_step = [&](int t) {
#pragma unroll
        for (int rr = 0; rr < RP; ++rr) {
            const int r = q * RP + rr;
            if (r < nrow) {
                const long m = (long)t * a.rows + row0 + r;
                const float* gp = a.gates + m * 4 * H + j;
                sv[rr][0] = gp[0]; sv[rr][1] = gp[H]; sv[rr][2] = gp[2 * H]; sv[rr][3] = gp[3 * H];
                sv[rr][4] = a.hs[m * H + j];
                sv[rr][5] = a.dout ? a.dout[m * H + j] : 0.f;
            } else {
#pragma unroll
                for (int u = 0; u < 6; ++u) sv[rr][u] = 0.f;
            }
        }
    };
#pragma unroll
    for (int rr = 0; rr < RP; ++rr) {
        const int r = q * RP + rr;
        dh[rr] = (a.dh_last && r < nrow) ? a.dh_last[(long)(row0 + r) * H + j] : 0.f;
    }
    load_step(a.seq - 1);

    for (int t = a.seq - 1; t >= 0; --t) {
        float keep[RP];
#pragma unroll
        for (int rr = 0; rr < RP; ++rr) {
            const int r = q * RP + rr;
            const float rg = sv[rr][0], zg = sv[rr][1], ng = sv[rr][2], hn = sv[rr][3], hp = sv[rr][4], d = dh[rr] + sv[rr][5];
            const float dnp = d * (1.f - zg) * (1.f - ng * ng), dzp = d * (hp - ng) * zg * (1.f - zg);
            const float drp = dnp * hn * rg * (1.f - rg), dhn = dnp * rg;
            keep[rr] = d * zg;
            dg_s[j * RT + r] = drp;
            dg_s[(H + j) * RT + r] = dzp;
            dg_s[(2 * H + j) * RT + r] = dhn;
            if (r < nrow) {
                const long m = (long)t * a.rows + row0 + r;
                float* gp = a.dgi + m * G + j;
                gp[0] = drp; gp[H] = dzp; gp[2 * H] = dnp;
                a.dghn[m * H + j] = dhn;
            }
        }
        __syncthreads();
        if (t > 0) load_step(t - 1);                                 // in flight across the contraction
        f32x2 acc[RT / 2];
#pragma unroll
        for (int p = 0; p < RT / 2; ++p) acc[p] = f32x2{0.f, 0.f};
#pragma unroll 4
        for (int c4 = q * (G / 4 / KS); c4 < (q + 1) * (G / 4 / KS); ++c4) {
            const f32x4 w = whh[c4 * H + j];
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                f32x2 v[RT / 2];
                load_rows(dg_s + (4 * c4 + cc) * RT, v);
#pragma unroll
                for (int p = 0; p < RT / 2; ++p) acc[p] += v[p] * w[cc];
            }
        }
#pragma unroll
        for (int p = 0; p < RT / 2; ++p) {
            part[(q * RT + 2 * p) * H + j] = acc[p].x;
            part[(q * RT + 2 * p + 1) * H + j] = acc[p].y;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < RP; ++rr) {
            const int r = q * RP + rr;
            float v = part[(0 * RT + r) * H + j];
#pragma unroll
            for (int qq = 1; qq < KS; ++qq) v += part[(qq * RT + r) * H + j];
            dh[rr] = keep[rr] + v;
        }
        // the next step's dg_s writes come after this step's reads (second barrier); its part writes after its own first barrier
    }
    if (a.dh0) {
#pragma unroll
        for (int rr = 0; rr < RP; ++rr) {
            const int r = q * RP + rr;
            if (r < nrow) a.dh0[(long)(row0 + r) * H + j] = dh[rr];
        }
    }
}

// ---- weight gradients: slab[chunk][c][k] = sum over the chunk's rows m of P[m][c] Q[m][k], plus the column sums of P ----
// P column c comes from p1 (c < 512, row stride 768) or p2 (c >= 512, row stride ld2): the input and the hidden gradients differ
// only in the n block.  Q row m = (step, row) is addressed through three strides, so x is read in place.
struct WgArgs {
    const float *p1, *p2, *qm;
    long ld2, sq_seq, sq_row, sq_t;
    long M;
    int rows, nin, chunk;
    float* slab;
};

__global__ __launch_bounds__(256) void gru_wgrad_kernel(const WgArgs a) {
    __shared__ float Ps[16][64], Qs[16][64];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int c0 = blockIdx.x * 64, k0 = blockIdx.y * 64, ch = blockIdx.z;
    const long m0 = (long)ch * a.chunk, m1 = min(a.M, m0 + a.chunk);
    const float* pp = c0 < 2 * H ? a.p1 + c0 : a.p2 + (c0 - 2 * H);
    const long ldp = c0 < 2 * H ? G : a.ld2;
    float acc[4][4] = {};
    float csum = 0.f;
    for (long mb = m0; mb < m1; mb += 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i, mm = e >> 6, cc = e & 63;
            const long m = mb + mm;
            const bool in = m < m1;
            Ps[mm][cc] = in ? pp[m * ldp + cc] : 0.f;
            const int k = k0 + cc;
            Qs[mm][cc] = (in && k < a.nin) ? a.qm[(m / a.rows) * a.sq_seq + (m % a.rows) * a.sq_row + k * a.sq_t] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int mm = 0; mm < 16; ++mm) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(&Ps[mm][4 * ty]), qv = *reinterpret_cast<const f32x4*>(&Qs[mm][4 * tx]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] += pv[u] * qv[v];
        }
        if (blockIdx.y == 0 && tid < 64) {
#pragma unroll
            for (int mm = 0; mm < 16; ++mm) csum += Ps[mm][tid];
        }
        __syncthreads();
    }
    float* sl = a.slab + (long)ch * ((long)G * a.nin + G);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int k = k0 + 4 * tx + v;
            if (k < a.nin) sl[(long)(c0 + 4 * ty + u) * a.nin + k] = acc[u][v];
        }
    if (blockIdx.y == 0 && tid < 64) sl[(long)G * a.nin + c0 + tid] = csum;
}

__global__ void relu_mask_kernel(const float* __restrict__ y, float* __restrict__ d, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !(y[i] > 0.f)) d[i] = 0.f;
}

void wgrad_chunking(long M, int* chunk, int* nchunks) {
    long c = ((M + 63) / 64 + 15) / 16 * 16;
    if (c < 256) c = 256;
    *chunk = (int)c;
    *nchunks = (int)((M + c - 1) / c);
}

struct WsLayout { size_t whhp, wihp, hs, gates, total; };
WsLayout ws_layout(const GruDims& s) {
    WsLayout L;
    const size_t T4 = (size_t)(s.input_size + 3) / 4 * 4, M = (size_t)s.seq_len * s.rows;
    L.whhp = 0;
    L.wihp = (size_t)H * G;
    L.hs = L.wihp + T4 * G;
    L.gates = L.hs + (s.training ? (M + s.rows) * H : 0);
    L.total = L.gates + (s.training ? M * 4 * H : 0);
    return L;
}

struct ScLayout { size_t whhq, dgi, dghn, slab, total; };
ScLayout sc_layout(const GruDims& s) {
    ScLayout L;
    const size_t M = (size_t)s.seq_len * s.rows;
    int chunk, nchunks;
    wgrad_chunking((long)M, &chunk, &nchunks);
    L.whhq = 0;
    L.dgi = (size_t)G * H;
    L.dghn = L.dgi + M * G;
    L.slab = L.dghn + M * H;
    L.total = L.slab + (size_t)nchunks * ((size_t)G * H + G);        // the hidden gradient's slab; the input one (T <= 255) is smaller
    return L;
}

}  // namespace

void gru_sizes(const GruDims& s, size_t* ws_floats, size_t* scratch_floats) {
    if (ws_floats) *ws_floats = ws_layout(s).total;
    if (scratch_floats) *scratch_floats = sc_layout(s).total;
}

int launch_relu_mask(const float* y, float* d, long n, hipStream_t st) {
    hipLaunchKernelGGL(relu_mask_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, y, d, n);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

int launch_gru_fwd(const GruDims& s, const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                   const float* h0, float* out, float* h_last, float* ws, hipStream_t st) {
    const WsLayout L = ws_layout(s);
    const int T = s.input_size, T4 = (T + 3) / 4 * 4;
    // W_hh[c][k] -> [k / 4][c][4], W_ih[c][k] -> [k / 4][c][4] (zero padded to T4)
    hipLaunchKernelGGL(gru_pack_kernel, dim3(cdiv((long)H * G, 256)), dim3(256), 0, st, w_hh, ws + L.whhp, G, H, (long)H, 1L);
    REGT_CHECK_LAUNCH();
    hipLaunchKernelGGL(gru_pack_kernel, dim3(cdiv((long)T4 * G, 256)), dim3(256), 0, st, w_ih, ws + L.wihp, G, T, (long)T, 1L);
    REGT_CHECK_LAUNCH();
    FwdArgs a{};
    a.seq = s.seq_len; a.rows = s.rows; a.T = T; a.T4 = T4; a.training = s.training;
    a.sx_seq = s.x_stride_seq; a.sx_row = s.x_stride_row; a.sx_t = s.x_stride_t;
    a.x = x; a.whhp = ws + L.whhp; a.wihp = ws + L.wihp; a.b_ih = b_ih; a.b_hh = b_hh; a.h0 = h0;
    a.out = out; a.h_last = h_last;
    a.hs = s.training ? ws + L.hs : nullptr;
    a.gates = s.training ? ws + L.gates : nullptr;
    constexpr int bytes = FWD_LDS_FLOATS * 4;
    static_assert(bytes <= 160 * 1024, "forward LDS");
    if (int rc = want_dynamic_lds<&gru_fwd_kernel>(bytes)) return rc;
    hipLaunchKernelGGL(gru_fwd_kernel, dim3(cdiv(s.rows, RT)), dim3(THREADS), bytes, st, a);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

int launch_gru_bwd(const GruDims& s, const float* x, const float* w_hh, const float* dout, const float* dh_last, float* const* grads,
                   float* dh0, const float* ws, float* scratch, hipStream_t st) {
    const WsLayout L = ws_layout(s);
    const ScLayout C = sc_layout(s);
    const long M = (long)s.seq_len * s.rows;
    // W_hh[c][j] -> [c / 4][j][4]
    hipLaunchKernelGGL(gru_pack_kernel, dim3(cdiv((long)H * G, 256)), dim3(256), 0, st, w_hh, scratch + C.whhq, H, G, 1L, (long)H);
    REGT_CHECK_LAUNCH();
    BwdArgs a{};
    a.seq = s.seq_len; a.rows = s.rows;
    a.whhq = scratch + C.whhq; a.hs = ws + L.hs; a.gates = ws + L.gates; a.dout = dout; a.dh_last = dh_last;
    a.dgi = scratch + C.dgi; a.dghn = scratch + C.dghn; a.dh0 = dh0;
    constexpr int bytes = BWD_LDS_FLOATS * 4;
    static_assert(bytes <= 64 * 1024, "backward LDS");
    hipLaunchKernelGGL(gru_bwd_kernel, dim3(cdiv(s.rows, RT)), dim3(THREADS), bytes, st, a);
    REGT_CHECK_LAUNCH();
    int chunk, nchunks;
    wgrad_chunking(M, &chunk, &nchunks);
    for (int pass = 0; pass < 2; ++pass) {                       // 0: dW_ih, db_ih from (dgi, x); 1: dW_hh, db_hh from (dgh, h_prev)
        WgArgs w{};
        w.p1 = scratch + C.dgi;
        w.M = M; w.rows = s.rows; w.chunk = chunk; w.slab = scratch + C.slab;
        if (pass == 0) {
            w.p2 = scratch + C.dgi + 2 * H; w.ld2 = G;
            w.qm = x; w.sq_seq = s.x_stride_seq; w.sq_row = s.x_stride_row; w.sq_t = s.x_stride_t; w.nin = s.input_size;
        } else {
            w.p2 = scratch + C.dghn; w.ld2 = H;
            w.qm = ws + L.hs; w.sq_seq = (long)s.rows * H; w.sq_row = H; w.sq_t = 1; w.nin = H;
        }
        hipLaunchKernelGGL(gru_wgrad_kernel, dim3(G / 64, cdiv(w.nin, 64), nchunks), dim3(256), 0, st, w);
        REGT_CHECK_LAUNCH();
        const long nw = (long)G * w.nin;
        SlabSegs sg{};
        add_seg(sg, grads[pass], nw);
        add_seg(sg, grads[2 + pass], G);
        if (int rc = launch_slab_reduce_final<true>(w.slab, nchunks, nw + G, sg, st)) return rc;      // the chunks in order, seeded with chunk 0
    }
    return REGT_OK;
}

}  // namespace regt
