// Transposed dual aggregation with the unpack as its epilogue (regt_input_gradient):
//   dXp[i, :] = init[i, :] + sum_e (a_e P[col_e, :] + l_e Q[col_e, :])          rows of W = T F floats, packed (t, f)
//   dx[i, f, t] = dXp[i, t F + f]                                                the reference's (N, F, T) layout
// over the CSR of the TRANSPOSED merged operator (two weights per entry: A_hat^T and L~^T; graph.transpose_csr orders the entries of a row
// by their original row id, which fixes the order of the sum).  The lane-group pull of spmm_csr.hip: G lanes own a row, pull up to G
// (col, a, l) triples with one coalesced load, broadcast them lane to lane, and gather both inputs of two entries (4 CH 16-byte loads
// per lane) before the first FMA.  Rows wider than G CH float4 run as column passes (blockIdx.y).  An empty row gives `init`.
// The unpack is the epilogue, not a launch of its own: a lane's float4 holds four features of ONE period (F % 4 == 0), and the row's T F
// floats land in the same T F floats of dx, only permuted -- four 4-byte stores per float4 into lines the same lane group completes at
// once, against a second launch that would read and write N T F floats again (a quarter more HBM traffic for this stage).
#include <limits.h>

#include "spmm_common.h"

namespace regt {

template <int G, int CH>
__global__ __launch_bounds__(256) void spmm_dual_t_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val_a,
                                                          const float* __restrict__ val_l, const float* __restrict__ P, const float* __restrict__ Q,
                                                          const float* __restrict__ init, float* __restrict__ dx, int nrows, int W4, int F, int T) {
    constexpr int GROUPS = 256 / G;
    const int gl = threadIdx.x % G, gid = threadIdx.x / G;
    const long W = (long)W4 * 4;
    const int ch0 = blockIdx.y * (G * CH) + gl;      // this lane's float4 columns: ch0 + c G
    for (long row = (long)blockIdx.x * GROUPS + gid; row < nrows; row += (long)gridDim.x * GROUPS) {
        float4 acc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int ch = ch0 + c * G;
            acc[c] = ch < W4 ? reinterpret_cast<const float4*>(init + row * W)[ch] : sp_zero4();
        }
        const int beg = rowptr[row], end = rowptr[row + 1];
        for (int base = beg; base < end; base += G) {
            const int n = end - base < G ? end - base : G;
            int myc = 0;
            float mya = 0.f, myl = 0.f;
            if (gl < n) { myc = col[base + gl]; mya = val_a[base + gl]; myl = val_l[base + gl]; }
            for (int e = 0; e < n; e += 2) {
                const bool two = e + 1 < n;              // (uniform over the group)
                const int c0 = __shfl(myc, e, G), c1 = __shfl(myc, two ? e + 1 : e, G);
                const float a0 = __shfl(mya, e, G), l0 = __shfl(myl, e, G);
                const float a1 = two ? __shfl(mya, e + 1, G) : 0.f, l1 = two ? __shfl(myl, e + 1, G) : 0.f;
                const float4* p0 = reinterpret_cast<const float4*>(P + (long)c0 * W);
                const float4* q0 = reinterpret_cast<const float4*>(Q + (long)c0 * W);
                const float4* p1 = reinterpret_cast<const float4*>(P + (long)c1 * W);
                const float4* q1 = reinterpret_cast<const float4*>(Q + (long)c1 * W);
                float4 vp0[CH], vq0[CH], vp1[CH], vq1[CH];
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int ch = ch0 + c * G;
                    const bool in = ch < W4;
                    vp0[c] = in ? p0[ch] : sp_zero4();
                    vq0[c] = in ? q0[ch] : sp_zero4();
                    vp1[c] = in && two ? p1[ch] : sp_zero4();
                    vq1[c] = in && two ? q1[ch] : sp_zero4();
                }
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    acc[c].x = fmaf(a0, vp0[c].x, acc[c].x); acc[c].y = fmaf(a0, vp0[c].y, acc[c].y);
                    acc[c].z = fmaf(a0, vp0[c].z, acc[c].z); acc[c].w = fmaf(a0, vp0[c].w, acc[c].w);
                    acc[c].x = fmaf(l0, vq0[c].x, acc[c].x); acc[c].y = fmaf(l0, vq0[c].y, acc[c].y);
                    acc[c].z = fmaf(l0, vq0[c].z, acc[c].z); acc[c].w = fmaf(l0, vq0[c].w, acc[c].w);
                    if (two) {
                        acc[c].x = fmaf(a1, vp1[c].x, acc[c].x); acc[c].y = fmaf(a1, vp1[c].y, acc[c].y);
                        acc[c].z = fmaf(a1, vp1[c].z, acc[c].z); acc[c].w = fmaf(a1, vp1[c].w, acc[c].w);
                        acc[c].x = fmaf(l1, vq1[c].x, acc[c].x); acc[c].y = fmaf(l1, vq1[c].y, acc[c].y);
                        acc[c].z = fmaf(l1, vq1[c].z, acc[c].z); acc[c].w = fmaf(l1, vq1[c].w, acc[c].w);
                    }
                }
            }
        }
        float* out = dx + row * W;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int ch = ch0 + c * G;
            if (ch < W4) {
                const int w = ch * 4, t = w / F, f = w - t * F;
                float* o = out + (long)f * T + t;
                o[0] = acc[c].x; o[T] = acc[c].y; o[2L * T] = acc[c].z; o[3L * T] = acc[c].w;
            }
        }
    }
}

template <int G, int CH>
static void launch_t(const int* rowptr, const int* col, const float* val_a, const float* val_l, const float* P, const float* Q, const float* init,
                     float* dx, int nrows, int W4, int F, int T, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(nrows, 256 / G), (unsigned)cdiv(W4, G * CH));
    hipLaunchKernelGGL((spmm_dual_t_kernel<G, CH>), grid, dim3(256), 0, st, rowptr, col, val_a, val_l, P, Q, init, dx, nrows, W4, F, T);
}

// P, Q, init (nrows, T F) packed rows, dx (nrows, F, T); F % 4 == 0; every float pointer 16-byte aligned; col entries in [0, nrows)
int launch_spmm_dual_t(const int* rowptr, const int* col, const float* val_a, const float* val_l, const float* P, const float* Q,
                       const float* init, float* dx, int nrows, int F, int T, hipStream_t st) {
    REGT_CHECK_ARG(nrows > 0 && F > 0 && F % 4 == 0 && T > 0 && (long)F * T <= INT_MAX / 4, "spmm_dual_t: nrows=%d F=%d T=%d (F a multiple of 4)", nrows, F, T);
    const int W4 = F * T / 4;
    if (W4 <= 8) launch_t<8, 1>(rowptr, col, val_a, val_l, P, Q, init, dx, nrows, W4, F, T, st);
    else if (W4 <= 16) launch_t<16, 1>(rowptr, col, val_a, val_l, P, Q, init, dx, nrows, W4, F, T, st);
    else if (W4 <= 32) launch_t<32, 1>(rowptr, col, val_a, val_l, P, Q, init, dx, nrows, W4, F, T, st);
    else if (W4 <= 64) launch_t<64, 1>(rowptr, col, val_a, val_l, P, Q, init, dx, nrows, W4, F, T, st);
    else if (W4 <= 128) launch_t<64, 2>(rowptr, col, val_a, val_l, P, Q, init, dx, nrows, W4, F, T, st);
    else launch_t<64, 4>(rowptr, col, val_a, val_l, P, Q, init, dx, nrows, W4, F, T, st);      // column passes of 256 float4
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace regt
