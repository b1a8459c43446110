// Neighbour aggregation: Y[r, :] = sum_e val[e] * X[col[e], :] over a destination-sorted CSR.
//
// This is the gather / scale / scatter-add of PyG's MessagePassing.propagate (the reference's
// GCNConv / ChebConv call sites) restated as a pull: every output row is owned by one lane group,
// so there are no float atomics and the sum runs in a fixed (edge) order.
//
// Mapping (CDNA4, wave = 64): a group of G lanes owns one row; each lane holds CH float4 column
// chunks, so a neighbour row is fetched with CH coalesced 16-B loads per lane (G*16 contiguous bytes
// per instruction).  The group first pulls up to G (col, val) pairs of its CSR segment with one
// coalesced load and then broadcasts them lane-to-lane (__shfl within the group) -- the segmented
// reduction never touches LDS or atomics.  Two edges are processed per step so that 2*CH gathers
// are in flight per lane before the first FMA.
//
// HBM-bound: algorithmic bytes = read X once + (col,val) + write Y.
#include "spmm_common.h"

namespace regt {

template <int G, int CH>
__global__ __launch_bounds__(256) void spmm_csr_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                       const float* __restrict__ val, const float* __restrict__ X,
                                                       float* __restrict__ Y, int nrows, int nrows_x, int W4, int ld4) {
    constexpr int GROUPS = 256 / G;
    const int gl = threadIdx.x % G;                // lane inside the group
    const int gid = threadIdx.x / G;
    const long W = (long)ld4 * 4;                  // row stride of X and Y; W4 = float4 columns handled by this launch
    for (long row = (long)blockIdx.x * GROUPS + gid; row < nrows; row += (long)gridDim.x * GROUPS) {
        float4 acc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[c] = sp_zero4();
        const int beg = rowptr[row], end = rowptr[row + 1];
        for (int base = beg; base < end; base += G) {
            const int n = end - base < G ? end - base : G;
            int myc = 0;
            float myv = 0.f;
            if (gl < n) { myc = col[base + gl]; myv = val[base + gl]; }
            int e = 0;
            for (; e + 1 < n; e += 2) {
                const int c0 = __shfl(myc, e, G), c1 = __shfl(myc, e + 1, G);
                const float v0 = __shfl(myv, e, G), v1 = __shfl(myv, e + 1, G);
                const float4* x0 = reinterpret_cast<const float4*>(X + (long)c0 * W);
                const float4* x1 = reinterpret_cast<const float4*>(X + (long)c1 * W);
                float4 a[CH], b[CH];
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int ch = gl + c * G;
                    a[c] = ch < W4 ? x0[ch] : sp_zero4();
                    b[c] = ch < W4 ? x1[ch] : sp_zero4();
                }
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    acc[c].x = fmaf(v0, a[c].x, acc[c].x); acc[c].y = fmaf(v0, a[c].y, acc[c].y);
                    acc[c].z = fmaf(v0, a[c].z, acc[c].z); acc[c].w = fmaf(v0, a[c].w, acc[c].w);
                    acc[c].x = fmaf(v1, b[c].x, acc[c].x); acc[c].y = fmaf(v1, b[c].y, acc[c].y);
                    acc[c].z = fmaf(v1, b[c].z, acc[c].z); acc[c].w = fmaf(v1, b[c].w, acc[c].w);
                }
            }
            if (e < n) {
                const int c0 = __shfl(myc, e, G);
                const float v0 = __shfl(myv, e, G);
                const float4* x0 = reinterpret_cast<const float4*>(X + (long)c0 * W);
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int ch = gl + c * G;
                    float4 a = ch < W4 ? x0[ch] : sp_zero4();
                    acc[c].x = fmaf(v0, a.x, acc[c].x); acc[c].y = fmaf(v0, a.y, acc[c].y);
                    acc[c].z = fmaf(v0, a.z, acc[c].z); acc[c].w = fmaf(v0, a.w, acc[c].w);
                }
            }
        }
        float4* y = reinterpret_cast<float4*>(Y + row * W);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int ch = gl + c * G;
            if (ch < W4) y[ch] = acc[c];
        }
    }
}

// The same row-per-lane-group pull with the MERGED operator (two weights per entry, both outputs from one gather): rows of any
// width that is a multiple of 4 floats -- the case the panel kernels (whole 128-byte panels, W % 32 == 0) do not cover, e.g. the
// reference's own TPIMS widths T * F = 48 and 96.  Small graphs only (X lives in the L2s), so no panel schedule is needed.
template <int G, int CH>
__global__ __launch_bounds__(256) void spmm_dual_csr_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                            const float* __restrict__ val_a, const float* __restrict__ val_l,
                                                            const float* __restrict__ X, float* __restrict__ YA, float* __restrict__ YL,
                                                            int nrows, int W4) {
    constexpr int GROUPS = 256 / G;
    const int gl = threadIdx.x % G, gid = threadIdx.x / G;
    const long W = (long)W4 * 4;
    for (long row = (long)blockIdx.x * GROUPS + gid; row < nrows; row += (long)gridDim.x * GROUPS) {
        float4 aa[CH], al[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) aa[c] = al[c] = sp_zero4();
        const int beg = rowptr[row], end = rowptr[row + 1];
        for (int base = beg; base < end; base += G) {
            const int n = end - base < G ? end - base : G;
            int myc = 0;
            float mya = 0.f, myl = 0.f;
            if (gl < n) { myc = col[base + gl]; mya = val_a[base + gl]; myl = val_l[base + gl]; }
            for (int e = 0; e < n; ++e) {
                const int c0 = __shfl(myc, e, G);
                const float va = __shfl(mya, e, G), vl = __shfl(myl, e, G);
                const float4* x0 = reinterpret_cast<const float4*>(X + (long)c0 * W);
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int ch = gl + c * G;
                    const float4 a = ch < W4 ? x0[ch] : sp_zero4();
                    aa[c].x = fmaf(va, a.x, aa[c].x); aa[c].y = fmaf(va, a.y, aa[c].y); aa[c].z = fmaf(va, a.z, aa[c].z); aa[c].w = fmaf(va, a.w, aa[c].w);
                    al[c].x = fmaf(vl, a.x, al[c].x); al[c].y = fmaf(vl, a.y, al[c].y); al[c].z = fmaf(vl, a.z, al[c].z); al[c].w = fmaf(vl, a.w, al[c].w);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int ch = gl + c * G;
            if (ch < W4) {
                reinterpret_cast<float4*>(YA + row * W)[ch] = aa[c];
                reinterpret_cast<float4*>(YL + row * W)[ch] = al[c];
            }
        }
    }
}

// ---- the two lane-group ladders: first rung whose max_w4 holds the row, each with the launch of its instantiation -----------------
// One pass over pass w4 float4 of rows of stride W16, starting at float4 column c4 (whole rows: c4 = 0, w4 = W16).
template <int G, int CH>
static void launch_single(const SpmmPlan& k, const SpmmPtrs& a, int c4, int w4, hipStream_t st) {
    hipLaunchKernelGGL((spmm_csr_kernel<G, CH>), dim3((unsigned)k.grid), dim3(256), 0, st, a.rowptr, a.col, a.val_a, static_cast<const float*>(a.X) + 4L * c4,
                       static_cast<float*>(a.YA) + 4L * c4, k.nnodes * k.nstack, k.x_rows, w4, k.W16);
}
template <int G, int CH>
static void launch_dual(const SpmmPlan& k, const SpmmPtrs& a, int, int, hipStream_t st) {
    hipLaunchKernelGGL((spmm_dual_csr_kernel<G, CH>), dim3((unsigned)k.grid), dim3(256), 0, st, a.rowptr, a.col, a.val_a, a.val_l, static_cast<const float*>(a.X),
                       static_cast<float*>(a.YA), static_cast<float*>(a.YL), k.nnodes, k.W16);
}
template <int G, int CH> static constexpr SpRung single(int max_w4) { return {max_w4, G, CH, launch_single<G, CH>}; }
template <int G, int CH> static constexpr SpRung dual(int max_w4) { return {max_w4, G, CH, launch_dual<G, CH>}; }
// The merged operator has no <32, 3> / <64, 3> rungs: 65..96 and 129..192 float4 take the next power of two there (no measurement
// of three-chunk lane groups with two accumulators is on record; the rungs were never added).
SpLadder spmm_ladder(bool merged) {
    static const SpRung one[] = {single<8, 1>(8), single<16, 1>(16), single<32, 1>(32), single<64, 1>(64), single<32, 3>(96), single<64, 2>(128),
                                 single<64, 3>(192), single<64, 4>(256), single<64, 8>(512)};
    static const SpRung two[] = {dual<8, 1>(8), dual<16, 1>(16), dual<32, 1>(32), dual<64, 1>(64), dual<64, 2>(128),
                                 dual<64, 4>(256), dual<64, 8>(512)};
    return merged ? SpLadder{two, 7} : SpLadder{one, 9};
}

// SP_CSR: one launch over whole rows.  SP_CSR_PASSES (rows wider than 2048 floats: the hidden-state aggregation of the stacked-conv
// baseline, T * 512): column passes of pass16 float4 each.
int spmm_launch_csr(const SpmmPlan& k, const SpmmPtrs& a, hipStream_t st) {
    const int pass16 = k.family == SP_CSR_PASSES ? k.pass16 : k.W16;
    for (int c4 = 0; c4 < k.W16; c4 += pass16) {
        k.rung->launch(k, a, c4, k.W16 - c4 < pass16 ? k.W16 - c4 : pass16, st);
        REGT_CHECK_LAUNCH();
    }
    return REGT_OK;
}

}  // namespace regt
