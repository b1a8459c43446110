// Input gradient of the TGCN cell in front of the transposed aggregation (regt_tgcn_backward):
//   dAx (N, F) = dzp Gz + drp Gr + dhp Gh = [dzp | drp] (N, 2C) [Gz; Gr] (2C, F) + dhp (N, C) Gh (C, F)
// a skinny GEMM with K = 3C and width F <= 64 that streams the three pre-activation gradients once (3 N C floats, HBM-bound) and writes
// dAx once; dx = A_hat^T dAx is the existing CSR pull over the transposed operator.
//
// A workgroup of four waves owns a tile of 128 rows, a wave 32 of them at the full (padded) width: one or two 32 x 32 fp32 MFMA
// accumulators.  K runs in chunks of 32 through LDS, first the 2C columns of [dzp | drp] against [Gz; Gr], then the C of dhp against Gh:
//   rows     16-byte global loads, eight lanes per 128-byte row piece, stored to As[row][k] with a row stride of 36 floats: the 16-byte
//            LDS reads of a wave (lane -> row lane % 32, floats 4 (lane / 32) .. + 3 of an 8-k group) start at banks 36 i mod 64, which
//            are sixteen distinct multiples of 4 in every 16-lane group the instruction is served in: no conflict
//   weights  Bs[k][col], zero beyond F and beyond the segment's K; lanes 0 .. 31 of a 4-byte read walk 32 consecutive floats of one k
// The contraction index of an MFMA step is free as long as both operands agree: lane half h of step u in group j takes k = 8 j + 4 h + u
// from both, so that a lane's four A values of a group are ONE 16-byte read.
// Order: every element of dAx is one accumulator that receives its 3C products in that fixed k order; no atomics, bit-reproducible.
#include "lane_helpers.h"
#include "kernels.h"

namespace regt {

constexpr int DX_TM = 128, DX_KC = 32, DX_LDA = DX_KC + 4;

template <int NT>
__global__ __launch_bounds__(256) void cell_dx_kernel(const float* __restrict__ dzr, const float* __restrict__ dhp,
                                                      const float* __restrict__ Gzr, const float* __restrict__ Gh,
                                                      float* __restrict__ dAx, int N, int C, int F) {
    constexpr int LDB = NT * 32;
    __shared__ __attribute__((aligned(16))) float As[DX_TM * DX_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[DX_KC * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lh = lane >> 5, lc = lane & 31;
    const long row0 = (long)blockIdx.x * DX_TM;
    f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
    const int ar = tid >> 3, ak = (tid & 7) * 4;      // staging: row ar + 32 pass, floats ak .. ak + 3 of the chunk
    for (int seg = 0; seg < 2; ++seg) {
        const float* A = seg ? dhp : dzr;
        const float* G = seg ? Gh : Gzr;
        const int K = seg ? C : 2 * C;               // = the row stride of A
        for (int k0 = 0; k0 < K; k0 += DX_KC) {
            __syncthreads();                         // the previous chunk has been consumed
#pragma unroll
            for (int pass = 0; pass < DX_TM / 32; ++pass) {
                const int r = ar + 32 * pass;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row0 + r < N && k0 + ak < K) v = *reinterpret_cast<const float4*>(A + (row0 + r) * K + k0 + ak);
                *reinterpret_cast<float4*>(&As[r * DX_LDA + ak]) = v;
            }
            for (int e = tid; e < DX_KC * LDB / 4; e += 256) {
                const int k = e / (LDB / 4), c = (e % (LDB / 4)) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k0 + k < K && c < F) v = *reinterpret_cast<const float4*>(G + (long)(k0 + k) * F + c);
                *reinterpret_cast<float4*>(&Bs[k * LDB + c]) = v;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < DX_KC / 8; ++j) {
                const float4 a = *reinterpret_cast<const float4*>(&As[(wave * 32 + lc) * DX_LDA + 8 * j + 4 * lh]);
                const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int n = 0; n < NT; ++n) acc[n] = mfma32(av[u], Bs[(8 * j + 4 * lh + u) * LDB + n * 32 + lc], acc[n]);
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int col = n * 32 + lc;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long row = row0 + wave * 32 + crow(i, lh);
            if (row < N && col < F) dAx[row * F + col] = acc[n][i];
        }
    }
}

// dzr (N, 2C) = [dzp | drp], dhp (N, C), Gzr (2C, F) = [Gz; Gr], Gh (C, F), dAx (N, F); C % 4 == 0, F % 4 == 0, F <= 64, every
// pointer 16-byte aligned (the caller has checked: api_model.hip regt_tgcn_backward)
int launch_cell_dx(const float* dzr, const float* dhp, const float* Gzr, const float* Gh, float* dAx, int N, int C, int F, hipStream_t st) {
    REGT_CHECK_ARG(N > 0 && C > 0 && C % 4 == 0 && F > 0 && F % 4 == 0 && F <= 64, "cell_dx: N=%d C=%d F=%d (C, F multiples of 4, F <= 64)", N, C, F);
    const dim3 grid((unsigned)cdiv(N, DX_TM));
    if (F <= 32) hipLaunchKernelGGL(cell_dx_kernel<1>, grid, dim3(256), 0, st, dzr, dhp, Gzr, Gh, dAx, N, C, F);
    else hipLaunchKernelGGL(cell_dx_kernel<2>, grid, dim3(256), 0, st, dzr, dhp, Gzr, Gh, dAx, N, C, F);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace regt
