// The snapshot on its way to the aggregation: (N, F, T) time-innermost (the reference's snapshot layout, load_dataset.py:451-457)
// -> (N, T, F) rows, as fp32 or rounded once to bf16, and packed fp32 rows -> bf16 rows.  None of these is an aggregation; they
// sit in front of the kernels of spmm_csr.hip / spmm_panel.hip, which read the rows they write next.
#include <stdlib.h>

#include "gemm_epilogue.h"      // pack_bf16x2: the library's one fp32 -> bf16 pair conversion

namespace regt {

// (N, F, T) time-innermost (the reference's snapshot layout, load_dataset.py:451-457) -> (N, T, F) rows.
__global__ void pack_x_kernel(const float* __restrict__ x, float* __restrict__ xp, long N, int F, int T) {
    const long total = N * F * T;
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        long n = o / ((long)F * T);
        int rem = (int)(o - n * F * T);
        int t = rem / F, f = rem - t * F;
        xp[o] = x[n * F * T + (long)f * T + t];
    }
}

// The same transposition staged through LDS: a workgroup takes NB whole nodes (NB * F * T floats, contiguous on both sides), reads
// them with coalesced 16-byte loads, and writes 16-byte pieces of (node, period) rows.  The snapshot is read exactly once ->
// non-temporal loads, so that the lines of x do not displace the packed rows (which the aggregation reads next) from the
// Infinity Cache.  F % 4 == 0, NB * F * T <= PACK_LDS_FLOATS.
constexpr int PACK_LDS_FLOATS = 4096;
__global__ __launch_bounds__(256) void pack_x_lds_kernel(const float* __restrict__ x, float* __restrict__ xp, int N, int F, int T, int NB) {
    __shared__ float4 tile4[PACK_LDS_FLOATS / 4];
    float* tile = reinterpret_cast<float*>(tile4);
    const int FT = F * T, F4 = F / 4;
    for (long n0 = (long)blockIdx.x * NB; n0 < N; n0 += (long)gridDim.x * NB) {
        const int nb = N - n0 < NB ? (int)(N - n0) : NB;
        const int tot4 = nb * FT / 4;                    // FT % 4 == 0 since F % 4 == 0
        const float4* src = reinterpret_cast<const float4*>(x + n0 * FT);
        for (int i = threadIdx.x; i < tot4; i += 256) {
            float4 v;
            const float* s = reinterpret_cast<const float*>(src + i);
            v.x = __builtin_nontemporal_load(s); v.y = __builtin_nontemporal_load(s + 1);
            v.z = __builtin_nontemporal_load(s + 2); v.w = __builtin_nontemporal_load(s + 3);
            tile4[i] = v;
        }
        __syncthreads();
        float4* dst = reinterpret_cast<float4*>(xp + n0 * FT);
        for (int o = threadIdx.x; o < tot4; o += 256) {  // o = (node, t, f4)
            const int n = o / (T * F4), rem = o - n * T * F4;
            const int t = rem / F4, f = (rem - t * F4) * 4;
            const float* b = tile + n * FT + f * T + t;
            dst[o] = make_float4(b[0], b[T], b[2 * T], b[3 * T]);      // (ordinary stores: the packed rows are read next)
        }
        __syncthreads();
    }
}

// grid-stride launches: one block per `per_block` items, at most `cap` blocks
static unsigned capped_blocks(long items, long per_block, int cap) {
    const int blocks = cdiv(items, per_block);
    return blocks > cap ? cap : blocks;
}
// LDS-staged with non-temporal loads of the snapshot (round 4: profiles/r04_pack_ab.txt -- the other variants measured there are gone);
// rows wider than the LDS tile or unaligned pointers take the element-wise kernel
int launch_pack_x(const float* x, float* xp, int N, int F, int T, hipStream_t st) {
    long total = (long)N * F * T;
    const int FT = F * T;
    if (F % 4 == 0 && FT <= PACK_LDS_FLOATS && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(xp)) & 15) == 0) {
        const int NB = PACK_LDS_FLOATS / FT;
        hipLaunchKernelGGL(pack_x_lds_kernel, dim3(capped_blocks(N, NB, 256 * 16)), dim3(256), 0, st, x, xp, N, F, T, NB);
        REGT_CHECK_LAUNCH();
        return REGT_OK;
    }
    hipLaunchKernelGGL(pack_x_kernel, dim3(capped_blocks(total, 256, 8192)), dim3(256), 0, st, x, xp, (long)N, F, T);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

// bf16 rows for the bf16 arithmetic (REGT_GEMM_MODE=bf16): x, A_hat x and L~ x only ever feed matrix-core operands there, so
// the snapshot is rounded once while it is packed (round to nearest even) and the aggregation reads and writes bf16 rows.
// (N, F, T) fp32 -> (N, T, F) bf16; F % 8 == 0: a thread writes the 16 bytes of 8 consecutive features of one (node, period)
__global__ void pack_x_bf16_kernel(const float* __restrict__ x, uint4* __restrict__ xp, long N, int F, int T) {
    const int f8 = F / 8;
    const long total = N * T * f8;
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long)gridDim.x * blockDim.x) {
        const long nt = o / f8;
        const int f0 = (int)(o - nt * f8) * 8;
        const long n = nt / T;
        const int t = (int)(nt - n * T);
        const float* s = x + n * F * T + (long)f0 * T + t;
        uint4 v;
#define REGT_NTL(k) __builtin_nontemporal_load(s + (k) * (long)T)      /* the snapshot is read once: keep it out of the caches' way */
        v.x = pack_bf16x2(REGT_NTL(0), REGT_NTL(1)); v.y = pack_bf16x2(REGT_NTL(2), REGT_NTL(3)); v.z = pack_bf16x2(REGT_NTL(4), REGT_NTL(5)); v.w = pack_bf16x2(REGT_NTL(6), REGT_NTL(7));
#undef REGT_NTL
        xp[o] = v;
    }
}
// LDS-staged form of the same (see pack_x_lds_kernel): coalesced non-temporal 16-byte reads of whole nodes, 16-byte bf16 pieces out
__global__ __launch_bounds__(256) void pack_x_bf16_lds_kernel(const float* __restrict__ x, uint4* __restrict__ xp, int N, int F, int T, int NB) {
    __shared__ float4 tile4[PACK_LDS_FLOATS / 4];
    const float* tile = reinterpret_cast<const float*>(tile4);
    const int FT = F * T, F8 = F / 8;
    for (long n0 = (long)blockIdx.x * NB; n0 < N; n0 += (long)gridDim.x * NB) {
        const int nb = N - n0 < NB ? (int)(N - n0) : NB;
        const int tot4 = nb * FT / 4, tot8 = nb * FT / 8;
        const float4* src = reinterpret_cast<const float4*>(x + n0 * FT);
        for (int i = threadIdx.x; i < tot4; i += 256) {
            const float* s = reinterpret_cast<const float*>(src + i);
            tile4[i] = make_float4(__builtin_nontemporal_load(s), __builtin_nontemporal_load(s + 1), __builtin_nontemporal_load(s + 2),
                                   __builtin_nontemporal_load(s + 3));
        }
        __syncthreads();
        uint4* dst = xp + n0 * (FT / 8);
        for (int o = threadIdx.x; o < tot8; o += 256) {  // o = (node, t, f8)
            const int n = o / (T * F8), rem = o - n * T * F8;
            const int t = rem / F8, f = (rem - t * F8) * 8;
            const float* b = tile + n * FT + f * T + t;
            dst[o] = make_uint4(pack_bf16x2(b[0], b[T]), pack_bf16x2(b[2 * T], b[3 * T]), pack_bf16x2(b[4 * T], b[5 * T]), pack_bf16x2(b[6 * T], b[7 * T]));
        }
        __syncthreads();
    }
}
int launch_pack_x_bf16(const float* x, void* xp, int N, int F, int T, hipStream_t st) {
    REGT_CHECK_ARG(F % 8 == 0, "pack_x (bf16 rows): F = %d must be a multiple of 8", F);
    const int FT = F * T;
    if (FT <= PACK_LDS_FLOATS && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(xp)) & 15) == 0) {
        const int NB = PACK_LDS_FLOATS / FT;
        hipLaunchKernelGGL(pack_x_bf16_lds_kernel, dim3(capped_blocks(N, NB, 256 * 16)), dim3(256), 0, st, x, reinterpret_cast<uint4*>(xp), N, F, T, NB);
        REGT_CHECK_LAUNCH();
        return REGT_OK;
    }
    const long total = (long)N * T * (F / 8);
    hipLaunchKernelGGL(pack_x_bf16_kernel, dim3(capped_blocks(total, 256, 16384)), dim3(256), 0, st, x, reinterpret_cast<uint4*>(xp), (long)N, F, T);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}
// n8 groups of 8 fp32 -> 8 bf16 (packed rows handed over as fp32 by a caller of regt_forward_packed).  Read once: non-temporal loads, so
// that the fp32 rows do not displace the bf16 rows (read next by the aggregation) from the Infinity Cache.
__global__ void cvt_rows_bf16_kernel(const float4* __restrict__ src, uint4* __restrict__ dst, long n8) {
    for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < n8; o += (long)gridDim.x * blockDim.x) {
        const float* s = reinterpret_cast<const float*>(src + 2 * o);
        float a[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = __builtin_nontemporal_load(s + i);
        dst[o] = make_uint4(pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]), pack_bf16x2(a[4], a[5]), pack_bf16x2(a[6], a[7]));
    }
}
int launch_cvt_rows_bf16(const float* src, void* dst, long n, hipStream_t st) {
    REGT_CHECK_ARG(n % 8 == 0, "cvt_rows_bf16: element count must be a multiple of 8");
    hipLaunchKernelGGL(cvt_rows_bf16_kernel, dim3(capped_blocks(n / 8, 256, 16384)), dim3(256), 0, st, reinterpret_cast<const float4*>(src), reinterpret_cast<uint4*>(dst), n / 8);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace regt
