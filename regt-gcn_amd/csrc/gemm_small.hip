// Tiny strided batched GEMMs C = A B for the (C x F)-sized weight compositions and their backward: one launch per product
// (small_gemm_kernel) or up to SG_MAX_TASKS products in one launch (small_gemm_multi_kernel).  VALU kernels: no matrix core, no
// epilogue functor -- nothing here is shared with the tiled GEMMs but the launcher interface of kernels.h.
#include "kernels.h"

namespace regt {

// One output element per group of 8 adjacent lanes: the K (and summed-batch) range is strided over the
// group and combined with a fixed xor-shuffle tree (deterministic).  Sizes here are <= 64 x 256 x 256
// outputs with K <= R*C, so the point is latency (enough waves), not FLOP/s.
template <int SG_SPLIT>   // 8: long K (weight compositions over K = C or R*C); 1: short K, many outputs
__global__ __launch_bounds__(256) void small_gemm_kernel(SmallGemm g) {
    const long per = (long)g.m * g.n;
    const int nb = g.sum_batch ? 1 : g.batch;
    const long total = per * nb;
    const int sub = threadIdx.x % SG_SPLIT;
    const long stride = (long)gridDim.x * blockDim.x / SG_SPLIT;
    long idx = ((long)blockIdx.x * blockDim.x + threadIdx.x) / SG_SPLIT;
    long wfirst = idx - (threadIdx.x % 64) / SG_SPLIT;           // wave-uniform loop bound (shuffles inside)
    for (; wfirst < total; wfirst += stride, idx += stride) {
        const bool valid = idx < total;
        float s = 0.f;
        int b = 0, i = 0, j = 0;
        if (valid) {
            b = (int)(idx / per);
            const long e = idx - (long)b * per;
            i = (int)(e / g.n);
            j = (int)(e % g.n);                                   // j fastest: coalesced when scj == 1 / sbj == 1
            const int b0 = g.sum_batch ? 0 : b, b1 = g.sum_batch ? g.batch : b + 1;
            for (int bb = b0; bb < b1; ++bb) {
                const float* A = g.A + (long)bb * g.sab + (long)i * g.sai;
                const float* B = g.B + (long)bb * g.sbb + (long)j * g.sbj;
                for (int k = sub; k < g.k; k += SG_SPLIT) s = fmaf(A[(long)k * g.sak], B[(long)k * g.sbk], s);
            }
        }
        if (SG_SPLIT == 8) {
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 4, 64);
        }
        if (valid && sub == 0) {
            float* c = g.C + (long)b * g.scb + (long)i * g.sci + (long)j * g.scj;
            *c = g.accumulate ? *c + s : s;
        }
    }
}

int launch_small_gemm(const SmallGemm& g, hipStream_t st) {
    REGT_CHECK_ARG(g.m > 0 && g.n > 0 && g.batch > 0, "small_gemm: empty problem");
    const long outputs = (long)g.m * g.n * (g.sum_batch ? 1 : g.batch);
    const long klen = (long)g.k * (g.sum_batch ? g.batch : 1);
    const bool split = klen >= 64;
    long total = outputs * (split ? 8 : 1);
    int blocks = cdiv(total, 256);
    if (blocks > 32768) blocks = 32768;
    if (split) hipLaunchKernelGGL(small_gemm_kernel<8>, dim3(blocks), dim3(256), 0, st, g);
    else hipLaunchKernelGGL(small_gemm_kernel<1>, dim3(blocks), dim3(256), 0, st, g);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

__global__ __launch_bounds__(256) void small_gemm_multi_kernel(SgBatch B) {
    int ti = 0;
    while (ti + 1 < B.ntask && (int)blockIdx.x >= B.block_start[ti + 1]) ++ti;
    // field-wise copy of the selected task (scalar selects; no dynamically indexed kernarg struct in scratch)
    const SgTask& T = B.task[ti];
    if (T.split == 0) {
        // Tiled form for the matrix-sized tasks (C x C, C x F outputs with K = F .. R C): one 32 x 32 output tile per workgroup,
        // 32-k chunks of both operands staged through LDS (each element is read from memory once per tile instead of once per
        // output element), a thread owns 2 x 2 outputs; sums run over (term, batch, k) in ascending order: deterministic.
        // Whichever of a tile's two indices is contiguous in memory is the one consecutive lanes walk.
        __shared__ float As[32][34], Bs[32][34];
        const int tiles_m = (T.m + 31) / 32, tiles_n = (T.n + 31) / 32;
        int w = blockIdx.x - B.block_start[ti];
        const int b = w / (tiles_m * tiles_n);
        w -= b * tiles_m * tiles_n;
        const int i0 = (w / tiles_n) * 32, j0 = (w % tiles_n) * 32;
        const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
        float c00 = 0.f, c01 = 0.f, c10 = 0.f, c11 = 0.f;
        for (int t = 0; t < T.nterm; ++t) {
            const SgTerm& q = T.term[t];
            const int b0 = q.sum_batch ? 0 : b, b1 = q.sum_batch ? q.batch : b + 1;
            const bool a_kfast = q.sak == 1, b_kfast = q.sbk == 1;
            for (int bb = b0; bb < b1; ++bb) {
                const float* A = q.A + (long)bb * q.sab;
                const float* Bp = q.B + (long)bb * q.sbb;
                for (int k0 = 0; k0 < q.k; k0 += 32) {
#pragma unroll
                    for (int e4 = 0; e4 < 4; ++e4) {
                        const int e = threadIdx.x + 256 * e4;
                        const int ia = a_kfast ? e >> 5 : e & 31, ka = a_kfast ? e & 31 : e >> 5;
                        As[ka][ia] = (i0 + ia < T.m && k0 + ka < q.k) ? A[(long)(i0 + ia) * q.sai + (long)(k0 + ka) * q.sak] : 0.f;
                        const int jb = b_kfast ? e >> 5 : e & 31, kb = b_kfast ? e & 31 : e >> 5;
                        Bs[kb][jb] = (j0 + jb < T.n && k0 + kb < q.k) ? Bp[(long)(k0 + kb) * q.sbk + (long)(j0 + jb) * q.sbj] : 0.f;
                    }
                    __syncthreads();
#pragma unroll 8
                    for (int k = 0; k < 32; ++k) {
                        const float a0 = As[k][2 * ty], a1 = As[k][2 * ty + 1], v0 = Bs[k][2 * tx], v1 = Bs[k][2 * tx + 1];
                        c00 = fmaf(a0, v0, c00); c01 = fmaf(a0, v1, c01);
                        c10 = fmaf(a1, v0, c10); c11 = fmaf(a1, v1, c11);
                    }
                    __syncthreads();
                }
            }
        }
        const float cc[2][2] = {{c00, c01}, {c10, c11}};
#pragma unroll
        for (int di = 0; di < 2; ++di)
#pragma unroll
            for (int dj = 0; dj < 2; ++dj) {
                const int i = i0 + 2 * ty + di, j = j0 + 2 * tx + dj;
                if (i < T.m && j < T.n) {
                    float v = cc[di][dj];
                    if (T.init) v += T.init[(long)i * T.init_si + (long)j * T.init_sj];
                    T.C[(long)b * T.scb + (long)i * T.sci + (long)j * T.scj] = v;
                }
            }
        return;
    }
    const long per = (long)T.m * T.n, total = per * T.nbatch;
    const int sp = T.split;                    // uniform per workgroup: a task starts on a workgroup boundary
    const int sub = sp == 8 ? (threadIdx.x & 7) : 0;
    const long idx = ((long)(blockIdx.x - B.block_start[ti]) * 256 + threadIdx.x) / sp;
    const bool valid = idx < total;
    float s = 0.f;
    int b = 0, i = 0, j = 0;
    if (valid) {
        b = (int)(idx / per);
        const long e = idx - (long)b * per;
        i = (int)(e / T.n);
        j = (int)(e % T.n);
        for (int t = 0; t < T.nterm; ++t) {
            const SgTerm& q = T.term[t];
            const int b0 = q.sum_batch ? 0 : b, b1 = q.sum_batch ? q.batch : b + 1;
            for (int bb = b0; bb < b1; ++bb) {
                const float* A = q.A + (long)bb * q.sab + (long)i * q.sai;
                const float* Bp = q.B + (long)bb * q.sbb + (long)j * q.sbj;
                for (int k = sub; k < q.k; k += sp) s = fmaf(A[(long)k * q.sak], Bp[(long)k * q.sbk], s);
            }
        }
    }
    if (sp == 8) {
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
    }
    if (valid && sub == 0) {
        if (T.init) s += T.init[(long)i * T.init_si + (long)j * T.init_sj];
        T.C[(long)b * T.scb + (long)i * T.sci + (long)j * T.scj] = s;
    }
}

int launch_small_gemm_multi(SgBatch& b, hipStream_t st) {
    REGT_CHECK_ARG(b.ntask > 0 && b.ntask <= SG_MAX_TASKS && !b.overflow, "small_gemm_multi: %d tasks%s", b.ntask,
                   b.overflow ? " (more than SG_MAX_TASKS were added)" : "");
    int blocks = 0;
    for (int t = 0; t < b.ntask; ++t) {
        b.block_start[t] = blocks;
        SgTask& task = b.task[t];
        const long outputs = (long)task.m * task.n * task.nbatch;
        REGT_CHECK_ARG(outputs > 0, "small_gemm_multi: empty task %d", t);
        long ksum = 0;                           // multiply-adds per output element
        for (int q = 0; q < task.nterm; ++q) ksum += (long)task.term[q].k * (task.term[q].sum_batch ? task.term[q].batch : 1);
        // eight lanes per output (strided k + xor tree) only pay off for long sums; a K = F product is one lane's work;
        // matrix-sized outputs take the tiled form (split = 0)
        // (sums longer than 256 over few tiles -- d cheb_w1 = sum over the owned regions, K = R C -- stay on the 8-lane form: 16
        // workgroups walking 64 chunks each were slower, 0.25 vs 0.15 ms for the launch)
        constexpr long tiled_maxk = 256;
        if (task.m >= 16 && task.n >= 16 && ksum >= 16 && ksum <= tiled_maxk) {
            task.split = 0;
            blocks += (int)((long)cdiv(task.m, 32) * cdiv(task.n, 32) * task.nbatch);
        } else {
            task.split = ksum > 32 ? 8 : 1;
            blocks += cdiv(outputs * task.split, 256);
        }
    }
    b.block_start[b.ntask] = blocks;
    hipLaunchKernelGGL(small_gemm_multi_kernel, dim3(blocks), dim3(256), 0, st, b);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace regt
