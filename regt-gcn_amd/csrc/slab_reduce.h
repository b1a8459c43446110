// The baselines' weight gradients end alike: every workgroup (or wave, or row chunk) leaves one row of partial sums in a slab of
// (nrows, width) floats, the rows are summed column by column in a FIXED order -- no float atomics, two runs give the same bits --
// and the sums are scattered to the gradient tensors.  Stated once here; DESIGN.md 3l lists who runs which order.
//   slab_reduce_chunks<CHUNK>   part[c] = rows [CHUNK c, CHUNK c + CHUNK) in row order from +0      (spatial.hip, stnorm.hip)
//   slab_reduce_final<SEED>     the rows in row order, from +0 or from row 0, then the scatter      (all four; stid.hip's own
//                               kernel calls slab_col_sum / slab_scatter and sums dnode in the same launch)
//   slab_reduce_tree<THREADS>   THREADS interleaved running sums, then a pairwise tree, then the scatter   (staeformer_*.hip)
#pragma once
#include "kernels.h"

namespace regt {

// segment k of the summed row, columns [end[k - 1], end[k]) (end[-1] = 0), goes to dst[k]; an empty segment's dst is never touched
struct SlabSegs {
    static constexpr int MAX = 3 + 4 * STID_MAX_LAYERS + 2;      // STID's parameter table, the longest
    int n;
    long end[MAX];
    float* dst[MAX];
};

inline void add_seg(SlabSegs& sg, float* dst, long count) {
    sg.dst[sg.n] = dst;
    sg.end[sg.n] = (sg.n ? sg.end[sg.n - 1] : 0) + count;
    ++sg.n;
}

// column e < end[n - 1] of the summed row -> its segment
__device__ __forceinline__ void slab_scatter(const SlabSegs& sg, long e, float v) {
    int s = 0;
    long start = 0;
    while (s < sg.n - 1 && e >= sg.end[s]) start = sg.end[s++];
    sg.dst[s][e - start] = v;
}

// Column e of the rows in row order.  The seed is part of the order: from +0 an all-(-0) column sums to +0, from row 0 to -0.
template <bool SEED_ROW0>
__device__ __forceinline__ float slab_col_sum(const float* __restrict__ slab, int nrows, long width, long e) {
    float v = SEED_ROW0 ? slab[e] : 0.f;
    for (int r = SEED_ROW0 ? 1 : 0; r < nrows; ++r) v += slab[(long)r * width + e];
    return v;
}

// Stage 1 (grid: columns / 256 x chunks): all loads of the chunk are issued first, then the adds in row order.  The running sum
// starts at +0 and so is never -0: the +0 a ragged last chunk is padded with changes no bit.
template <int CHUNK>
__global__ __launch_bounds__(256) void slab_reduce_chunks(const float* __restrict__ slab, int nrows, long width, float* __restrict__ part) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= width) return;
    const int r0 = blockIdx.y * CHUNK, r1 = min(r0 + CHUNK, nrows);
    float v[CHUNK];
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) v[k] = r0 + k < r1 ? slab[(long)(r0 + k) * width + e] : 0.f;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) s += v[k];
    part[(long)blockIdx.y * width + e] = s;
}

template <bool SEED_ROW0>
__global__ __launch_bounds__(256) void slab_reduce_final(const float* __restrict__ slab, int nrows, long width, const SlabSegs sg) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < width) slab_scatter(sg, e, slab_col_sum<SEED_ROW0>(slab, nrows, width, e));
}

// One workgroup per column: thread t adds rows t, t + THREADS, ... in order, then a pairwise tree.  For row counts in the tens of
// thousands, where one running sum loses the bits a cancelling column needs.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void slab_reduce_tree(const float* __restrict__ slab, long nrows, long width, const SlabSegs sg) {
    __shared__ float sm[THREADS];
    const long c = blockIdx.x;
    float s = 0.f;
    for (long r = threadIdx.x; r < nrows; r += THREADS) s += slab[r * width + c];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int half = THREADS / 2; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half) sm[threadIdx.x] += sm[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) slab_scatter(sg, c, sm[0]);
}

template <bool SEED_ROW0>
int launch_slab_reduce_final(const float* slab, int nrows, long width, const SlabSegs& sg, hipStream_t st) {
    hipLaunchKernelGGL(slab_reduce_final<SEED_ROW0>, dim3(cdiv(width, 256)), dim3(256), 0, st, slab, nrows, width, sg);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

// the two stages: part holds cdiv(nrows, CHUNK) rows
template <int CHUNK>
int launch_slab_reduce_chunked(const float* slab, int nrows, long width, float* part, const SlabSegs& sg, hipStream_t st) {
    const int nchunks = cdiv(nrows, CHUNK);
    hipLaunchKernelGGL(slab_reduce_chunks<CHUNK>, dim3(cdiv(width, 256), nchunks), dim3(256), 0, st, slab, nrows, width, part);
    REGT_CHECK_LAUNCH();
    return launch_slab_reduce_final<false>(part, nchunks, width, sg, st);
}

}  // namespace regt
