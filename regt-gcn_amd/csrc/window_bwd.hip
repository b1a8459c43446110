// Backward of the attention-weighted window sum over a ring of per-time-step cell outputs (window.hip):
//   hidden[w]  = sum_{p < T} prob[p] * ring[slot(w + p)]                      slot(j) = (first_slot + j) % ring_len, w < windows
//   dring[slot(j)] (+)= sum_{w : 0 <= j - w < T} prob[j - w] * dhidden[w]       j < windows + T - 1      (window_adjoint_kernel)
//   dprob[p]   = sum_{w, n, c} dhidden[w, n, c] * ring[slot(w + p), n, c]                                (window_attgrad_kernel)
//   dlogit     = prob * (dprob - sum_q prob[q] dprob[q])                                                 (window_att_final_kernel)
// Both passes are memory-bound mirrors of window_sum_kernel: a thread owns one 16-byte piece of the flattened (n, c) plane and a chunk of
// WC consecutive slots (adjoint) or windows (attention gradient), blockIdx.y is the chunk.  Vector stores only, no float atomics.
//
// Order of the adjoint.  A slot's accumulator starts from the value dring holds (accumulate) or from 0 and receives its windows in
// ASCENDING window order, one fmaf(prob[j - w], dhidden[w], acc) each.  So a step's dS is the same bits whether its windows arrive in one
// call or split over consecutive accumulating calls in ascending order, whatever chunk the slot falls in and whatever first_slot /
// ring_len are: a batch of windows hands its partial sums to the next one through dring.
//
// Order of the attention gradient.  Per thread: its pieces e ascending (grid stride), per piece the chunk's slots ascending and per slot
// the windows ascending, one fmaf per float into the period's accumulator.  The period index p = j - w is a compile-time constant of
// the fully unrolled slot walk, so the T <= WINDOW_BWD_MAX_T accumulators stay in registers (a per-thread dp[T] indexed by a runtime p
// would live in scratch).  Then a butterfly over the wave, the four waves of a workgroup in wave order, one partial row per workgroup,
// and one launch that adds the rows in a fixed order: the result depends on the call's arguments and the device's CU count only.
#include <algorithm>

#include "kernels.h"

namespace regt {

constexpr int WINDOW_BWD_LOADS = 4;      // 16-byte loads a thread issues before it consumes the first

template <int WC>
__global__ __launch_bounds__(256) void window_adjoint_kernel(const float4* __restrict__ dhidden, const float* __restrict__ probs,
                                                             float4* __restrict__ dring, long slab4, int ring_len, int first_slot,
                                                             int windows, int T, int accumulate) {
    const int covered = windows + T - 1;                 // <= ring_len (checked on the host): no slot is met twice
    const int j0 = blockIdx.y * WC;                      // the chunk's first slot, counted from first_slot
    const int ns = covered - j0 < WC ? covered - j0 : WC;
    const int wlo = j0 - (T - 1) > 0 ? j0 - (T - 1) : 0;                       // the windows that contain one of the chunk's slots:
    const int whi = j0 + ns - 1 < windows - 1 ? j0 + ns - 1 : windows - 1;     // wlo .. whi, at most ns + T - 1 of them
    const int nwin = whi - wlo + 1;
    int s0 = first_slot + j0;                            // < 2 ring_len
    if (s0 >= ring_len) s0 -= ring_len;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < slab4; e += gridDim.x * 256L) {
        float4 acc[WC];
#pragma unroll
        for (int i = 0; i < WC; ++i) {
            acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (accumulate && i < ns) {
                int s = s0 + i;
                if (s >= ring_len) s -= ring_len;
                acc[i] = dring[s * slab4 + e];
            }
        }
        for (int k0 = 0; k0 < nwin; k0 += WINDOW_BWD_LOADS) {
            float4 v[WINDOW_BWD_LOADS];
#pragma unroll
            for (int u = 0; u < WINDOW_BWD_LOADS; ++u) {
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k0 + u < nwin) v[u] = dhidden[(long)(wlo + k0 + u) * slab4 + e];      // windows past the chunk's last one are never read
            }
#pragma unroll
            for (int u = 0; u < WINDOW_BWD_LOADS; ++u) {
                if (k0 + u < nwin) {
                    const int w = wlo + k0 + u;
#pragma unroll
                    for (int i = 0; i < WC; ++i) {
                        const int p = j0 + i - w;        // wave-uniform, as are w and i
                        if (i < ns && (unsigned)p < (unsigned)T) {
                            const float pr = probs[p];
                            acc[i].x = fmaf(pr, v[u].x, acc[i].x);
                            acc[i].y = fmaf(pr, v[u].y, acc[i].y);
                            acc[i].z = fmaf(pr, v[u].z, acc[i].z);
                            acc[i].w = fmaf(pr, v[u].w, acc[i].w);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < WC; ++i) {
            if (i < ns) {
                int s = s0 + i;
                if (s >= ring_len) s -= ring_len;
                dring[s * slab4 + e] = acc[i];
            }
        }
    }
}

template <int WC>
__global__ __launch_bounds__(256) void window_attgrad_kernel(const float4* __restrict__ ring, const float4* __restrict__ dhidden,
                                                             float* __restrict__ partial, long slab4, int ring_len, int first_slot,
                                                             int windows, int T) {
    constexpr int TB = WINDOW_BWD_MAX_T;
    constexpr int WALK = WC + TB - 1;                    // slots of a full chunk at the largest T
    const int w0 = blockIdx.y * WC;
    const int nw = windows - w0 < WC ? windows - w0 : WC;
    const int nslots = nw + T - 1;
    int s0 = first_slot + w0;
    if (s0 >= ring_len) s0 -= ring_len;
    float dp[TB];
#pragma unroll
    for (int p = 0; p < TB; ++p) dp[p] = 0.f;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < slab4; e += gridDim.x * 256L) {
        float4 dh[WC];
#pragma unroll
        for (int w = 0; w < WC; ++w) {
            dh[w] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (w < nw) dh[w] = dhidden[(long)(w0 + w) * slab4 + e];
        }
        int s = s0;                                      // the walk's slot and its slab, stepped: no table of slot offsets in SGPRs
        const float4* slab = ring + s0 * slab4 + e;
#pragma unroll
        for (int jb = 0; jb < WALK; jb += WINDOW_BWD_LOADS) {
            if (jb < nslots) {                           // wave-uniform: the groups past the chunk's last slot are skipped
                float4 v[WINDOW_BWD_LOADS];
#pragma unroll
                for (int u = 0; u < WINDOW_BWD_LOADS; ++u) {
                    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (jb + u < nslots) {               // slots past the chunk's last one are never read
                        v[u] = *slab;
                        slab += slab4;
                        if (++s == ring_len) { s = 0; slab = ring + e; }
                    }
                }
#pragma unroll
                for (int u = 0; u < WINDOW_BWD_LOADS; ++u) {
#pragma unroll
                    for (int w = 0; w < WC; ++w) {
                        const int p = jb + u - w;        // a constant once the walk is unrolled: dp[p] is a register
                        if (p >= 0 && p < TB) {
                            if (jb + u < nslots && w < nw && p < T) {
                                dp[p] = fmaf(dh[w].x, v[u].x, dp[p]);
                                dp[p] = fmaf(dh[w].y, v[u].y, dp[p]);
                                dp[p] = fmaf(dh[w].z, v[u].z, dp[p]);
                                dp[p] = fmaf(dh[w].w, v[u].w, dp[p]);
                            }
                        }
                    }
                }
            }
        }
    }
    // wave butterfly, then the four waves in wave order: one partial row per workgroup
    __shared__ float red[4][TB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int p = 0; p < TB; ++p) {
        if (p < T) {
            float s = dp[p];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            if (lane == 0) red[wave][p] = s;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < T) {
        const int p = threadIdx.x;
        const long row = (long)blockIdx.y * gridDim.x + blockIdx.x;
        partial[row * T + p] = (red[0][p] + red[1][p]) + (red[2][p] + red[3][p]);
    }
}

// dprob[p] = fixed-order sum of the workgroups' partial rows; dlogit = prob (dprob - sum_q prob[q] dprob[q]), added to d_attention or written
__global__ __launch_bounds__(256) void window_att_final_kernel(const float* __restrict__ partial, long nrows, const float* __restrict__ probs,
                                                               float* __restrict__ d_attention, int T, int accumulate) {
    __shared__ float red[256];
    __shared__ float dp[WINDOW_BWD_MAX_T];
    for (int t = 0; t < T; ++t) {
        float s = 0.f;
        for (long b = threadIdx.x; b < nrows; b += 256) s += partial[b * T + t];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) dp[t] = red[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float mean = 0.f;
        for (int t = 0; t < T; ++t) mean += probs[t] * dp[t];
        for (int t = 0; t < T; ++t) {
            const float g = probs[t] * (dp[t] - mean);
            d_attention[t] = accumulate ? d_attention[t] + g : g;
        }
    }
}

__global__ __launch_bounds__(256) void deliver_kernel(DeliverArgs a) {
    const int k = blockIdx.y;
    const float* __restrict__ src = a.src[k];
    float* __restrict__ dst = a.dst[k];
    for (long i = blockIdx.x * 256L + threadIdx.x; i < a.n[k]; i += gridDim.x * 256L) dst[i] = a.accumulate ? dst[i] + src[i] : src[i];
}

// a memory-bound grid: enough workgroups to fill the chip a few times over, the rest by the grid stride (window.hip's rule)
static unsigned window_grid_x(long slab4, int chunks) {
    const long want = (slab4 + 255) / 256, cap = std::max(1L, 8L * device_cus() / chunks);
    return (unsigned)std::min(want, cap);
}

// dhidden (windows, N, C), probs (T), dring (ring_len, N, C); the caller has checked the arguments (api_model.hip: regt_window_forward's
// list and T <= WINDOW_BWD_MAX_T, windows + T - 1 <= ring_len)
int launch_window_adjoint(const float* dhidden, const float* probs, float* dring, int ring_len, int first_slot, int windows, int N, int T,
                          int C, int accumulate, hipStream_t st) {
    const long slab4 = (long)N * C / 4;
    const int wc = window_chunk(windows);
    const int chunks = cdiv((long)windows + T - 1, wc);
    REGT_CHECK_ARG(chunks <= WINDOW_MAX_CHUNKS, "window adjoint: %d slots exceed the %d a launch covers", windows + T - 1, WINDOW_MAX_CHUNKS * wc);
    const dim3 grid(window_grid_x(slab4, chunks), (unsigned)chunks);
    const float4* d4 = reinterpret_cast<const float4*>(dhidden);
    float4* r4 = reinterpret_cast<float4*>(dring);
    if (wc == 1) hipLaunchKernelGGL(window_adjoint_kernel<1>, grid, dim3(256), 0, st, d4, probs, r4, slab4, ring_len, first_slot, windows, T, accumulate);
    else hipLaunchKernelGGL(window_adjoint_kernel<WINDOW_WC>, grid, dim3(256), 0, st, d4, probs, r4, slab4, ring_len, first_slot, windows, T, accumulate);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

// rows of T floats the attention gradient's first pass writes: one per workgroup
long window_attgrad_blocks(int windows, int N, int C) {
    const int chunks = cdiv(windows, window_chunk(windows));
    return (long)window_grid_x((long)N * C / 4, chunks) * chunks;
}

int launch_window_attgrad(const float* ring, const float* dhidden, const float* probs, float* partial, float* d_attention, int ring_len,
                          int first_slot, int windows, int N, int T, int C, int accumulate, hipStream_t st) {
    REGT_CHECK_ARG(T <= WINDOW_BWD_MAX_T, "window attention gradient: T=%d exceeds %d", T, WINDOW_BWD_MAX_T);
    const long slab4 = (long)N * C / 4;
    const int wc = window_chunk(windows);
    const int chunks = cdiv(windows, wc);
    REGT_CHECK_ARG(chunks <= WINDOW_MAX_CHUNKS, "window attention gradient: %d windows exceed the %d a launch covers", windows, WINDOW_MAX_CHUNKS * wc);
    const dim3 grid(window_grid_x(slab4, chunks), (unsigned)chunks);
    const float4* r4 = reinterpret_cast<const float4*>(ring);
    const float4* d4 = reinterpret_cast<const float4*>(dhidden);
    if (wc == 1) hipLaunchKernelGGL(window_attgrad_kernel<1>, grid, dim3(256), 0, st, r4, d4, partial, slab4, ring_len, first_slot, windows, T);
    else hipLaunchKernelGGL(window_attgrad_kernel<WINDOW_WC>, grid, dim3(256), 0, st, r4, d4, partial, slab4, ring_len, first_slot, windows, T);
    REGT_CHECK_LAUNCH();
    hipLaunchKernelGGL(window_att_final_kernel, dim3(1), dim3(256), 0, st, partial, (long)grid.x * grid.y, probs, d_attention, T, accumulate);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

int launch_deliver(const DeliverArgs& a, hipStream_t st) {
    REGT_CHECK_ARG(a.count >= 1 && a.count <= 4, "deliver: %d vectors", a.count);
    long most = 1;
    for (int k = 0; k < a.count; ++k) most = std::max(most, a.n[k]);
    const dim3 grid((unsigned)std::min<long>((most + 255) / 256, 1024), (unsigned)a.count);
    hipLaunchKernelGGL(deliver_kernel, grid, dim3(256), 0, st, a);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace regt
