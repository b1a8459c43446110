// Attention-weighted window sum over a ring of per-time-step cell outputs:
//   hidden[w, n, c] = sum_{p < T} prob[p] * ring[(first_slot + w + p) % ring_len, n, c]        w < windows
// The cell of RegionalA3TGCN / A3TGCN is called with H = None in every period, so its output for a raw time step does not depend on
// the window the step is read through: consecutive stride-1 windows share T - 1 of their T slabs, and this kernel is all that is left
// of the attention sum once the slabs are cached.  Memory-bound: one fused multiply-add per loaded float.
//
// Mapping.  A slab is N * C / 4 float4 pieces (the (n, c) plane flattened: no node tile, no column tile, one ragged tail).  A thread
// owns one piece and a chunk of WC consecutive windows, WC accumulators in registers; blockIdx.y is the chunk.  It walks the chunk's
// nw + T - 1 slots ONCE, U loads in flight, and every loaded value feeds the windows that contain its slot: slot j of the chunk is
// period p = j - w of window w.  Slots ascend, so every accumulator receives its periods p = 0, 1, .., T - 1 in that order, one fmaf
// each, starting from 0 -- the same bits whatever `windows`, `first_slot`, `ring_len` or chunk a window is computed in.  WC = 1 is
// the serving form (T slab reads, one write), WC = WINDOW_WC the evaluation form ((WC + T - 1) / WC slab reads per window).
#include <algorithm>

#include "kernels.h"

namespace regt {

constexpr int WINDOW_LOADS = 4;      // 16-byte loads a thread issues before it consumes the first

template <int WC>
__global__ __launch_bounds__(256) void window_sum_kernel(const float4* __restrict__ ring, const float* __restrict__ probs,
                                                         float4* __restrict__ hidden, long slab4, int ring_len, int first_slot,
                                                         int windows, int T) {
    const int w0 = blockIdx.y * WC;
    const int nw = windows - w0 < WC ? windows - w0 : WC;
    const int nslots = nw + T - 1;                       // <= ring_len (checked on the host): no slot is met twice
    int s0 = first_slot + w0;                            // < 2 ring_len
    if (s0 >= ring_len) s0 -= ring_len;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < slab4; e += gridDim.x * 256L) {
        float4 acc[WC];
#pragma unroll
        for (int w = 0; w < WC; ++w) acc[w] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j0 = 0; j0 < nslots; j0 += WINDOW_LOADS) {
            float4 v[WINDOW_LOADS];
#pragma unroll
            for (int u = 0; u < WINDOW_LOADS; ++u) {
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (j0 + u < nslots) {                   // slots past the chunk's last one are never read
                    int s = s0 + j0 + u;
                    if (s >= ring_len) s -= ring_len;
                    v[u] = ring[s * slab4 + e];
                }
            }
#pragma unroll
            for (int u = 0; u < WINDOW_LOADS; ++u) {
                const int j = j0 + u;
                if (j < nslots) {
#pragma unroll
                    for (int w = 0; w < WC; ++w) {
                        const int p = j - w;             // wave-uniform, as are j and w
                        if (w < nw && (unsigned)p < (unsigned)T) {
                            const float pr = probs[p];
                            acc[w].x = fmaf(pr, v[u].x, acc[w].x);
                            acc[w].y = fmaf(pr, v[u].y, acc[w].y);
                            acc[w].z = fmaf(pr, v[u].z, acc[w].z);
                            acc[w].w = fmaf(pr, v[u].w, acc[w].w);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int w = 0; w < WC; ++w)
            if (w < nw) hidden[(long)(w0 + w) * slab4 + e] = acc[w];
    }
}

int window_chunk(int windows) { return windows == 1 ? 1 : WINDOW_WC; }

// ring (ring_len, N, C), probs (T) = softmax of the attention logits, hidden (windows, N, C); the caller has checked the arguments
// (api_model.hip: C % 4 == 0, 1 <= T <= min(255, ring_len), 0 <= first_slot < ring_len, windows + T - 1 <= ring_len or windows == 1).
int launch_window_sum(const float* ring, const float* probs, float* hidden, int ring_len, int first_slot, int windows, int N, int T,
                      int C, hipStream_t st) {
    const long slab4 = (long)N * C / 4;
    const int wc = window_chunk(windows);
    const int chunks = cdiv(windows, wc);
    REGT_CHECK_ARG(chunks <= WINDOW_MAX_CHUNKS, "window sum: %d windows exceed the %d a launch covers", windows, WINDOW_MAX_CHUNKS * WINDOW_WC);
    // a memory-bound grid: enough workgroups to fill the chip a few times over, the rest by the grid stride
    const long want = (slab4 + 255) / 256, cap = std::max(1L, 8L * device_cus() / chunks);
    const dim3 grid((unsigned)std::min(want, cap), (unsigned)chunks);
    const float4* r4 = reinterpret_cast<const float4*>(ring);
    float4* h4 = reinterpret_cast<float4*>(hidden);
    if (wc == 1) hipLaunchKernelGGL(window_sum_kernel<1>, grid, dim3(256), 0, st, r4, probs, h4, slab4, ring_len, first_slot, windows, T);
    else hipLaunchKernelGGL(window_sum_kernel<WINDOW_WC>, grid, dim3(256), 0, st, r4, probs, h4, slab4, ring_len, first_slot, windows, T);
    REGT_CHECK_LAUNCH();
    return REGT_OK;
}

}  // namespace regt
