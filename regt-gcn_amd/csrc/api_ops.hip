// Validated wrappers of single ops: graph preparation, aggregation, packing, linear, weight gradient, GAT attention, losses.
#include "api_internal.h"

using namespace regt;

extern "C" {

size_t regt_graph_workspace_bytes(int64_t E, int32_t N) { return graph_workspace_bytes((long)E, N); }

int32_t regt_gcn_csr(const int64_t* ei, const float* w, int64_t E, int32_t N, int32_t* rowptr, int32_t* col, float* val,
                     int32_t* flags_dev, void* ws, size_t ws_bytes, regt_stream_t st) {
    REGT_CHECK_ARG((ei || E == 0) && rowptr && col && val && flags_dev && ws, "regt_gcn_csr: NULL pointer");
    return graph_gcn_csr(ei, w, (long)E, N, rowptr, col, val, flags_dev, ws, ws_bytes, (hipStream_t)st);
}

int32_t regt_gcn_dis(const int64_t* ei, const float* w, int64_t E, int32_t N, float* dis_out, int32_t* flags_dev, void* ws, size_t ws_bytes,
                     regt_stream_t st) {
    REGT_CHECK_ARG((ei || E == 0) && dis_out && flags_dev && ws, "regt_gcn_dis: NULL pointer");
    return graph_gcn_dis(ei, w, (long)E, N, dis_out, flags_dev, ws, ws_bytes, (hipStream_t)st);
}

int32_t regt_cheb_edge_weights(const int64_t* ei, const float* w, int64_t E, int32_t N, float* out, int32_t* flags_dev,
                               void* ws, size_t ws_bytes, regt_stream_t st) {
    REGT_CHECK_ARG((ei || E == 0) && (out || E == 0) && flags_dev && ws, "regt_cheb_edge_weights: NULL pointer");
    return graph_cheb_edge_weights(ei, w, (long)E, N, out, flags_dev, ws, ws_bytes, (hipStream_t)st);
}

int32_t regt_raw_csr(const int64_t* ei, const float* v, int64_t E, int32_t N, int32_t* rowptr, int32_t* col, float* val,
                     int32_t* flags_dev, void* ws, size_t ws_bytes, regt_stream_t st) {
    REGT_CHECK_ARG((ei || E == 0) && rowptr && col && val && flags_dev && ws, "regt_raw_csr: NULL pointer");
    return graph_raw_csr(ei, v, (long)E, N, rowptr, col, val, flags_dev, ws, ws_bytes, (hipStream_t)st);
}

int32_t regt_graph_fingerprint(const int64_t* ei, const float* w, int64_t E, uint64_t* out_dev, regt_stream_t st) {
    REGT_CHECK_ARG((ei || E == 0) && out_dev, "regt_graph_fingerprint: NULL pointer");
    return graph_fingerprint(ei, w, (long)E, reinterpret_cast<unsigned long long*>(out_dev), (hipStream_t)st);
}

int32_t regt_spmm_csr(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, float* Y, int32_t nrows,
                      int32_t nrows_x, int32_t width, regt_stream_t st) {
    REGT_CHECK_ARG(rowptr && col && val && X && Y, "regt_spmm_csr: NULL pointer");
    return launch_spmm_csr(rowptr, col, val, X, Y, nrows, nrows_x, width, 1, (hipStream_t)st);
}

int32_t regt_spmm_dual(const int32_t* rowptr, const int32_t* col, const float* val_a, const float* val_l, const float* X,
                       float* YA, float* YL, int32_t N, int32_t width, regt_stream_t st) {
    REGT_CHECK_ARG(rowptr && col && val_a && val_l && X && YA && YL, "regt_spmm_dual: NULL pointer");
    return launch_spmm_dual(rowptr, col, val_a, val_l, X, YA, YL, N, width, (hipStream_t)st);
}

int32_t regt_pack_x(const float* x, float* xp, int32_t N, int32_t F, int32_t T, regt_stream_t st) {
    REGT_CHECK_ARG(x && xp && N > 0 && F > 0 && T > 0, "regt_pack_x: bad argument");
    return launch_pack_x(x, xp, N, F, T, (hipStream_t)st);
}

int32_t regt_linear(const float* A, int64_t lda, int64_t M, int32_t K, const float* W, int64_t ldw, int32_t N,
                    const float* bias, int32_t act, float slope, float* out, int64_t ldo, regt_stream_t st) {
    REGT_CHECK_ARG(A && W && out && M > 0 && K > 0 && N > 0, "regt_linear: bad argument");
    REGT_CHECK_ARG(act >= 0 && act <= 4, "regt_linear: act must be 0 (none), 1 (leaky_relu), 2 (relu), 3 (sigmoid) or 4 (tanh)");
    EpiBiasAct e{out, ldo, bias, act, slope};
    return launch_gemm_bias_act(one_seg(make_seg(A, lda, W, nullptr, ldw, INT_MAX, K, true)), M, N, e, (hipStream_t)st);
}

static void wgrad_chunks(int64_t M, int* kchunk, int* nchunks) {
    long kc = ((M + 127) / 128 + 31) / 32 * 32;
    if (kc < 512) kc = 512;
    *kchunk = (int)kc;
    *nchunks = (int)((M + kc - 1) / kc);
}

size_t regt_wgrad_slab_floats(int64_t M, int32_t N, int32_t K, int32_t with_bias) {
    int kc, nc;
    wgrad_chunks(M, &kc, &nc);
    return (size_t)nc * ((size_t)N * K + (with_bias ? N : 0));
}

int32_t regt_wgrad(const float* dOut, int64_t ldd, const float* A, int64_t lda, int64_t M, int32_t N, int32_t K, float* dW,
                   int64_t ldw, float* dbias, float* slab, regt_stream_t st) {
    REGT_CHECK_ARG(dOut && A && dW && slab && M > 0 && N > 0 && K > 0, "regt_wgrad: bad argument");
    int kc, nc;
    wgrad_chunks(M, &kc, &nc);
    // the caller's slab is sized by regt_wgrad_slab_floats; the 64-float alignment slack of the queue is not needed here
    ReduceQueue rq(slab, ((long)nc * ((long)N * K + (dbias ? N : 0)) + 63) & ~63L, (hipStream_t)st);
    TRY(wgrad_full(rq, "wgrad", dOut, ldd, N, A, lda, K, 0, M, kc, nc, dW, ldw, dbias, (hipStream_t)st));
    return rq.flush();
}

int32_t regt_wgrad_slabs(const float* P, int64_t ldp, int32_t Nout, const float* Q, int64_t ldq, int32_t Nin, int64_t M, int32_t kchunk,
                         int32_t nchunks, int32_t colsum, float* slab, int32_t any_rows, const char** kernel, regt_stream_t st) {
    REGT_CHECK_ARG(P && Q && slab && M > 0 && Nout > 0 && Nin > 0 && kchunk > 0 && nchunks > 0, "regt_wgrad_slabs: bad argument");
    REGT_CHECK_ARG((long)kchunk * nchunks >= M && (long)kchunk * (nchunks - 1) < M, "regt_wgrad_slabs: the chunks must tile the M rows");
    WgradArgs a{P, ldp, Nout, Q, ldq, Nin, 0, M, kchunk, nullptr, nchunks, slab, colsum ? 1 : 0};
    WgradKernel ran = WG_GENERIC32;
    TRY(launch_wgrad_slabs(a, (hipStream_t)st, any_rows != 0, &ran));
    if (kernel) *kernel = wgrad_kernel_name(ran);
    return REGT_OK;
}

int32_t regt_pack_x_bf16(const float* x, void* xp, int32_t N, int32_t F, int32_t T, regt_stream_t st) {
    REGT_CHECK_ARG(x && xp && N > 0 && F > 0 && T > 0, "regt_pack_x_bf16: bad argument");
    return launch_pack_x_bf16(x, xp, N, F, T, (hipStream_t)st);
}

int32_t regt_spmm_dual_bf16(const int32_t* rowptr, const int32_t* col, const float* val_a, const float* val_l, const void* X,
                            void* YA, void* YL, int32_t N, int32_t x_rows, int32_t width, regt_stream_t st) {
    REGT_CHECK_ARG(rowptr && col && val_a && val_l && X && YA && YL && x_rows >= N, "regt_spmm_dual_bf16: NULL pointer / x_rows < N");
    return launch_spmm_dual_bf16(rowptr, col, val_a, val_l, X, YA, YL, N, x_rows, width, (hipStream_t)st);
}

int32_t regt_gat_forward(const int32_t* rowptr, const int32_t* col, const float* x, const float* u_src, const float* u_dst, float slope,
                         int32_t N, int32_t T, int32_t F, float* out, float* stats, regt_stream_t st) {
    REGT_CHECK_ARG(rowptr && col && x && u_src && u_dst && out && stats, "regt_gat_forward: NULL pointer");
    REGT_CHECK_ARG(al16(x) && al16(u_src) && al16(u_dst) && al16(out) && al16(stats), "regt_gat_forward: pointers must be 16-byte aligned");
    return launch_gat_forward(rowptr, col, x, u_src, u_dst, slope, N, T, F, out, stats, (hipStream_t)st);
}

int32_t regt_gat_backward(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col, const float* x,
                          const float* u_src, float slope, int32_t N, int32_t T, int32_t F, const float* dout, float* stats, float* dsd,
                          regt_stream_t st) {
    REGT_CHECK_ARG(rowptr && col && t_rowptr && t_col && x && u_src && dout && stats && dsd, "regt_gat_backward: NULL pointer");
    REGT_CHECK_ARG(al16(x) && al16(u_src) && al16(dout) && al16(stats), "regt_gat_backward: pointers must be 16-byte aligned");
    return launch_gat_backward(rowptr, col, t_rowptr, t_col, x, u_src, slope, N, T, F, dout, stats, dsd, (hipStream_t)st);
}

int32_t regt_mean_csr(const int64_t* ei, int64_t E, int32_t N, int32_t* rowptr, int32_t* col, float* val, int32_t* flags_dev, void* ws,
                      size_t ws_bytes, regt_stream_t st) {
    REGT_CHECK_ARG((ei || E == 0) && rowptr && col && val && flags_dev && ws, "regt_mean_csr: NULL pointer");
    return graph_mean_csr(ei, (long)E, N, rowptr, col, val, flags_dev, ws, ws_bytes, (hipStream_t)st);
}

int32_t regt_relu_backward(const float* y, float* d, int64_t n, regt_stream_t st) {
    REGT_CHECK_ARG(y && d, "regt_relu_backward: y or d is NULL");
    REGT_CHECK_ARG(n >= 1 && n < (1L << 31), "regt_relu_backward: n must be in [1, 2^31), got %ld", (long)n);   // one thread each
    return regt::launch_relu_mask(y, d, (long)n, (hipStream_t)st);
}

int32_t regt_mse_loss_grad(const float* pred, const float* y, float* dpred, float* loss_out, int64_t count,
                           int64_t global_count, regt_stream_t st) {
    REGT_CHECK_ARG(pred && y && count > 0 && global_count > 0, "regt_mse_loss_grad: bad argument");
    return launch_mse_grad(pred, y, dpred, loss_out, (long)count, 1.0f / (float)global_count, (hipStream_t)st);
}

}  // extern "C"
