/* regtgcn.h -- C ABI of libregtgcn_hip.so, the MI355X (gfx950) implementation of the RegT-GCN
 * forward/backward hot path.
 *
 * The reference (raynbowy23/RegT-GCN) is pure Python: its hot path has no FFI of its own, it
 * reaches the device through torch / torch_geometric operator calls.  The entry points below are
 * therefore the op sites of that path, one C function per site, so that a reference maintainer can
 * bind them with ctypes (INTEGRATION.md shows the stub).  Citations are relative to the reference
 * root.  All pointers are DEVICE pointers unless the name ends in `_host`; all matrices are
 * row-major fp32; indices are int64 on input (the reference's edge_index dtype) and int32 inside
 * prepared operators.  Every function enqueues on `stream` (a hipStream_t passed as void*), never
 * synchronises, allocates nothing, and returns 0 on success or a non-zero code with a message
 * available from regt_last_error().  Buffers are owned by the caller for the duration of the
 * enqueued work.
 */
#ifndef REGTGCN_H
#define REGTGCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* regt_stream_t;

#define REGT_ABI_VERSION 8

int32_t regt_abi_version(void);
/* Message of the last failing call on this thread ("" if none). */
const char* regt_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Graph preparation (once per static graph).
 *
 * Replaces the normalisation PyG recomputes inside every conv call because the reference builds
 * its layers with cached=False (models/RegionalTemporalGCN.py:54,73):
 *   GCNConv  gcn_norm          -- call sites models/utils.py:169,175,181
 *   ChebConv __norm__/get_laplacian -- call sites models/RegionalTemporalGCN.py:136-140,
 *                                      models/TemporalGCN.py:88
 * edge_index is the reference's (2,E) int64 tensor (row 0 = source, row 1 = target), edge_weight
 * its (E,) fp32 edge_attr or NULL for unit weights.
 * flags_dev[0] receives bit0 = an index was out of [0,N), bit1 = a negative weight was seen.
 * ---------------------------------------------------------------------------------------------- */
size_t regt_graph_workspace_bytes(int64_t num_edges, int32_t num_nodes);

/* A_hat = D^-1/2 (A + I) D^-1/2 as a destination-sorted CSR; rowptr (N+1), col/val (E + N). */
int32_t regt_gcn_csr(const int64_t* edge_index, const float* edge_weight, int64_t num_edges, int32_t num_nodes,
                     int32_t* rowptr, int32_t* col, float* val, int32_t* flags_dev,
                     void* workspace, size_t workspace_bytes, regt_stream_t stream);

/* D^-1/2 of that normalisation alone: dis_out (N) = (in-degree sum in edge order + self loop)^-1/2, 0 where the degree is 0 --
 * the value regt_gcn_csr multiplies into every entry.  A region shard computes it for its own nodes and publishes it (one
 * all-reduce at graph preparation) so that the ranks that read those nodes as halo sources can finish their rows of A_hat
 * without normalising the global graph. */
int32_t regt_gcn_dis(const int64_t* edge_index, const float* edge_weight, int64_t num_edges, int32_t num_nodes, float* dis_out,
                     int32_t* flags_dev, void* workspace, size_t workspace_bytes, regt_stream_t stream);

/* Per-edge scaled-Laplacian weights of ChebConv(K=2, 'sym', lambda_max=None): out_weight (E). */
int32_t regt_cheb_edge_weights(const int64_t* edge_index, const float* edge_weight, int64_t num_edges,
                               int32_t num_nodes, float* out_weight, int32_t* flags_dev,
                               void* workspace, size_t workspace_bytes, regt_stream_t stream);

/* Destination-sorted CSR of given per-edge values (self loops dropped); rowptr (N+1), col/val (E). */
int32_t regt_raw_csr(const int64_t* edge_index, const float* edge_value, int64_t num_edges, int32_t num_nodes,
                     int32_t* rowptr, int32_t* col, float* val, int32_t* flags_dev,
                     void* workspace, size_t workspace_bytes, regt_stream_t stream);

/* Mean-aggregation operator of SAGEConv(aggr='mean') (base block 'graphsage' of the TGCN cell, models/utils.py:99-100): row i
 * holds every listed in-edge j -> i (self loops and duplicate edges as listed) with weight 1 / in-degree(i); rowptr (N+1),
 * col/val (E).  Nodes without in-edges get an empty row (their mean is 0, as in PyG). */
int32_t regt_mean_csr(const int64_t* edge_index, int64_t num_edges, int32_t num_nodes, int32_t* rowptr, int32_t* col,
                      float* val, int32_t* flags_dev, void* workspace, size_t workspace_bytes, regt_stream_t stream);

/* Order-independent 64-bit fingerprint of (edge_index, edge_weight) -- cache key for prepared graphs. */
int32_t regt_graph_fingerprint(const int64_t* edge_index, const float* edge_weight, int64_t num_edges,
                               uint64_t* out_dev, regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Sparse aggregation -- MessagePassing.propagate (gather x[row], scale, scatter-add at col) of both
 * conv types, as a pull over the prepared CSR:  Y[r,:] = sum_e val[e] * X[col[e],:].
 * X has nrows_x rows, Y nrows rows, both `width` fp32 wide (multiple of 4), 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int32_t regt_spmm_csr(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, float* Y,
                      int32_t nrows, int32_t nrows_x, int32_t width, regt_stream_t stream);

/* Both operators in one pass over a merged CSR (two weights per entry): YA = A x, YL = L x; width % 4 == 0 (widths that are no
 * multiple of 32 floats -- e.g. the reference's T * F = 48 -- take a whole-row kernel and must not exceed 2048). */
int32_t regt_spmm_dual(const int32_t* rowptr, const int32_t* col, const float* val_a, const float* val_l, const float* X,
                       float* YA, float* YL, int32_t num_nodes, int32_t width, regt_stream_t stream);

/* The same with bf16 rows in and out (REGT_GEMM_MODE=bf16: x, A_hat x and L~ x only ever feed bf16 matrix-core operands
 * there): X is (x_rows >= N) x width bf16 -- own rows first, then the halo rows of a region shard --, YA / YL are N x width
 * bf16; fp32 accumulation in CSR order, one rounding (to nearest even) per output element; width % 64 == 0. */
int32_t regt_spmm_dual_bf16(const int32_t* rowptr, const int32_t* col, const float* val_a, const float* val_l, const void* X,
                            void* YA, void* YL, int32_t num_nodes, int32_t x_rows, int32_t width, regt_stream_t stream);

/* Snapshot layout change (N,F,T) time-innermost (load_dataset.py:451-457) -> (N,T,F) rows. */
int32_t regt_pack_x(const float* x, float* x_packed, int32_t num_nodes, int32_t num_features, int32_t periods,
                    regt_stream_t stream);

/* ... rounding the snapshot to bf16 (nearest even) on the way: x_packed is (N, T, F) bf16, F % 8 == 0. */
int32_t regt_pack_x_bf16(const float* x, void* x_packed, int32_t num_nodes, int32_t num_features, int32_t periods,
                         regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Dense contraction -- torch.nn.Linear / PyG Linear call sites:
 *   out[M,N] = act(A[M,K] W[N,K]^T + bias)     act: 0 none, 1 leaky_relu(slope), 2 relu
 *                                              (3 sigmoid, 4 tanh: gate epilogues of the zero-hidden cell)
 * and the matching weight gradient  dW[N,K] = dOut[M,N]^T A[M,K]  (+ optional dbias = column sums).
 * regt_wgrad needs `slab` of regt_wgrad_slab_floats(...) floats.
 * Operands (pinned by tests/test_gpu_windows.py): any leading dimension >= the logical width and any 4-byte aligned pointer
 * (16-byte aligned rows only select the vector kernels); bias / dbias may be NULL.  Nothing outside the M x K, N x K and M x N
 * windows (and the N bias words, the slab) is read into a result or written; what dW, dbias and `slab` hold on entry is irrelevant.
 * ---------------------------------------------------------------------------------------------- */
int32_t regt_linear(const float* A, int64_t lda, int64_t M, int32_t K, const float* W, int64_t ldw, int32_t N,
                    const float* bias, int32_t act, float slope, float* out, int64_t ldo, regt_stream_t stream);
size_t regt_wgrad_slab_floats(int64_t M, int32_t N, int32_t K, int32_t with_bias);
int32_t regt_wgrad(const float* dOut, int64_t ldd, const float* A, int64_t lda, int64_t M, int32_t N, int32_t K,
                   float* dW, int64_t ldw, float* dbias, float* slab, regt_stream_t stream);
/* Diagnostic entry (kernel tests and A/B timings; no model path calls it): the row-chunk slabs of a weight gradient before their
 * reduction.  For each of the `nchunks` chunks of `kchunk` rows (the last may be shorter) slab[c] = P[chunk c]^T Q, (Nout x Nin)
 * floats, followed by the Nout column sums of P[chunk c] when colsum != 0.  The kernel is the one the library chooses for these
 * arguments under the current arithmetic and switches; any_rows != 0 lifts only the row-count gate of the wave-owned fp32 kernel
 * (Nin == 256, Nout % 256 == 0), so that it can be run on chunks of a few slabs.  *kernel (may be NULL) receives the name of the
 * kernel that ran (a static string). */
int32_t regt_wgrad_slabs(const float* P, int64_t ldp, int32_t Nout, const float* Q, int64_t ldq, int32_t Nin, int64_t M, int32_t kchunk,
                         int32_t nchunks, int32_t colsum, float* slab, int32_t any_rows, const char** kernel, regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-model forward / backward.
 *
 * regt_dims:  N nodes, T periods (<= 255), F node features, C hidden (256 in the reference), R regions,
 *             O output_dim, H1 head hidden (128);  regional = 1 for RegionalTemporalGCN
 *             (models/RegionalTemporalGCN.py:9-149), 0 for TemporalGCN / A3TGCN (models/TemporalGCN.py:7-91).
 * regt_graph: stacked CSR with 2N rows -- rows [0,N) = A_hat of the full graph, rows [N,2N) = the
 *             (merged, node-disjoint) regional scaled Laplacians; node_region (N) = region whose
 *             Laplacian owns the node's row; chunk_tab (n_chunks,2) = [row_begin,row_end) ranges of
 *             (node*T + t) rows that lie inside one region, chunk_region (n_chunks) their region.
 * regt_params: the reference's state_dict tensors (names in comments), read-only.
 * regt_grads:  same tensors, written (not accumulated) by regt_backward; NULL entries are skipped.
 *
 * Reproducibility: for T <= 64 (the reference uses 6 and 12) two calls on the same inputs give bit-identical outputs and
 * gradients -- every sum has a fixed order, and an element of the hidden state receives at most two atomically added
 * partial sums (two addends commute).  For 64 < T <= 255 a node spans three or more 64-row blocks of the candidate
 * kernel, its hidden state is the sum of three or more float atomics in arrival order, and results can differ in the last
 * bits from run to run (parity within 1e-5 still holds; tests/test_gpu_model.py runs T = 150).
 * ---------------------------------------------------------------------------------------------- */
typedef struct regt_dims {
    int32_t N, T, F, C, R, O, H1;
    int32_t regional;
    float lrelu_slope;      /* 0.01 (F.leaky_relu default, RegionalTemporalGCN.py:143) */
    /* ABI v6 -- per-call configuration (no process state involved; zero-initialised = the process defaults):
     * arith: GEMM arithmetic of THIS call: 0 = the process default (regt_set_gemm_mode / REGT_GEMM_MODE), 1 = fp32 MFMA,
     *        2 = exact bf16x3 split, 3 = bf16 operands.  regt_backward must be given the value its forward ran with
     *        (checked against what the forward stored in the workspace).
     * flags: REGT_DIMS_* bits below. */
    int32_t arith;
    uint32_t flags;
} regt_dims;
#define REGT_ARITH_DEFAULT 0
#define REGT_ARITH_FP32 1
#define REGT_ARITH_BF16X3 2
#define REGT_ARITH_BF16 3
#define REGT_DIMS_NO_BF16_ROWS 1u   /* bf16 arithmetic without the bf16-row layout / fused forward (= regt_set_option("xbf", 0)) */
#define REGT_DIMS_NO_FUSED_BWD 2u   /* bf16 arithmetic with the three data-gradient launches (= regt_set_option("fused_bwd", 0)) */
#define REGT_DIMS_NO_SIDE_STREAM 4u /* every kernel of this call on `stream` itself (no library side stream) */
#define REGT_DIMS_FORWARD_ONLY 8u   /* regt_forward / _packed / _packed_bf16 / regt_cell_forward: no backward will follow (see below) */
#define REGT_DIMS_NO_HEAD 16u       /* regt_forward / regt_backward without the head (see regt_backward below) */

typedef struct regt_graph {
    const int32_t* rowptr;        /* (2N+1) */
    const int32_t* col;
    const float* val;
    const int32_t* node_region;   /* (N) */
    const int32_t* chunk_tab;     /* (n_chunks, 2) */
    const int32_t* chunk_region;  /* (n_chunks) */
    int32_t n_chunks;
    /* optional merged operator (N rows): one entry per distinct (row, col) of the two halves above with the
     * A_hat weight and the L~ weight side by side; when present (and T*F % 32 == 0 or T*F <= 2048) both aggregations are
     * produced by ONE gather pass.  All four NULL = not provided. */
    const int32_t* m_rowptr;      /* (N+1) */
    const int32_t* m_col;
    const float* m_val_a;
    const float* m_val_l;
    /* overlap = 1: the regional graphs are NOT node-disjoint (the reference's "random" decomposition,
     * load_dataset.py:324-329).  rowptr/col/val then hold (1+R)*N rows: A_hat, then one scaled Laplacian per
     * region; node_region / chunk tables / merged operator are ignored. */
    int32_t overlap;
    /* Region ids [region_lo, region_hi) that own rows of THIS graph (a region shard of a multi-GPU run owns a block of
     * the global regions; tgnn.linear stays replicated at its global size).  Per-region composed weights are only
     * built for these, and the gradient blocks of the other regions receive just the term every region shares.
     * 0, 0 = all of [0, R). */
    int32_t region_lo, region_hi;
    /* 1 = node_region is non-decreasing (the nodes of a region are contiguous: what every shipped decomposition produces).  The bf16
     * arithmetic then runs the row-owning fused forward kernel (csrc/fused_rows.hip); 0 = unknown / not sorted: the 64-row fused
     * kernel, which handles any order.  (ABI v7) */
    int32_t region_sorted;
} regt_graph;

typedef struct regt_params {
    const float* attention;      /* tgnn._attention (T) */
    const float* conv_lin_w[3];  /* tgnn._base_tgcn.conv_{z,r,h}.lin.weight (C,F) */
    const float* conv_bias[3];   /* tgnn._base_tgcn.conv_{z,r,h}.bias (C) */
    const float* gate_w[3];      /* tgnn._base_tgcn.linear_{z,r,h}.weight (C,2C) */
    const float* gate_b[3];      /* tgnn._base_tgcn.linear_{z,r,h}.bias (C) */
    const float* cheb_w0;        /* tgnn.conv.lins.0.weight (C,F) */
    const float* cheb_w1;        /* tgnn.conv.lins.1.weight (C,F) */
    const float* cheb_bias;      /* tgnn.conv.bias (C) */
    const float* region_w;       /* tgnn.linear.weight (C,R*C)   (regional only) */
    const float* region_b;       /* tgnn.linear.bias (C)         (regional only) */
    const float* head1_w;        /* linear1.weight (H1,C) */
    const float* head1_b;        /* linear1.bias (H1) */
    const float* head2_w;        /* linear2.weight (O,H1) */
    const float* head2_b;        /* linear2.bias (O) */
} regt_params;

typedef struct regt_grads {
    float* attention;
    float* conv_lin_w[3];
    float* conv_bias[3];
    float* gate_w[3];
    float* gate_b[3];
    float* cheb_w0;
    float* cheb_w1;
    float* cheb_bias;
    float* region_w;
    float* region_b;
    float* head1_w;
    float* head1_b;
    float* head2_w;
    float* head2_b;
} regt_grads;

/* Bytes of device workspace regt_forward / regt_backward need (same buffer for both: the forward
 * leaves the activations the backward reads).  The size depends on the CU count of the current device (the weight-gradient slabs
 * are sized for the chunk counts the launches pick from it): call it with the execution device current. */
size_t regt_workspace_bytes(const regt_dims* dims, int32_t n_chunks, int32_t overlap);

/* Forward-only calls (evaluation, serving): with REGT_DIMS_FORWARD_ONLY in dims->flags the four forward entry points compute pred
 * and hidden exactly as without it -- bit for bit, same kernels' arithmetic and summation orders -- but write no array that only the
 * backward reads, and need only the bytes this function returns (a workspace of regt_workspace_bytes is accepted too).
 *   bf16 arithmetic on the fused forward (C = 256, F = 32 / 64, node-disjoint regions, merged operator): no (N*T x C) array at all --
 *     bf16 rows of x, A_hat x, L~ x, the head's (N x H1) activation, the composed weights.
 *   every other form (fp32, bf16x3, bf16 without bf16 rows, overlapping regions, TemporalGCN, regt_cell_forward): h, [Z | R] (the R
 *     half is left unwritten) and q = h R: four (N*T x C) element arrays instead of the training layout's nine.
 * The function reads host-side fields of `graph` only and dereferences no device pointer: overlap, n_chunks, region_sorted,
 * region_lo / region_hi and whether the m_* and chunk_* pointers are NULL; it picks the form the forward will take from them, from
 * dims->arith / dims->flags and the process options.  0 = invalid dims or NULL graph (message in regt_last_error).
 * The form is the one the training forward takes for the same call, so the flag never changes which arithmetic runs.
 * regt_forward_only_workspace_bytes sizes regt_forward and regt_cell_forward.  The packed entry points are sized by
 * regt_forward_only_packed_workspace_bytes with the call's own x_rows and row type (x_is_bf16: 0 = regt_forward_packed, 1 =
 * regt_forward_packed_bf16), because both enter the choice of the form exactly as in the forward (fp32 rows take the fused form up to
 * x_rows = 2 N, and x_rows * T * F * 2 must stay below 2^32 bytes) and the fused form keeps a bf16 copy of all x_rows fp32 rows in
 * the workspace.  With x_rows = N it returns what regt_forward_only_workspace_bytes returns.  0 also for x_rows < N, and for bf16
 * rows where the fused form does not apply (regt_forward_packed_bf16 refuses those).
 * Refused with an error, before anything is launched: a forward-only call with workspace_bytes below its sizing function's value
 * (a workspace of exactly that value is accepted); and regt_backward / regt_cell_backward on a workspace whose last forward was
 * forward-only (it holds nothing they could read).
 * As with regt_workspace_bytes, a size may depend on the CU count of the current device (today only the training layout's slab region
 * does): call both with the execution device current. */
size_t regt_forward_only_workspace_bytes(const regt_dims* dims, const regt_graph* graph);
size_t regt_forward_only_packed_workspace_bytes(const regt_dims* dims, const regt_graph* graph, int32_t x_rows, int32_t x_is_bf16);

/* x (N,F,T) -> pred (N,O), hidden (N,C).  RegionalTemporalGCN.forward / TemporalGCN.forward. */
int32_t regt_forward(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const float* x,
                     float* pred, float* hidden, void* workspace, size_t workspace_bytes, regt_stream_t stream);

/* Region-sharded variant (one process per GPU): the caller has already packed its own N rows with
 * regt_pack_x into the first N rows of x_packed (x_rows >= N rows of T*F floats) and filled rows
 * [N, x_rows) with the halo rows received from the other ranks; graph->col of the A_hat half may
 * point at any of the x_rows rows.  Everything else is as regt_forward. */
int32_t regt_forward_packed(const regt_dims* dims, const regt_graph* graph, const regt_params* params,
                            const float* x_packed, int32_t x_rows, float* pred, float* hidden,
                            void* workspace, size_t workspace_bytes, regt_stream_t stream);

/* The same for a caller that packs (regt_pack_x_bf16) and exchanges its rows as bf16 -- half the bytes on the xGMI links and
 * no conversion pass; needs REGT_GEMM_MODE=bf16 and a shape the fused forward covers (C = 256, F = 64, node-disjoint
 * regions, merged operator), otherwise an error is returned.  regt_backward must then get the same buffer as x_packed. */
int32_t regt_forward_packed_bf16(const regt_dims* dims, const regt_graph* graph, const regt_params* params,
                                 const void* x_packed_bf16, int32_t x_rows, float* pred, float* hidden,
                                 void* workspace, size_t workspace_bytes, regt_stream_t stream);

/* Gradients of all parameters given dL/dpred (N,O) and optionally dL/dhidden (N,C) (may be NULL).
 * Must follow regt_forward on the same workspace; `hidden` is that forward's hidden output;
 * x_packed is NULL after regt_forward, or the buffer given to regt_forward_packed. */
/* REGT_DIMS_NO_HEAD in dims->flags: the cell alone, for a caller that runs the head elsewhere (regt_window_backward).
 *   regt_forward:  pred may be NULL and is not written; the head is not run.  Combines with REGT_DIMS_FORWARD_ONLY.
 *   regt_backward: dpred may be NULL and is not read; dhidden is required (16-byte aligned) and is the WHOLE upstream gradient of
 *     `hidden`; the head launches are skipped and grads->head1_w / head1_b / head2_w / head2_b are neither read nor written.  Every
 *     other gradient is what a call without the flag gives for dpred = 0 and the same dhidden, bit for bit.
 * Without the flag everything is as before (a NULL dpred is refused).  regt_forward_packed / _packed_bf16 and regt_cell_forward /
 * regt_cell_backward refuse the flag. */
int32_t regt_backward(const regt_dims* dims, const regt_graph* graph, const regt_params* params,
                      const regt_grads* grads, const float* dpred, const float* dhidden, const float* hidden,
                      const float* x_packed, void* workspace, size_t workspace_bytes, regt_stream_t stream);

/* The part of the path every A3TGCN-style model of the reference shares -- TGCN cell (models/utils.py:163-203) over all
 * periods, attention-weighted sum, relu/linear head -- on a hidden input the CALLER computed: h_in is (N*T, C), row
 * node*T + t.  Replaces `self._base_tgcn(X[:, :, period], edge_index, edge_weight, h)` + head for models whose
 * embedding stage is not the regional one, e.g. models/ConvStackedTemporalGCN.py:117-126 (five stacked GCNConv).
 * dims.regional must be 0, dims.R is ignored (pass 1); graph needs rowptr/col/val of A_hat only (N rows, regt_gcn_csr);
 * params/grads: cheb_* and region_* are not used.  Workspace: regt_workspace_bytes(dims, 0, 0).
 * regt_cell_backward additionally returns dL/dh_in in dh_in (N*T, C). */
int32_t regt_cell_forward(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const float* x,
                          const float* h_in, float* pred, float* hidden, void* workspace, size_t workspace_bytes,
                          regt_stream_t stream);
int32_t regt_cell_backward(const regt_dims* dims, const regt_graph* graph, const regt_params* params,
                           const regt_grads* grads, const float* dpred, const float* dhidden, const float* hidden,
                           const float* h_in, float* dh_in, void* workspace, size_t workspace_bytes, regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * One step of the TGCN cell alone -- TGCN.forward(X, edge_index, edge_weight, H), models/utils.py:163-203 -- with no attention and no
 * head, differentiable in X and H (additive entries: REGT_ABI_VERSION is unchanged).
 *     H' (N, C) = Z * H + (1 - Z) * H~      x (N, F), A_hat = graph (N rows, regt_gcn_csr), h_in (N, C) or NULL = zeros
 * dims: T must be 1 and regional 0; R, O and H1 are ignored; arith fp32 or bf16x3 (the bf16 arithmetic is refused).  params / grads:
 * only conv_lin_w, conv_bias, gate_w and gate_b are used, every other entry may be NULL.
 * regt_tgcn_forward runs the cell stages of regt_cell_forward at T = 1: h_out is, bit for bit, the `hidden` regt_cell_forward gives
 * with a ONE-element attention tensor (a single logit has probability exactly 1).  REGT_DIMS_FORWARD_ONLY: same h_out, a smaller
 * workspace (regt_tgcn_workspace_bytes with the flag set), and regt_tgcn_backward on that workspace is refused.
 * regt_tgcn_backward must follow regt_tgcn_forward on the same workspace with the same h_in (NULL again where it was NULL); h_out is
 * that forward's output, dh_out (N, C) the whole upstream gradient.  The parameter gradients (written, not accumulated) and dh_in are
 * those of regt_cell_backward at T = 1 for dpred = 0 and dhidden = dh_out, bit for bit.  dx (N, F), optional (NULL = not wanted:
 * nothing is launched for it), is the gradient of x:
 *     dAx (N, F) = dzp Gz + drp Gr + dhp Gh      (csrc/cell_dx.hip: the three pre-activation gradients are read once, 3 N C floats;
 *                                                 G_k = U_k[:, :C] W_k are the composed (C, F) weights of the forward)
 *     dx  (N, F) = A_hat^T dAx                   (regt_spmm_csr over t_rowptr / t_col / t_val, the CSR of A_hat^T)
 * dh_in (N, C), optional, is the gradient of h_in.  Every sum has a fixed order: bit-reproducible.
 * Refused before anything is launched (message in regt_last_error): NULL dims / graph / required params, grads or pointers; C % 4 or
 * F % 4 != 0; T != 1; regional != 0; the bf16 arithmetic; workspace_bytes below regt_tgcn_workspace_bytes(dims) (0 = refused dims);
 * dx without the transposed operator; x, h_in, h_out, dh_out, dx, dh_in or workspace not 16-byte aligned; F > 64 with dx.
 * ---------------------------------------------------------------------------------------------- */
size_t regt_tgcn_workspace_bytes(const regt_dims* dims);
int32_t regt_tgcn_forward(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const float* x, const float* h_in,
                          float* h_out, void* workspace, size_t workspace_bytes, regt_stream_t stream);
int32_t regt_tgcn_backward(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const regt_grads* grads,
                           const float* dh_out, const float* h_in, const float* h_out, const int32_t* t_rowptr, const int32_t* t_col,
                           const float* t_val, float* dx, float* dh_in, void* workspace, size_t workspace_bytes, regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The whole model's input gradient dL/dx (N, F, T) of RegionalTemporalGCN / TemporalGCN (additive entries: REGT_ABI_VERSION is unchanged).
 * regt_input_gradient must follow regt_backward (and its regt_forward) on the same workspace with the same dims, graph and params;
 * REGT_DIMS_NO_HEAD is allowed.  It reads what regt_backward left there -- dzr = [dp_z | dp_r] (M, 2C), dhp (M, C) and ds (M, C), the
 * embedding's pre-activation gradient; rows m = node T + t -- and the composed weights of the forward, writes nothing into the workspace and
 * changes no output of regt_backward:
 *     dAX (M, F) = dzr [Gz; Gr] + dhp Gh      dXd = ds A0      dLX = ds A_region(node)      (csrc/model_dx.hip: one pass over the rows,
 *                                                                                            4 M C floats in, 3 M F floats out)
 *     collapsed TemporalGCN form:             dXd = dzr P0zr + dh W0      dLX = dzr P1zr + dh W1
 *     dx (N, F, T) = unpack(dXd + A_hat^T dAX + L~^T dLX)                                   (csrc/spmm_dual_t.hip)
 * t_rowptr (N + 1), t_col, t_val_a, t_val_l: the CSR of the TRANSPOSE of the merged operator (graph->m_*), both weights per entry; the
 * entries of a row ordered by their original row id.  L~ is not symmetric for asymmetric edge weights: the forward's operator does not do.
 * scratch: regt_input_gradient_scratch_bytes(dims) bytes of the caller's, 16-byte aligned (0 = refused dims); the workspace layout and
 * regt_workspace_bytes are unchanged.  Covers fp32 and bf16x3, node-disjoint regions in any node order, R = 1, TemporalGCN in both forms,
 * T <= 255, block-diagonal (snapshot-batched) graphs.  Every sum has a fixed order: bit-reproducible.  All launches go on `stream`.
 * graph->node_region is read on the device and not validated: an id outside [0, R) is clamped into that range (the gradient of such a
 * row is then wrong; no memory outside the region blocks is read).
 * Refused before anything is launched (message in regt_last_error): NULL dims / graph / params / dx / workspace / scratch; dx, workspace,
 * scratch or the Chebyshev weights not 16-byte aligned; workspace_bytes below regt_workspace_bytes or scratch_bytes below
 * regt_input_gradient_scratch_bytes; the bf16 arithmetic; graph->overlap = 1; a workspace whose last forward ran with
 * REGT_DIMS_FORWARD_ONLY or read packed rows (regt_forward_packed*: halo gradients need an exchange); F > 64; a NULL transposed operator.
 * ---------------------------------------------------------------------------------------------- */
size_t regt_input_gradient_scratch_bytes(const regt_dims* dims);
int32_t regt_input_gradient(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const int32_t* t_rowptr,
                            const int32_t* t_col, const float* t_val_a, const float* t_val_l, float* dx, void* workspace,
                            size_t workspace_bytes, void* scratch, size_t scratch_bytes, regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Streaming inference: the attention-weighted sum over a RING of cached per-time-step cell outputs, then the head.
 *
 * RegionalA3TGCN.forward / A3TGCN.forward call the cell with H = None in every period (models/RegionalTemporalGCN.py:134-146,
 * models/TemporalGCN.py:84-90), so the cell's output S_s (N, C) of raw time step s does not depend on the window it is read through.
 * S_s is what regt_forward returns as `hidden` for T = 1 with a ONE-element attention tensor (a single logit has probability exactly
 * 1); REGT_DIMS_FORWARD_ONLY applies.  A caller keeps the last outputs in `ring` and replaces T - 1 of every window's T cell
 * evaluations by reads:
 *     hidden[w, n, c] = sum_{p < T} softmax(attention)_p * ring[(first_slot + w + p) % ring_len, n, c]        w < windows
 *     pred[w]         = linear2(relu(linear1(relu(hidden[w]))))
 * Layout: ring (ring_len, N, C) fp32 contiguous, slab s = the cell output of one time step; window w covers slots first_slot + w ..
 * first_slot + w + T - 1, modulo ring_len; pred (windows, N, O), hidden (windows, N, C); attention (T) are the model's logits, the
 * head tensors are regt_params' head1_w/b, head2_w/b.  ring, hidden and workspace 16-byte aligned.
 * Order: every element of hidden is accumulated p = 0, 1, .., T - 1 with one fused multiply-add each, starting from 0: a window's
 * hidden (and pred) is the same bits for every windows, first_slot, ring_len it is computed with.  Slabs outside the
 * windows + T - 1 slots named above are not read.  The head runs in the process arithmetic (regt_set_gemm_mode).
 * Limits: C % 4 == 0, 1 <= T <= 255, windows * N < 2^31, windows <= 65535 * regt_window_chunk(2) (= 1 048 560).
 * Refused before anything is launched (message in regt_last_error): a NULL pointer; ring_len < T; first_slot outside [0, ring_len);
 * windows > 1 with windows + T - 1 > ring_len (the windows would wrap onto themselves; a single window may start anywhere); C % 4 != 0;
 * T > 255; a limit above exceeded; workspace_bytes below regt_window_workspace_bytes(N, C, H1, O, windows) (0 = refused dimensions).
 * regt_window_chunk(windows): how many windows one thread of the kernel accumulates at once for a call of `windows` windows (1 for a
 * single window, the chunk width WC otherwise): a chunk of nw <= WC windows reads nw + T - 1 slabs and writes nw.
 * ---------------------------------------------------------------------------------------------- */
int32_t regt_window_chunk(int32_t windows);
size_t regt_window_workspace_bytes(int32_t N, int32_t C, int32_t H1, int32_t O, int32_t windows);
int32_t regt_window_forward(const float* ring, int32_t ring_len, int32_t first_slot, int32_t windows, int32_t N, int32_t T,
                            int32_t C, int32_t O, int32_t H1, const float* attention, const float* head1_w, const float* head1_b,
                            const float* head2_w, const float* head2_b, float* pred, float* hidden, void* workspace,
                            size_t workspace_bytes, regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Streamed training: the backward of regt_window_forward.
 *
 * With fixed weights the gradient of a run of consecutive stride-1 windows factors through the per-step cell outputs S_s:
 *     dring[slot(j)]  (+)= sum_{w : 0 <= j - w < T} prob[j - w] * dhidden[w]          j < windows + T - 1   (the step's dS)
 *     d_attention[p]  (+)= prob[p] * (dprob[p] - sum_q prob[q] dprob[q]),   dprob[p] = sum_{w, n, c} dhidden[w, n, c] * ring[slot(w + p), n, c]
 * with slot(j) = (first_slot + j) % ring_len, prob = softmax(attention) and dhidden = the head's backward on dpred.  The call recomputes
 * the head's hidden activation from `hidden` (the forward's output; its workspace is not needed), runs the head's backward on
 * windows * N rows (dhidden stays in the workspace) and then the two passes above.  ring, hidden, dpred as in regt_window_forward;
 * dring has the ring's shape and slot mapping.
 * accumulate = 0: d_attention, d_head1_w, d_head1_b, d_head2_w, d_head2_b and the windows + T - 1 covered slots of dring are written;
 * accumulate = 1: they are added to.  Slots of dring outside the covered ones are not touched.
 * Order: a covered slot's accumulator starts from the value dring holds (accumulate = 1) or from 0 and receives its windows in
 * ascending window order, one fused multiply-add each.  So the dS of a step is the same bits whether its windows arrive in one call
 * or split over consecutive accumulating calls in ascending order, whatever chunk of the kernel it falls in and whatever first_slot /
 * ring_len are: a batch of windows hands its partial sums to the next one through dring.  d_attention is reduced in a fixed order that
 * depends on the arguments and the device's CU count only (two calls give the same bits).
 * Limits: regt_window_forward's, T <= regt_window_backward_max_t() (32), windows + T - 1 <= ring_len for every window count.
 * Refused before anything is launched: regt_window_forward's list, a larger T, workspace_bytes below
 * regt_window_backward_workspace_bytes(N, C, H1, O, windows, T) (0 = refused dimensions; it depends on the CU count of the current
 * device), dring / hidden / workspace not 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
size_t regt_window_backward_workspace_bytes(int32_t N, int32_t C, int32_t H1, int32_t O, int32_t windows, int32_t T);
int32_t regt_window_backward_max_t(void);
int32_t regt_window_backward(const float* ring, int32_t ring_len, int32_t first_slot, int32_t windows, int32_t N, int32_t T,
                             int32_t C, int32_t O, int32_t H1, const float* attention, const float* head1_w, const float* head1_b,
                             const float* head2_w, const float* head2_b, const float* hidden, const float* dpred, float* dring,
                             int32_t accumulate, float* d_attention, float* d_head1_w, float* d_head1_b, float* d_head2_w,
                             float* d_head2_b, void* workspace, size_t workspace_bytes, regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Zero-hidden TGCN cell + attention over periods + head, on gate inputs the CALLER aggregated.
 *
 * The reference's GraphSAGETemporalGCN and GATTemporal call `self._base_tgcn(X[:, :, period], edge_index, H)`
 * (models/GraphSAGETemporalGCN.py:93-95, models/GATTemporal.py:78-80): the third positional parameter of TGCN.forward is
 * edge_weight, so H stays None and the cell starts from zeros (models/utils.py:163-166).  With H = 0 the GRU reduces to
 *     Z = sigmoid(a_z gz^T + cz),   H~ = tanh(a_h gh^T + ch),   H' = (1 - Z) * H~,   hidden = sum_t softmax(att)_t H'_t
 * (the reset gate only ever multiplies H = 0).  a_z (M, kz) / a_h (M, kh), M = N*T rows ordered node*T + t, are the
 * aggregated inputs of the two live gates -- [mean-neighbour x | x] for SAGEConv, the attention-weighted neighbour sum of
 * GATConv (regt_gat_forward) -- and gz (C, kz) / gh (C, kh), cz / ch (C) the composed weights U_k[:, :C] W_k and biases
 * U_k[:, :C] b_k + u_k.  dims: N, T, C, O, H1 are used.  regt_cell0_backward writes the gradients of args' tensors; the
 * optional a_z / a_h entries (M, kz) / (M, kh) receive dL/d(input) (needed when the inputs depend on parameters: GAT).
 * ---------------------------------------------------------------------------------------------- */
typedef struct regt_cell0_args {
    const float* a_z; const float* a_h;
    int32_t kz, kh;
    const float* gz; const float* gh; const float* cz; const float* ch;
    const float* attention;                                          /* (T) */
    const float* head1_w; const float* head1_b; const float* head2_w; const float* head2_b;
} regt_cell0_args;
typedef struct regt_cell0_grads {
    float* a_z; float* a_h;                                          /* optional (NULL = not needed) */
    float* gz; float* gh; float* cz; float* ch;
    float* attention;                                                /* optional */
    float* head1_w; float* head1_b; float* head2_w; float* head2_b;
} regt_cell0_grads;
size_t regt_cell0_workspace_bytes(const regt_dims* dims, int32_t kz, int32_t kh);
int32_t regt_cell0_forward(const regt_dims* dims, const regt_cell0_args* args, float* pred, float* hidden, void* workspace,
                           size_t workspace_bytes, regt_stream_t stream);
int32_t regt_cell0_backward(const regt_dims* dims, const regt_cell0_args* args, const regt_cell0_grads* grads, const float* dpred,
                            const float* dhidden, const float* hidden, void* workspace, size_t workspace_bytes,
                            regt_stream_t stream);

/* GATConv (heads = 1, add_self_loops, negative_slope `slope`) attention aggregation on the INPUT rows, all T periods at once:
 *   e_ij = leaky_relu(<x_j, u_src> + <x_i, u_dst>),  alpha_ij = softmax over the in-edges of i,  out_i = sum_j alpha_ij x_j
 * with u_src = W^T att_src, u_dst = W^T att_dst (F) -- the conv's output is then out W^T + bias (models/utils.py:97-98 call
 * sites).  rowptr/col: the pattern of regt_gcn_csr (in-edges without self loops + one self loop per node).  x, out:
 * (N, T, F) packed rows; stats (N*T, 4) floats are kept for the backward.  regt_gat_backward turns dL/dout (N, T, F) into
 * the score gradients dsd (N*T, 2) = (dL/ds_j, dL/dd_i) per row; du_src = dsd[:, 0]^T x and du_dst = dsd[:, 1]^T x are then
 * ordinary regt_wgrad contractions.  t_rowptr/t_col: the transposed pattern (out-edges of every node).  F % 4 == 0, F <= 256;
 * x, out, dout, u_src, u_dst and stats 16-byte aligned (rows are read and written in 16-byte pieces). */
int32_t regt_gat_forward(const int32_t* rowptr, const int32_t* col, const float* x, const float* u_src, const float* u_dst,
                         float slope, int32_t num_nodes, int32_t periods, int32_t num_features, float* out, float* stats,
                         regt_stream_t stream);
int32_t regt_gat_backward(const int32_t* rowptr, const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col,
                          const float* x, const float* u_src, float slope, int32_t num_nodes, int32_t periods,
                          int32_t num_features, const float* dout, float* stats, float* dsd, regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * SpatialGCN (models/SpatialGCN.py): its first ChebConv(K=2, 64 channels), ReLU and dropout, summed over the periods
 * (the second ChebConv is linear and its outputs are summed over the periods, so it runs once, on this sum):
 *   S[n, :] = sum_{t = 0..T-1} keep_t * 2 * relu(x[n,t,:] W0^T + lx[n,t,:] W1^T + bias)      (eval: keep = NULL, no scale)
 * x_packed (N, T, F) from regt_pack_x, lx_packed = L~ x_packed at width T*F (regt_spmm_csr over the ChebConv operator);
 * w0 / w1 (64, F) = gcn.lins.{0,1}.weight, bias (64) = gcn.bias; S (N, 64).  keep: uint32 (N*T, 2), row node*T + t, bit j
 * of word w keeps channel 32w + j; NULL = eval mode.  F % 4 == 0, 4 <= F <= 64, 1 <= T <= 255; x, lx, bias, S, dS 16-byte
 * aligned.  The backward recomputes the pre-activation and writes dw0, dw1 (64, F) and dbias (64) from dS (N, 64); it needs
 * `slab` of regt_spatial_embed_slab_floats(N, T, F) floats (0 = invalid dims).  Sums run in a fixed order: bit-reproducible.
 * ---------------------------------------------------------------------------------------------- */
size_t regt_spatial_embed_slab_floats(int32_t num_nodes, int32_t periods, int32_t num_features);
int32_t regt_spatial_embed_forward(const float* x_packed, const float* lx_packed, const float* w0, const float* w1, const float* bias,
                                   const uint32_t* keep, int32_t num_nodes, int32_t periods, int32_t num_features, float* s_out,
                                   regt_stream_t stream);
int32_t regt_spatial_embed_backward(const float* x_packed, const float* lx_packed, const float* w0, const float* w1,
                                    const float* bias, const uint32_t* keep, const float* ds, int32_t num_nodes, int32_t periods,
                                    int32_t num_features, float* dw0, float* dw1, float* dbias, float* slab, regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * STNorm (models/STNorm.py) with channels = 16, kernel_size = 2: start_conv, blocks * layers gated dilated-conv layers on
 * [x | TNorm(x) | SNorm(x)] with residual and skip connections, and the two-conv head.
 *   x (batch, seq_len, num_nodes, in_dim) -- the reference's forward input; out (batch, out_dim, num_nodes, L_out) with
 *   L_out = max(seq_len, RF) - RF + 1, RF = 1 + blocks * (2^layers - 1).
 *   params: device pointers, 6 head entries (start_conv.weight, .bias, end_conv_1.weight, .bias, end_conv_2.weight, .bias),
 *   then 12 per layer i (filter_convs.i.weight, .bias, gate_convs.i.*, residual_convs.i.*, skip_convs.i.*, tn.i.gamma,
 *   tn.i.beta, sn.i.gamma, sn.i.beta; NULL where tnorm / snorm is 0).  running: tn.i.running_mean, tn.i.running_var per
 *   layer (NULL table when tnorm is 0).  grads: the layout of params.
 *   tnorm_group: TNorm statistics pool groups of that many consecutive batch elements (batch for the module call); in
 *   training mode the forward updates the running buffers group by group, in order.  The forward writes the layer inputs
 *   and statistics the backward reads into `workspace`; the backward alone uses `scratch`.  Sizes in floats from
 *   regt_stnorm_sizes (REGT_ERR_ARG for invalid dims).  num_nodes >= 2; 1 <= in_dim, out_dim <= 256; layers <= 8;
 *   blocks * layers <= 64 (in_dim / out_dim: the LDS rows of the start-conv / head backward).  Every table entry
 *   must be a contiguous fp32 device tensor of the reference's shape (regtgcn_amd.ops checks that before the call).  Sums run in a fixed order without float atomics: bit-reproducible.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t num_nodes, batch, tnorm_group, seq_len, in_dim, out_dim, blocks, layers, tnorm, snorm, training;
} regt_stnorm_dims;
int32_t regt_stnorm_sizes(const regt_stnorm_dims* dims, size_t* workspace_floats, size_t* scratch_floats);
int32_t regt_stnorm_forward(const regt_stnorm_dims* dims, const float* x, const float* const* params, float* const* running,
                            float* out, float* workspace, regt_stream_t stream);
int32_t regt_stnorm_backward(const regt_stnorm_dims* dims, const float* x, const float* const* params, float* const* running,
                             const float* dout, float* const* grads, const float* workspace, float* scratch, regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * STID (models/STID.py) with if_time_in_day = if_day_in_week = False, as run.py:134 builds it: a per-node network.
 *   x (batch, input_len, num_nodes, in_features) -- the reference's forward input; the kernels read the first input_dim
 *   features of every time step in place.  out (batch, output_len, num_nodes, 1).
 *   params: device pointers in state_dict order: node_emb (num_nodes, 32) (NULL when if_node is 0),
 *   time_series_emb_layer.weight (32, input_dim * input_len, 1, 1), .bias, then per layer i encoder.i.fc1.weight
 *   (hidden, hidden, 1, 1), .bias, encoder.i.fc2.weight, .bias, then regression_layer.weight (output_len, hidden, 1, 1),
 *   .bias: 3 + 4 * num_layer + 2 entries, hidden = 32 + 32 * if_node.  grads: the layout of params.
 *   keep: NULL (eval: no dropout) or int32 words (num_layer, batch, num_nodes, hidden / 32); bit j of word w keeps channel
 *   32 w + j of the block's activation, kept values are scaled by 1 / (1 - dropout_p).  The backward takes the same words.
 *   workspace: NULL (nothing is kept) or workspace_floats floats, which the forward fills with the block inputs and
 *   activations that the backward reads; scratch is the backward's own.  Sizes from regt_stid_sizes (REGT_ERR_ARG for
 *   invalid dims).  Limits: embed_dim == node_dim == 32; 1 <= num_layer <= 8; 1 <= input_len <= 255;
 *   1 <= input_dim <= in_features <= 256; input_dim * input_len <= 192; 1 <= output_len <= 64; num_nodes, batch >= 1;
 *   0 <= dropout_p < 1.  Every table entry must be a contiguous fp32 device tensor of the reference's shape
 *   (regtgcn_amd.ops checks that before the call).  Sums run in a fixed order without float atomics: bit-reproducible.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t num_nodes, batch, input_len, in_features, input_dim, embed_dim, node_dim, num_layer, output_len, if_node;
    float dropout_p;
} regt_stid_dims;
int32_t regt_stid_sizes(const regt_stid_dims* dims, size_t* workspace_floats, size_t* scratch_floats);
int32_t regt_stid_forward(const regt_stid_dims* dims, const float* x, const float* const* params, const uint32_t* keep, float* out,
                          float* workspace, regt_stream_t stream);
int32_t regt_stid_backward(const regt_stid_dims* dims, const float* x, const float* const* params, const uint32_t* keep,
                           const float* dout, float* const* grads, const float* workspace, float* scratch, regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * One torch.nn.GRU layer (one layer, one direction, gates stacked r, z, n) over a whole sequence: what models/StackedGRU.py
 * runs twice.  r = sigmoid(W_ir x + b_ir + W_hr h + b_hr), z likewise, n = tanh(W_in x + b_in + r (W_hn h + b_hn)),
 * h' = (1 - z) n + z h.
 *   x: element (step s, row b, input k) at x[s * x_stride_seq + b * x_stride_row + k * x_stride_t] (strides in elements, >= 0),
 *   read in place.  w_ih (768, input_size), w_hh (768, 256), b_ih, b_hh (768).  h0 (rows, 256) or NULL (zeros).
 *   out (seq_len, rows, 256) or NULL; h_last (rows, 256) or NULL; not both NULL.
 *   workspace: workspace_floats floats, always required (it holds the repacked weights); with training = 1 the forward also
 *   leaves every step's state and gate activations there for the backward.  The size depends on training.
 *   regt_gru_backward (training = 1 only): weights = {w_ih, w_hh, b_ih, b_hh}, grads the same layout (overwritten);
 *   dout (seq_len, rows, 256) or NULL, dh_last (rows, 256) or NULL, not both NULL; dh0 (rows, 256) or NULL receives the
 *   gradient of h0.  h0 is accepted for symmetry and not read (the workspace holds it).  scratch: scratch_floats floats.
 *   Limits: hidden == 256; 1 <= input_size <= 255; seq_len >= 1; rows >= 1; seq_len * rows < 2^31 - rows.  workspace and
 *   scratch 16-byte aligned.  One workgroup owns 8 rows for the whole sequence and waits for no other workgroup.  Sums run in
 *   a fixed order without float atomics: bit-reproducible.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t seq_len, rows, input_size, hidden, training;
    int64_t x_stride_seq, x_stride_row, x_stride_t;
} regt_gru_dims;
int32_t regt_gru_sizes(const regt_gru_dims* dims, size_t* workspace_floats, size_t* scratch_floats);
int32_t regt_gru_forward(const regt_gru_dims* dims, const float* x, const float* w_ih, const float* w_hh, const float* b_ih,
                         const float* b_hh, const float* h0, float* out, float* h_last, float* workspace, regt_stream_t stream);
int32_t regt_gru_backward(const regt_gru_dims* dims, const float* x, const float* const* weights, const float* h0, const float* dout,
                          const float* dh_last, float* const* grads, float* dh0, const float* workspace, float* scratch,
                          regt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * STAEformer (models/STAEformer.py), INFERENCE only (dropout is the identity; nothing is kept for a backward), with
 * use_mixed_proj = True.  run.py:132 builds it with tod_embedding_dim = 0: model_dim = 24 + 24 + 80 = 128, 4 heads of 32.
 *   x (batch, in_steps, num_nodes, in_features) -- the reference's forward input; the first input_dim features feed input_proj,
 *   feature 1 * steps_per_day indexes tod_embedding and feature 2 indexes dow_embedding, truncated toward zero as .long() does
 *   and then CLAMPED into the table (negative or NaN -> row 0, too large -> the last row; the reference raises there): nothing
 *   outside a table is read.  out (batch, out_steps, num_nodes, output_dim).
 *   model_dim = input_embedding_dim + tod_embedding_dim + dow_embedding_dim + spatial_embedding_dim + adaptive_embedding_dim,
 *   concatenated in that order; a block of width 0 is absent.
 *   params: device pointers in state_dict order: node_emb (num_nodes, spatial), adaptive_embedding (in_steps, num_nodes,
 *   adaptive), input_proj.weight (input_embedding_dim, input_dim), .bias, tod_embedding.weight (steps_per_day, tod),
 *   dow_embedding.weight (days_per_week, dow) -- NULL where the width is 0 --, output_proj.weight (out_steps * output_dim,
 *   in_steps * model_dim), .bias; then 16 per layer, the num_layers temporal layers first, then the num_layers spatial ones:
 *   attn.FC_Q.weight, .bias, attn.FC_K.*, attn.FC_V.*, attn.out_proj.*, feed_forward.0.*, feed_forward.2.*, ln1.weight, .bias,
 *   ln2.weight, .bias: 8 + 32 * num_layers entries.
 *   workspace: workspace_floats floats from regt_stae_sizes (REGT_ERR_ARG outside the limits), 16-byte aligned: two activation
 *   buffers, Q|K|V, the attention output and the feed-forward hidden.
 *   Limits: head width model_dim / num_heads == 32; model_dim % 32 == 0, model_dim <= 256; feed_forward_dim % 32 == 0,
 *   feed_forward_dim <= 1024; 1 <= in_steps <= 255; 1 <= num_layers <= 8; 1 <= input_dim <= in_features <= 256 (in_features >= 2
 *   / >= 3 with a time-of-day / day-of-week embedding); out_steps * output_dim <= 64; use_mixed_proj == 1; input_embedding_dim >= 1;
 *   steps_per_day, days_per_week, batch, num_nodes >= 1; ln_eps > 0.  Every table entry must be a contiguous fp32 device tensor of
 *   the reference's shape (regtgcn_amd.ops checks that before the call).  Sums run in a fixed order without float atomics:
 *   bit-reproducible.
 *
 * regt_stae_attention: multi-head self-attention softmax(Q K^T / sqrt(32)) V along one axis of a (B, T, N, 32 * heads) tensor whose
 *   rows (b T + t) N + n lie ld floats apart in q, k and v (three pointers, possibly column windows of one buffer) and ldo floats
 *   apart in out.  axis = 1: along T, one sequence per (b, n); axis = 2: along N, one sequence per (b, t).  Head h owns columns
 *   [32 h, 32 h + 32).  Any sequence length; no score matrix is formed in memory; no mask.  heads <= 8; ld, ldo multiples of 4 and
 *   >= 32 * heads; q, k, v, out 16-byte aligned.  Only the M x 32 * heads window of out is written.
 * regt_stae_add_layernorm: out = LayerNorm(residual + y) * gamma + beta over rows of D floats (biased variance, eps inside the
 *   root, as nn.LayerNorm); dense rows; out may alias residual.  D % 32 == 0, 32 <= D <= 256; 1 <= M < 2^31.
 *
 * Training of one self-attention layer (regtgcn_amd.nn.SelfAttentionLayer composes these with regt_linear / regt_wgrad /
 * regt_relu_backward; the whole model still runs for inference only).  Additive entries, fp32, no float atomics, bit-reproducible.
 * regt_stae_attention_train: regt_stae_attention that also stores lse (M x heads floats, row-major, 16-byte aligned): per (row,
 *   head) the log-sum-exp of the scaled scores.  out is the same, bit for bit, as regt_stae_attention's.
 * regt_stae_attention_backward: given out and dout (rows ldo apart) and lse of the training forward, writes dq, dk, dv, whose rows
 *   lie one common ldg floats apart (three pointers, possibly the column windows of one M x 3 * 32 * heads buffer); only their
 *   M x 32 * heads windows are written.  scratch: regt_stae_attention_backward_scratch_floats floats (0: arguments out of
 *   range), 16-byte aligned.  Same limits as regt_stae_attention; ld, ldo, ldg multiples of 4, >= 32 * heads; every pointer 16-byte
 *   aligned; batch * in_steps * num_nodes < 2^31 / 4.  No score matrix is formed in memory.
 * regt_stae_add_layernorm_backward: for out = LayerNorm(residual + y) * gamma + beta (regt_stae_add_layernorm with out different
 *   from residual) and dout = dL/dout: dz (M x D) = dL/dresidual = dL/dy, dgamma (D), dbeta (D).  The row statistics are recomputed
 *   from residual and y; gamma may hold zeros.  dz must not alias an input.  scratch:
 *   regt_stae_add_layernorm_backward_scratch_floats floats (0: arguments out of range).  D % 32 == 0, 32 <= D <= 256;
 *   1 <= M < 2^31 / 4; eps > 0; every pointer 16-byte aligned.
 *
 * Training of the whole model (regtgcn_amd.nn.STAEformerTrainable composes these with the layer's entries above).  Additive
 * entries, fp32, no float atomics, bit-reproducible; nothing outside the documented windows is written.  dims is checked as for
 * regt_stae_forward (same limits), M = batch * in_steps * num_nodes rows of D = model_dim floats, rows (b T + t) N + n.
 * regt_stae_embed: layer 0's input X0 (M x D, dense rows) from x -- the very kernel regt_stae_forward starts with.  params: the
 *   first six entries of the table above (node_emb, adaptive_embedding, input_proj.weight, .bias, tod_embedding.weight,
 *   dow_embedding.weight; NULL where the width is 0).
 * regt_stae_embed_backward: given x and dx0 (M x D, dense rows) writes the gradients of those six entries into grads (same order,
 *   same shapes, NULL where the width is 0 -- both ways); x gets no gradient.  A table row's gradient goes to the row the forward
 *   read AFTER its clamp; a row no input hits gets exactly 0.  Limit: input_embedding_dim * (input_dim + 1) + steps_per_day *
 *   tod_embedding_dim + days_per_week * dow_embedding_dim <= 15360 floats (one chunk's partial sums live in the LDS).  scratch:
 *   regt_stae_embed_backward_scratch_floats floats (0: arguments out of range): one partial of that many floats per chunk of rows.
 * regt_stae_output_proj: out (batch, out_steps, num_nodes, output_dim), contiguous, = the use_mixed_proj tail of x (M x D) -- the
 *   very kernel regt_stae_forward ends with.  w (out_steps * output_dim, in_steps * D), bias (out_steps * output_dim).
 * regt_stae_output_proj_backward: dout[b, o, n, c] is read at dout + b sb + o so + n sn + c sc (element strides >= 0: a strided
 *   window is fine); writes dx (M x D, dense rows; NULL: not wanted), dw and db (shapes of w and bias).  scratch:
 *   regt_stae_output_proj_backward_scratch_floats floats (0: arguments out of range): partial dw | db per chunk of (b, n) pairs.
 * regt_stae_drop_add_layernorm: out = LayerNorm(residual + keep y / (1 - p)) * gamma + beta: regt_stae_add_layernorm with dropout
 *   on the branch y.  keep: (M, D / 32) 32-bit words, row-major, 4-byte aligned; bit j of word w keeps column 32 w + j.  keep ==
 *   NULL: no dropout and no scaling, the bits of regt_stae_add_layernorm.  0 <= p < 1; other limits as regt_stae_add_layernorm.
 * regt_stae_drop_add_layernorm_backward: dz (M x D) = dL/dresidual, dy (M x D) = dL/dy = keep dz / (1 - p), written in the same
 *   pass, dgamma, dbeta.  keep == NULL: regt_stae_add_layernorm_backward (dz is the gradient of y too; dy is not touched and may be
 *   NULL).  dz and dy must not alias an input or each other.  scratch: regt_stae_drop_add_layernorm_backward_scratch_floats floats
 *   (0: arguments out of range).  Limits as regt_stae_add_layernorm_backward; 0 <= p < 1.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t batch, in_steps, num_nodes, in_features, input_dim;
    int32_t input_embedding_dim, tod_embedding_dim, dow_embedding_dim, spatial_embedding_dim, adaptive_embedding_dim;
    int32_t steps_per_day, days_per_week, num_heads, feed_forward_dim, num_layers, out_steps, output_dim, use_mixed_proj;
    float ln_eps;
} regt_stae_dims;
int32_t regt_stae_sizes(const regt_stae_dims* dims, size_t* workspace_floats);
int32_t regt_stae_forward(const regt_stae_dims* dims, const float* x, const float* const* params, float* out, float* workspace,
                          regt_stream_t stream);
int32_t regt_stae_attention(const float* q, const float* k, const float* v, int64_t ld, int32_t batch, int32_t in_steps,
                            int32_t num_nodes, int32_t heads, int32_t axis, float* out, int64_t ldo, regt_stream_t stream);
int32_t regt_stae_add_layernorm(const float* residual, const float* y, const float* gamma, const float* beta, float eps, int64_t rows,
                                int32_t width, float* out, regt_stream_t stream);
int32_t regt_stae_attention_train(const float* q, const float* k, const float* v, int64_t ld, int32_t batch, int32_t in_steps,
                                  int32_t num_nodes, int32_t heads, int32_t axis, float* out, int64_t ldo, float* lse,
                                  regt_stream_t stream);
size_t regt_stae_attention_backward_scratch_floats(int32_t batch, int32_t in_steps, int32_t num_nodes, int32_t heads);
int32_t regt_stae_attention_backward(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* dout,
                                     int64_t ldo, const float* lse, int32_t batch, int32_t in_steps, int32_t num_nodes, int32_t heads,
                                     int32_t axis, float* dq, float* dk, float* dv, int64_t ldg, float* scratch, regt_stream_t stream);
size_t regt_stae_add_layernorm_backward_scratch_floats(int64_t rows, int32_t width);
int32_t regt_stae_add_layernorm_backward(const float* residual, const float* y, const float* gamma, const float* dout, float eps,
                                         int64_t rows, int32_t width, float* dz, float* dgamma, float* dbeta, float* scratch,
                                         regt_stream_t stream);
int32_t regt_stae_embed(const regt_stae_dims* dims, const float* x, const float* const* params, float* out, regt_stream_t stream);
size_t regt_stae_embed_backward_scratch_floats(const regt_stae_dims* dims);
int32_t regt_stae_embed_backward(const regt_stae_dims* dims, const float* x, const float* dx0, float* const* grads, float* scratch,
                                 regt_stream_t stream);
int32_t regt_stae_output_proj(const regt_stae_dims* dims, const float* x, const float* w, const float* bias, float* out,
                              regt_stream_t stream);
size_t regt_stae_output_proj_backward_scratch_floats(const regt_stae_dims* dims);
int32_t regt_stae_output_proj_backward(const regt_stae_dims* dims, const float* x, const float* w, const float* dout, int64_t sb,
                                       int64_t so, int64_t sn, int64_t sc, float* dx, float* dw, float* db, float* scratch,
                                       regt_stream_t stream);
int32_t regt_stae_drop_add_layernorm(const float* residual, const float* y, const uint32_t* keep, float p, const float* gamma,
                                     const float* beta, float eps, int64_t rows, int32_t width, float* out, regt_stream_t stream);
size_t regt_stae_drop_add_layernorm_backward_scratch_floats(int64_t rows, int32_t width);
int32_t regt_stae_drop_add_layernorm_backward(const float* residual, const float* y, const uint32_t* keep, float p, const float* gamma,
                                              const float* dout, float eps, int64_t rows, int32_t width, float* dz, float* dy,
                                              float* dgamma, float* dbeta, float* scratch, regt_stream_t stream);

/* relu's gradient in place: d[i] = 0 where y[i] <= 0, y the relu's output (the head of StackedGRU between two regt_linear calls).
 * 1 <= n < 2^31. */
int32_t regt_relu_backward(const float* y, float* d, int64_t n, regt_stream_t stream);

/* Arithmetic of the dense contractions.  0 (default): fp32 MFMA (v_mfma_f32_32x32x2_f32).  1: every fp32 operand is
 * split exactly into three bf16 pieces and the six leading partial products run on the bf16 MFMA with fp32
 * accumulation -- fp32-level rounding error (dropped terms <= 3 * 2^-24 of a product), ~2x the matrix-pipe rate.
 * Also selectable with REGT_GEMM_MODE=bf16x3 before the first call.  Returns the previous mode. */
int32_t regt_set_gemm_mode(int32_t mode);
/* The current mode, read only (what regt_set_gemm_mode would return, without setting anything). */
int32_t regt_gemm_mode(void);

/* Developer switches (A/B timing and the bit-for-bit comparisons of tests/test_gpu_fused.py): stores the value as the switch
 * normalises it and returns the previous value; -1 for an unknown name.  Host state only (one table, csrc/options.hip); the five
 * switches that name a variable start from it when it is set in the environment at their first use (any non-zero value reads as 1).
 *   "xbf" (REGT_XBF; 0 | 1, default 1): under REGT_GEMM_MODE=bf16, bf16 rows of x / A_hat x / L~ x and the fused forward kernel
 *     where the shape allows; 0 = the three-launch forward on fp32 rows.
 *   "fused_bwd" (REGT_FUSED_BWD; 0 | 1, default 1): the three data-gradient launches of that arithmetic as one kernel.
 *   "fused_rows" (0 | 1 | 2, default 1): the row-owning fused forward where it applies; 0 = the 64-row kernel everywhere, 2 = the
 *     row-owning kernel as two workgroups of four waves (a test form).
 *   "embed_kernel" (0 | 1, default 1): fp32 arithmetic, the regional embedding as its own kernel; 0 = through the general GEMM core.
 *   "spmm_rows" (REGT_SPMM_ROWS; 0 | 1, default 0 -- opt-in, measured slower): the row-block aggregation kernel (CSR entries of a
 *     workgroup's rows held in LDS) instead of the column-panel kernels.
 *   "dgrad1_gen" (REGT_DGRAD1_GEN; 0 | 1, default 1): fp32 arithmetic, the candidate data gradient forms its left operand dhp from
 *     Z, H~, dOH while staging it and its epilogue writes dzp and the attention dots (no separate cell-backward pass); 0 = the two
 *     launches.
 *   "tgcn_collapse" (REGT_TGCN_COLLAPSE; 0 | 1, default 1): regional = 0 (TemporalGCN), fp32 / bf16x3: the gates' linear use of the
 *     activation-free hidden input folded into x and L~ x (gate GEMM at K = 3F, no K = 2C gate data gradient); 0 = uncollapsed.
 * Weight gradients of the bf16-row layout (both operands stored as bf16):
 *   "wgrad_ring" (any depth >= 0, negative = 0; default 6): 16-row half slabs requested ahead through a register ring (4 | 6 | 8);
 *     0 = the one-ahead kernel, same partial sums bit for bit.
 *   "wgrad_tile" (256, anything else = 128; default 256): output rows per tile.
 *   "wgrad_ring256" (4, anything else = 2; default 2): ring depth of the 256-row tile.
 *   "wgrad_pairs" (0 | 1 | 2, anything else = 2; default 2 = on with the ring kernel): the two gradients of each left operand as one
 *     launch.
 *   "wgrad_wave" (0 | 1, default 1): row chunks of those launches sized so that all their workgroups are resident at once (another
 *     summation order over chunk boundaries than 0, the fixed ~128 chunks).  Under the fp32 arithmetic it also selects the
 *     wave-owned kernel (one workgroup per CU, one row chunk per CU) for the 256-column weight gradients of large problems; 0 keeps
 *     the three-workgroup kernel and its chunks.
 *   "wgrad_bnw64" (0 | 1, default 1): fp32 rows, a 33..64-wide right-hand side ([x | L~ x] at F = 32) as one 64-column tile instead
 *     of two of 32 (bit-identical).
 * The first two also exist per call: regt_dims.flags.  Environment only, read at first use: REGT_GEMM_MODE (above), REGT_FP32_CORE=wide,
 * REGT_GEMM_DESC=table, REGT_HIPGRAPH=1|2, REGT_SIDE_STREAM=0, REGT_SPMM_PL=8|16, REGT_FUSED_TRACE=1|2. */
int32_t regt_set_option(const char* name, int32_t value);

/* Developer hook (REGT_FUSED_TRACE=1, tools/fused_trace.py): shader-clock stamps of the last fused forward launch, 8 per 64-row
 * tile (start, tables, h, R / q, Z_0, candidate_0, Z_1, candidate_1), copied to out_host; synchronises the device.  Returns
 * the number of values written, 0 when tracing is off. */
int64_t regt_debug_trace(int64_t* out_host, int64_t capacity);

/* Per-stage timing with HIP events recorded on the launch stream (used by bench.py for the
 * roofline figures).  collect() waits for the recorded events and writes "name count total_ms"
 * lines into buf. */
int32_t regt_profile_enable(int32_t on);
/* Optional (environment REGT_HIPGRAPH=1; =2 for every size): small problems (N*T <= 32768 rows) replay a captured
 * hipGraph from the second call on identical buffers.  Off by default -- not faster at TPIMS size.  out[0..5] = forward {eager, captured, replayed},
 * backward {eager, captured, replayed} call counts. */
int32_t regt_graph_stats(int64_t* out);
int32_t regt_profile_collect(char* buf, size_t buf_bytes);

/* loss = mean((pred - y)^2) over `count` entries with mean taken over `global_count`
 * (run.py:180); writes dpred = dloss/dpred and the scalar loss. */
int32_t regt_mse_loss_grad(const float* pred, const float* y, float* dpred, float* loss_out, int64_t count,
                           int64_t global_count, regt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* REGTGCN_H */
