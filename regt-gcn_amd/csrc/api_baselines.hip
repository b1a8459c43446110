// Entry points of the baselines with their argument checks: SpatialGCN, STNorm, STID, StackedGRU, STAEformer (inference, the op-site
// forward / backward entries of its trainable self-attention layer, and those of whole-model training: embedding, output projection,
// keep-bit dropout folded into add+LayerNorm).
#include "api_internal.h"

using namespace regt;

extern "C" {

size_t regt_spatial_embed_slab_floats(int32_t N, int32_t T, int32_t F) { return T > 255 ? 0 : spatial_slab_floats(N, T, F); }

static int spatial_check_dims(const char* what, int32_t N, int32_t T, int32_t F) {
    REGT_CHECK_ARG(N >= 1, "%s: num_nodes must be >= 1, got %d", what, N);
    REGT_CHECK_ARG(T >= 1 && T <= 255, "%s: periods must be in [1, 255], got %d", what, T);
    REGT_CHECK_ARG(F >= 4 && F <= 64 && F % 4 == 0, "%s: num_features must be a multiple of 4 in [4, 64], got %d", what, F);
    return REGT_OK;
}

int32_t regt_spatial_embed_forward(const float* x, const float* lx, const float* w0, const float* w1, const float* b, const uint32_t* keep,
                                   int32_t N, int32_t T, int32_t F, float* s_out, regt_stream_t st) {
    REGT_CHECK_ARG(x && lx && w0 && w1 && b && s_out, "regt_spatial_embed_forward: NULL pointer");
    if (int rc = spatial_check_dims("regt_spatial_embed_forward", N, T, F)) return rc;
    REGT_CHECK_ARG(al16(x) && al16(lx) && al16(b) && al16(s_out) && (!keep || (reinterpret_cast<uintptr_t>(keep) & 7) == 0),
                   "regt_spatial_embed_forward: x, lx, bias, s_out must be 16-byte aligned, keep 8-byte aligned");
    return launch_spatial_fwd(x, lx, w0, w1, b, keep, N, T, F, s_out, (hipStream_t)st);
}

int32_t regt_spatial_embed_backward(const float* x, const float* lx, const float* w0, const float* w1, const float* b,
                                    const uint32_t* keep, const float* ds, int32_t N, int32_t T, int32_t F, float* dw0, float* dw1,
                                    float* db, float* slab, regt_stream_t st) {
    REGT_CHECK_ARG(x && lx && w0 && w1 && b && ds && dw0 && dw1 && db && slab, "regt_spatial_embed_backward: NULL pointer");
    if (int rc = spatial_check_dims("regt_spatial_embed_backward", N, T, F)) return rc;
    REGT_CHECK_ARG(al16(x) && al16(lx) && al16(ds) && (!keep || (reinterpret_cast<uintptr_t>(keep) & 7) == 0),
                   "regt_spatial_embed_backward: x, lx, ds must be 16-byte aligned, keep 8-byte aligned");
    return launch_spatial_bwd(x, lx, w0, w1, b, keep, ds, N, T, F, dw0, dw1, db, slab, (hipStream_t)st);
}

static int stnorm_check(const char* what, const regt_stnorm_dims* d, regt::StnDims* s) {
    REGT_CHECK_ARG(d != nullptr, "%s: dims is NULL", what);
    REGT_CHECK_ARG(d->num_nodes >= 2, "%s: num_nodes must be >= 2 (SNorm's unbiased variance), got %d", what, d->num_nodes);
    REGT_CHECK_ARG(d->batch >= 1 && d->seq_len >= 1, "%s: batch and seq_len must be >= 1, got %d, %d", what, d->batch, d->seq_len);
    REGT_CHECK_ARG(d->tnorm_group >= 1 && d->batch % d->tnorm_group == 0, "%s: tnorm_group %d must divide batch %d", what,
                   d->tnorm_group, d->batch);
    REGT_CHECK_ARG(d->in_dim >= 1 && d->in_dim <= regt::ST_MAX_CH && d->out_dim >= 1 && d->out_dim <= regt::ST_MAX_CH,
                   "%s: in_dim and out_dim must be in [1, %d], got %d, %d", what, regt::ST_MAX_CH, d->in_dim, d->out_dim);
    REGT_CHECK_ARG(d->blocks >= 1 && d->layers >= 1 && d->layers <= 8 && (long)d->blocks * d->layers <= 64,
                   "%s: need 1 <= layers <= 8 and 1 <= blocks * layers <= 64, got blocks %d layers %d", what, d->blocks, d->layers);
    *s = regt::StnDims{d->num_nodes, d->batch, d->tnorm_group, d->seq_len, d->in_dim, d->out_dim, d->blocks, d->layers,
                       d->tnorm ? 1 : 0, d->snorm ? 1 : 0, d->training ? 1 : 0};
    return REGT_OK;
}

static int stnorm_check_params(const char* what, const regt::StnDims& s, const void* const* p, const void* const* run, bool need_run) {
    REGT_CHECK_ARG(p != nullptr, "%s: parameter table is NULL", what);
    for (int k = 0; k < regt::ST_HEAD_PARAMS; ++k) REGT_CHECK_ARG(p[k] != nullptr, "%s: head entry %d is NULL", what, k);
    for (int i = 0; i < s.blocks * s.layers; ++i) {
        const void* const* q = p + regt::ST_HEAD_PARAMS + regt::ST_LAYER_PARAMS * i;
        for (int k = 0; k < 8; ++k) REGT_CHECK_ARG(q[k] != nullptr, "%s: layer %d entry %d is NULL", what, i, k);
        if (s.tnorm) REGT_CHECK_ARG(q[8] && q[9], "%s: layer %d TNorm gamma / beta is NULL", what, i);
        if (s.snorm) REGT_CHECK_ARG(q[10] && q[11], "%s: layer %d SNorm gamma / beta is NULL", what, i);
        if (s.tnorm && run) REGT_CHECK_ARG(run[2 * i] && run[2 * i + 1], "%s: layer %d running buffers are NULL", what, i);
    }
    if (s.tnorm && need_run) REGT_CHECK_ARG(run != nullptr, "%s: running-buffer table is NULL", what);
    return REGT_OK;
}

int32_t regt_stnorm_sizes(const regt_stnorm_dims* d, size_t* ws, size_t* scratch) {
    regt::StnDims s;
    if (int rc = stnorm_check("regt_stnorm_sizes", d, &s)) return rc;
    REGT_CHECK_ARG(regt::stnorm_sizes(s, ws, scratch), "regt_stnorm_sizes: unsupported dims");
    return REGT_OK;
}

int32_t regt_stnorm_forward(const regt_stnorm_dims* d, const float* x, const float* const* params, float* const* running, float* out,
                            float* ws, regt_stream_t st) {
    regt::StnDims s;
    if (int rc = stnorm_check("regt_stnorm_forward", d, &s)) return rc;
    REGT_CHECK_ARG(x && out && ws, "regt_stnorm_forward: NULL pointer");
    if (int rc = stnorm_check_params("regt_stnorm_forward", s, reinterpret_cast<const void* const*>(params),
                                     reinterpret_cast<const void* const*>(running), true))
        return rc;
    return regt::launch_stnorm_fwd(s, x, params, running, out, ws, (hipStream_t)st);
}

int32_t regt_stnorm_backward(const regt_stnorm_dims* d, const float* x, const float* const* params, float* const* running,
                             const float* dout, float* const* grads, const float* ws, float* scratch, regt_stream_t st) {
    regt::StnDims s;
    if (int rc = stnorm_check("regt_stnorm_backward", d, &s)) return rc;
    REGT_CHECK_ARG(x && dout && grads && ws && scratch, "regt_stnorm_backward: NULL pointer");
    if (int rc = stnorm_check_params("regt_stnorm_backward", s, reinterpret_cast<const void* const*>(params),
                                     reinterpret_cast<const void* const*>(running), true))
        return rc;
    if (int rc = stnorm_check_params("regt_stnorm_backward (grads)", s, reinterpret_cast<const void* const*>(grads), nullptr, false)) return rc;
    return regt::launch_stnorm_bwd(s, x, params, running, dout, grads, ws, scratch, (hipStream_t)st);
}

static int stid_check(const char* what, const regt_stid_dims* d, regt::StidDims* s) {
    REGT_CHECK_ARG(d != nullptr, "%s: dims is NULL", what);
    REGT_CHECK_ARG(d->num_nodes >= 1, "%s: num_nodes must be >= 1, got %d", what, d->num_nodes);
    REGT_CHECK_ARG(d->batch >= 1, "%s: batch must be >= 1, got %d", what, d->batch);
    REGT_CHECK_ARG(d->embed_dim == 32, "%s: embed_dim must be 32, got %d", what, d->embed_dim);
    REGT_CHECK_ARG(d->node_dim == 32, "%s: node_dim must be 32, got %d", what, d->node_dim);
    REGT_CHECK_ARG(d->num_layer >= 1 && d->num_layer <= regt::STID_MAX_LAYERS, "%s: num_layer must be in [1, %d], got %d", what,
                   regt::STID_MAX_LAYERS, d->num_layer);
    REGT_CHECK_ARG(d->input_len >= 1 && d->input_len <= 255, "%s: input_len must be in [1, 255], got %d", what, d->input_len);
    REGT_CHECK_ARG(d->in_features >= 1 && d->in_features <= 256, "%s: in_features must be in [1, 256], got %d", what, d->in_features);
    REGT_CHECK_ARG(d->input_dim >= 1 && d->input_dim <= d->in_features, "%s: input_dim must be in [1, in_features = %d], got %d", what,
                   d->in_features, d->input_dim);
    REGT_CHECK_ARG((long)d->input_dim * d->input_len <= regt::STID_MAX_KIN, "%s: input_dim * input_len must be <= %d, got %d * %d", what,
                   regt::STID_MAX_KIN, d->input_dim, d->input_len);
    REGT_CHECK_ARG(d->output_len >= 1 && d->output_len <= regt::STID_MAX_OUT, "%s: output_len must be in [1, %d], got %d", what,
                   regt::STID_MAX_OUT, d->output_len);
    REGT_CHECK_ARG(d->dropout_p >= 0.f && d->dropout_p < 1.f, "%s: dropout_p must be in [0, 1), got %g", what, (double)d->dropout_p);
    REGT_CHECK_ARG((long)d->batch * d->num_nodes * 64 * (2 * d->num_layer + 1) < (1L << 40), "%s: batch * num_nodes is too large", what);
    *s = regt::StidDims{d->num_nodes, d->batch, d->input_len, d->in_features, d->input_dim, d->embed_dim, d->node_dim, d->num_layer,
                        d->output_len, d->if_node ? 1 : 0, d->dropout_p};
    return REGT_OK;
}

static int stid_check_table(const char* what, const regt::StidDims& s, const void* const* p) {
    REGT_CHECK_ARG(p != nullptr, "%s: table is NULL", what);
    if (s.if_node) REGT_CHECK_ARG(p[0] != nullptr, "%s: entry 0 (node_emb) is NULL", what);
    for (int k = 1; k < 3 + 4 * s.num_layer + 2; ++k) REGT_CHECK_ARG(p[k] != nullptr, "%s: entry %d is NULL", what, k);
    return REGT_OK;
}

int32_t regt_stid_sizes(const regt_stid_dims* d, size_t* ws, size_t* scratch) {
    regt::StidDims s;
    if (int rc = stid_check("regt_stid_sizes", d, &s)) return rc;
    REGT_CHECK_ARG(regt::stid_sizes(s, ws, scratch), "regt_stid_sizes: unsupported dims");
    return REGT_OK;
}

int32_t regt_stid_forward(const regt_stid_dims* d, const float* x, const float* const* params, const uint32_t* keep, float* out, float* ws,
                          regt_stream_t st) {
    regt::StidDims s;
    if (int rc = stid_check("regt_stid_forward", d, &s)) return rc;
    REGT_CHECK_ARG(x && out, "regt_stid_forward: x or out is NULL");
    if (int rc = stid_check_table("regt_stid_forward: params", s, reinterpret_cast<const void* const*>(params))) return rc;
    return regt::launch_stid_fwd(s, x, params, keep, out, ws, (hipStream_t)st);
}

int32_t regt_stid_backward(const regt_stid_dims* d, const float* x, const float* const* params, const uint32_t* keep, const float* dout,
                           float* const* grads, const float* ws, float* scratch, regt_stream_t st) {
    regt::StidDims s;
    if (int rc = stid_check("regt_stid_backward", d, &s)) return rc;
    REGT_CHECK_ARG(x && dout && ws && scratch, "regt_stid_backward: x, dout, workspace or scratch is NULL");
    if (int rc = stid_check_table("regt_stid_backward: params", s, reinterpret_cast<const void* const*>(params))) return rc;
    if (int rc = stid_check_table("regt_stid_backward: grads", s, reinterpret_cast<const void* const*>(grads))) return rc;
    return regt::launch_stid_bwd(s, x, params, keep, dout, grads, ws, scratch, (hipStream_t)st);
}

static int gru_check(const char* what, const regt_gru_dims* d, regt::GruDims* s) {
    REGT_CHECK_ARG(d != nullptr, "%s: dims is NULL", what);
    REGT_CHECK_ARG(d->hidden == regt::GRU_HIDDEN, "%s: hidden must be %d, got %d", what, regt::GRU_HIDDEN, d->hidden);
    REGT_CHECK_ARG(d->input_size >= 1 && d->input_size <= regt::GRU_MAX_INPUT, "%s: input_size must be in [1, %d], got %d", what,
                   regt::GRU_MAX_INPUT, d->input_size);
    REGT_CHECK_ARG(d->seq_len >= 1, "%s: seq_len must be >= 1, got %d", what, d->seq_len);
    REGT_CHECK_ARG(d->rows >= 1, "%s: rows must be >= 1, got %d", what, d->rows);
    REGT_CHECK_ARG((long)d->seq_len * d->rows < (1L << 31) - d->rows, "%s: seq_len * rows must be below 2^31, got %d * %d", what, d->seq_len,
                   d->rows);
    REGT_CHECK_ARG(d->x_stride_seq >= 0 && d->x_stride_row >= 0 && d->x_stride_t >= 0, "%s: x strides must be >= 0", what);
    *s = regt::GruDims{d->seq_len, d->rows, d->input_size, d->hidden, d->training ? 1 : 0, (long)d->x_stride_seq, (long)d->x_stride_row,
                       (long)d->x_stride_t};
    return REGT_OK;
}

int32_t regt_gru_sizes(const regt_gru_dims* d, size_t* ws, size_t* scratch) {
    regt::GruDims s;
    if (int rc = gru_check("regt_gru_sizes", d, &s)) return rc;
    regt::gru_sizes(s, ws, scratch);
    return REGT_OK;
}

int32_t regt_gru_forward(const regt_gru_dims* d, const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                         const float* h0, float* out, float* h_last, float* ws, regt_stream_t st) {
    regt::GruDims s;
    if (int rc = gru_check("regt_gru_forward", d, &s)) return rc;
    REGT_CHECK_ARG(x && w_ih && w_hh && b_ih && b_hh, "regt_gru_forward: x or a weight is NULL");
    REGT_CHECK_ARG(ws != nullptr, "regt_gru_forward: workspace is NULL");
    REGT_CHECK_ARG(out || h_last, "regt_gru_forward: out and h_last are both NULL");
    REGT_CHECK_ARG(((uintptr_t)ws & 15) == 0, "regt_gru_forward: workspace must be 16-byte aligned");
    return regt::launch_gru_fwd(s, x, w_ih, w_hh, b_ih, b_hh, h0, out, h_last, ws, (hipStream_t)st);
}

int32_t regt_gru_backward(const regt_gru_dims* d, const float* x, const float* const* weights, const float* h0, const float* dout,
                          const float* dh_last, float* const* grads, float* dh0, const float* ws, float* scratch, regt_stream_t st) {
    regt::GruDims s;
    if (int rc = gru_check("regt_gru_backward", d, &s)) return rc;
    (void)h0;                                                   // the workspace holds it as step 0's previous state
    REGT_CHECK_ARG(s.training, "regt_gru_backward: dims.training must be 1 (the forward saves nothing otherwise)");
    REGT_CHECK_ARG(x && ws && scratch, "regt_gru_backward: x, workspace or scratch is NULL");
    REGT_CHECK_ARG(weights && grads, "regt_gru_backward: weights or grads table is NULL");
    for (int k = 0; k < 4; ++k) REGT_CHECK_ARG(weights[k] && grads[k], "regt_gru_backward: weights or grads entry %d is NULL", k);
    REGT_CHECK_ARG(dout || dh_last, "regt_gru_backward: dout and dh_last are both NULL");
    REGT_CHECK_ARG((((uintptr_t)ws | (uintptr_t)scratch) & 15) == 0, "regt_gru_backward: workspace and scratch must be 16-byte aligned");
    return regt::launch_gru_bwd(s, x, weights[1], dout, dh_last, grads, dh0, ws, scratch, (hipStream_t)st);
}

static int stae_check(const char* what, const regt_stae_dims* d, regt::StaeDims* s) {
    REGT_CHECK_ARG(d != nullptr, "%s: dims is NULL", what);
    REGT_CHECK_ARG(d->batch >= 1 && d->num_nodes >= 1, "%s: batch and num_nodes must be >= 1, got %d, %d", what, d->batch, d->num_nodes);
    REGT_CHECK_ARG(d->in_steps >= 1 && d->in_steps <= 255, "%s: in_steps must be in [1, 255], got %d", what, d->in_steps);
    REGT_CHECK_ARG(d->use_mixed_proj == 1, "%s: use_mixed_proj must be 1 (the temporal_proj tail is not built)", what);
    REGT_CHECK_ARG(d->input_embedding_dim >= 1 && d->tod_embedding_dim >= 0 && d->dow_embedding_dim >= 0 && d->spatial_embedding_dim >= 0 &&
                       d->adaptive_embedding_dim >= 0,
                   "%s: embedding widths must be >= 0 (input_embedding_dim >= 1)", what);
    const long D = (long)d->input_embedding_dim + d->tod_embedding_dim + d->dow_embedding_dim + d->spatial_embedding_dim + d->adaptive_embedding_dim;
    REGT_CHECK_ARG(D % 32 == 0 && D <= regt::STAE_MAX_DIM, "%s: model_dim (the sum of the five embedding widths) must be a multiple of 32, at most %d, got %ld",
                   what, regt::STAE_MAX_DIM, D);
    REGT_CHECK_ARG(d->num_heads >= 1 && D == (long)d->num_heads * regt::STAE_HEAD_DIM, "%s: head width model_dim / num_heads must be %d, got model_dim %ld, num_heads %d",
                   what, regt::STAE_HEAD_DIM, D, d->num_heads);
    REGT_CHECK_ARG(d->feed_forward_dim >= 32 && d->feed_forward_dim % 32 == 0 && d->feed_forward_dim <= regt::STAE_MAX_FF,
                   "%s: feed_forward_dim must be a multiple of 32 in [32, %d], got %d", what, regt::STAE_MAX_FF, d->feed_forward_dim);
    REGT_CHECK_ARG(d->num_layers >= 1 && d->num_layers <= regt::STAE_MAX_LAYERS, "%s: num_layers must be in [1, %d], got %d", what,
                   regt::STAE_MAX_LAYERS, d->num_layers);
    REGT_CHECK_ARG(d->in_features >= 1 && d->in_features <= 256, "%s: in_features must be in [1, 256], got %d", what, d->in_features);
    REGT_CHECK_ARG(d->input_dim >= 1 && d->input_dim <= d->in_features, "%s: input_dim must be in [1, in_features = %d], got %d", what,
                   d->in_features, d->input_dim);
    REGT_CHECK_ARG((d->tod_embedding_dim == 0 || d->in_features >= 2) && (d->dow_embedding_dim == 0 || d->in_features >= 3),
                   "%s: in_features must cover the time-of-day (1) and day-of-week (2) feature columns, got %d", what, d->in_features);
    REGT_CHECK_ARG(d->steps_per_day >= 1 && d->days_per_week >= 1, "%s: steps_per_day and days_per_week must be >= 1, got %d, %d", what,
                   d->steps_per_day, d->days_per_week);
    REGT_CHECK_ARG(d->out_steps >= 1 && d->output_dim >= 1 && (long)d->out_steps * d->output_dim <= regt::STAE_MAX_OUT,
                   "%s: out_steps * output_dim must be in [1, %d], got %d * %d", what, regt::STAE_MAX_OUT, d->out_steps, d->output_dim);
    REGT_CHECK_ARG(d->ln_eps > 0.f, "%s: ln_eps must be > 0, got %g", what, (double)d->ln_eps);
    REGT_CHECK_ARG((long)d->batch * d->in_steps * d->num_nodes < (1L << 31) / 4, "%s: batch * in_steps * num_nodes is too large", what);
    *s = regt::StaeDims{d->batch, d->in_steps, d->num_nodes, d->in_features, d->input_dim, d->input_embedding_dim, d->tod_embedding_dim,
                        d->dow_embedding_dim, d->spatial_embedding_dim, d->adaptive_embedding_dim, d->steps_per_day, d->days_per_week,
                        d->num_heads, d->feed_forward_dim, d->num_layers, d->out_steps, d->output_dim, d->ln_eps};
    return REGT_OK;
}

// the six embedding entries of a parameter or gradient table (node_emb, adaptive_embedding, input_proj w, b, tod, dow): those of
// width 0 may be NULL
static int stae_embed_table_check(const char* what, const char* kind, const regt::StaeDims& s, const void* const* p) {
    const bool need[6] = {s.e_sp > 0, s.e_adp > 0, true, true, s.e_tod > 0, s.e_dow > 0};
    for (int k = 0; k < 6; ++k) REGT_CHECK_ARG(!need[k] || p[k] != nullptr, "%s: %s entry %d is NULL", what, kind, k);
    return REGT_OK;
}

static int stae_check_table(const char* what, const regt::StaeDims& s, const void* const* p) {
    REGT_CHECK_ARG(p != nullptr, "%s: parameter table is NULL", what);
    if (int rc = stae_embed_table_check(what, "head", s, p)) return rc;
    for (int k = 6; k < regt::STAE_HEAD_PARAMS; ++k) REGT_CHECK_ARG(p[k] != nullptr, "%s: head entry %d is NULL", what, k);
    for (int k = regt::STAE_HEAD_PARAMS; k < regt::STAE_HEAD_PARAMS + 2 * s.num_layers * regt::STAE_LAYER_PARAMS; ++k)
        REGT_CHECK_ARG(p[k] != nullptr, "%s: layer entry %d is NULL", what, k);
    return REGT_OK;
}

// out[M x N] = act(A[M x K] W^T + bias), rows of A / out at lda / ldo
static int stae_linear(const float* A, long lda, long M, int K, const float* W, int N, const float* bias, int act, float* out, long ldo,
                       hipStream_t st) {
    GemmSegs S{};
    S.nseg = 1;
    S.seg[0] = make_seg(A, lda, W, nullptr, K, INT_MAX, K, true);
    S.row_div = 1;
    EpiBiasAct e{out, ldo, bias, act, 0.f};
    return launch_gemm_bias_act(S, M, N, e, st);
}

// The whole inference launch sequence.  Workspace (floats): X and Y (M x D each), Q|K|V (M x 3D), the attention output (M x D) and the
// feed-forward hidden (M x FF).  Per layer: three projections into Q|K|V, attention along the layer's axis, out_proj -> Y,
// X = LN1(X + Y), hidden = relu(X W1^T + b1), Y = hidden W2^T + b2, X = LN2(X + Y).
static int stae_forward(const regt::StaeDims& s, const float* x, const float* const* P, float* out, float* ws, hipStream_t st) {
    const int D = regt::stae_model_dim(s), FF = s.ff_dim;
    const long M = (long)s.batch * s.in_steps * s.num_nodes;
    float *X = ws, *Y = X + M * D, *QKV = Y + M * D, *AO = QKV + 3 * M * D, *Hf = AO + M * D;
    {
        PROF("stae_embed", st);
        TRY(regt::launch_stae_embed(s, x, P, X, st));
    }
    for (int i = 0; i < 2 * s.num_layers; ++i) {
        const float* const* p = P + regt::STAE_HEAD_PARAMS + i * regt::STAE_LAYER_PARAMS;
        const int axis = i < s.num_layers ? 1 : 2;
        {
            PROF("stae_qkv", st);
            for (int j = 0; j < 3; ++j) TRY(stae_linear(X, D, M, D, p[2 * j], D, p[2 * j + 1], ACT_NONE, QKV + j * D, 3 * D, st));
        }
        {
            PROF(axis == 1 ? "stae_attention_t" : "stae_attention_s", st);
            TRY(regt::launch_stae_attention(QKV, QKV + D, QKV + 2 * D, 3 * D, s.batch, s.in_steps, s.num_nodes, s.num_heads, axis, AO, D, st));
        }
        {
            PROF("stae_out_proj", st);
            TRY(stae_linear(AO, D, M, D, p[6], D, p[7], ACT_NONE, Y, D, st));
        }
        {
            PROF("stae_add_layernorm", st);
            TRY(regt::launch_stae_add_layernorm(X, Y, p[12], p[13], s.ln_eps, M, D, X, st));
        }
        {
            PROF("stae_feed_forward", st);
            TRY(stae_linear(X, D, M, D, p[8], FF, p[9], ACT_RELU, Hf, FF, st));
            TRY(stae_linear(Hf, FF, M, FF, p[10], D, p[11], ACT_NONE, Y, D, st));
        }
        {
            PROF("stae_add_layernorm", st);
            TRY(regt::launch_stae_add_layernorm(X, Y, p[14], p[15], s.ln_eps, M, D, X, st));
        }
    }
    PROF("stae_output_proj", st);
    return regt::launch_stae_output_proj(s, X, P[6], P[7], out, st);
}

int32_t regt_stae_sizes(const regt_stae_dims* d, size_t* ws) {
    regt::StaeDims s;
    if (int rc = stae_check("regt_stae_sizes", d, &s)) return rc;
    REGT_CHECK_ARG(ws != nullptr, "regt_stae_sizes: workspace_floats is NULL");
    *ws = (size_t)s.batch * s.in_steps * s.num_nodes * (6 * (size_t)regt::stae_model_dim(s) + s.ff_dim);
    return REGT_OK;
}

int32_t regt_stae_forward(const regt_stae_dims* d, const float* x, const float* const* params, float* out, float* ws, regt_stream_t st) {
    regt::StaeDims s;
    if (int rc = stae_check("regt_stae_forward", d, &s)) return rc;
    REGT_CHECK_ARG(x && out && ws, "regt_stae_forward: x, out or workspace is NULL");
    REGT_CHECK_ARG(al16(ws), "regt_stae_forward: workspace must be 16-byte aligned");
    if (int rc = stae_check_table("regt_stae_forward", s, reinterpret_cast<const void* const*>(params))) return rc;
    return stae_forward(s, x, params, out, ws, (hipStream_t)st);
}

// the shape arguments every attention entry shares
static int stae_attention_check(const char* what, int32_t B, int32_t T, int32_t N, int32_t heads, int32_t axis) {
    REGT_CHECK_ARG(axis == 1 || axis == 2, "%s: axis must be 1 (temporal) or 2 (spatial), got %d", what, axis);
    REGT_CHECK_ARG(B >= 1 && T >= 1 && N >= 1, "%s: batch, in_steps and num_nodes must be >= 1, got %d, %d, %d", what, B, T, N);
    REGT_CHECK_ARG(heads >= 1 && heads * regt::STAE_HEAD_DIM <= regt::STAE_MAX_DIM, "%s: heads must be in [1, %d], got %d", what,
                   regt::STAE_MAX_DIM / regt::STAE_HEAD_DIM, heads);
    REGT_CHECK_ARG((long)B * T * N < (1L << 31) / 4, "%s: batch * in_steps * num_nodes is too large", what);
    return REGT_OK;
}

// every leading dimension (`names`: "ld and ldo", in the backward "ld, ldo and ldg") covers the 32 * heads columns and keeps a
// row's float4s aligned
static int stae_ld_check(const char* what, int32_t heads, const char* names, std::initializer_list<int64_t> lds) {
    const long D = (long)heads * regt::STAE_HEAD_DIM;
    char got[96] = "";
    bool ok = true;
    for (int64_t ld : lds) {
        ok = ok && ld >= D && ld % 4 == 0;
        snprintf(got + strlen(got), sizeof got - strlen(got), "%s%ld", got[0] ? ", " : "", (long)ld);
    }
    REGT_CHECK_ARG(ok, "%s: %s must be multiples of 4, at least 32 * heads = %ld, got %s", what, names, D, got);
    return REGT_OK;
}

int32_t regt_stae_attention(const float* q, const float* k, const float* v, int64_t ld, int32_t B, int32_t T, int32_t N, int32_t heads,
                            int32_t axis, float* out, int64_t ldo, regt_stream_t st) {
    REGT_CHECK_ARG(q && k && v && out, "regt_stae_attention: NULL pointer");
    if (int rc = stae_attention_check("regt_stae_attention", B, T, N, heads, axis)) return rc;
    if (int rc = stae_ld_check("regt_stae_attention", heads, "ld and ldo", {ld, ldo})) return rc;
    REGT_CHECK_ARG(al16(q) && al16(k) && al16(v) && al16(out), "regt_stae_attention: q, k, v and out must be 16-byte aligned");
    return regt::launch_stae_attention(q, k, v, (long)ld, B, T, N, heads, axis, out, (long)ldo, (hipStream_t)st);
}

int32_t regt_stae_attention_train(const float* q, const float* k, const float* v, int64_t ld, int32_t B, int32_t T, int32_t N, int32_t heads,
                                  int32_t axis, float* out, int64_t ldo, float* lse, regt_stream_t st) {
    REGT_CHECK_ARG(q && k && v && out && lse, "regt_stae_attention_train: NULL pointer");
    if (int rc = stae_attention_check("regt_stae_attention_train", B, T, N, heads, axis)) return rc;
    if (int rc = stae_ld_check("regt_stae_attention_train", heads, "ld and ldo", {ld, ldo})) return rc;
    REGT_CHECK_ARG(al16(q) && al16(k) && al16(v) && al16(out) && al16(lse), "regt_stae_attention_train: q, k, v, out and lse must be 16-byte aligned");
    return regt::launch_stae_attention(q, k, v, (long)ld, B, T, N, heads, axis, out, (long)ldo, (hipStream_t)st, lse);
}

size_t regt_stae_attention_backward_scratch_floats(int32_t B, int32_t T, int32_t N, int32_t heads) {
    if (stae_attention_check("regt_stae_attention_backward_scratch_floats", B, T, N, heads, 1)) return 0;
    return regt::stae_attention_bwd_scratch_floats((long)B * T * N, heads);
}

int32_t regt_stae_attention_backward(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* dout,
                                     int64_t ldo, const float* lse, int32_t B, int32_t T, int32_t N, int32_t heads, int32_t axis, float* dq,
                                     float* dk, float* dv, int64_t ldg, float* scratch, regt_stream_t st) {
    REGT_CHECK_ARG(q && k && v && out && dout && lse && dq && dk && dv && scratch, "regt_stae_attention_backward: NULL pointer");
    if (int rc = stae_attention_check("regt_stae_attention_backward", B, T, N, heads, axis)) return rc;
    if (int rc = stae_ld_check("regt_stae_attention_backward", heads, "ld, ldo and ldg", {ld, ldo, ldg})) return rc;
    REGT_CHECK_ARG(al16(q) && al16(k) && al16(v) && al16(out) && al16(dout) && al16(lse) && al16(dq) && al16(dk) && al16(dv) && al16(scratch),
                   "regt_stae_attention_backward: every pointer must be 16-byte aligned");
    return regt::launch_stae_attention_bwd(q, k, v, (long)ld, out, dout, (long)ldo, lse, B, T, N, heads, axis, dq, dk, dv, (long)ldg, scratch,
                                           (hipStream_t)st);
}

// The D, M and eps rules of add+LayerNorm.  The forward entries take M < 2^31 rows, the backward entries a quarter of that; the
// scratch sizes have no eps to check and pass 1.
constexpr long LN_FWD_ROWS = 1L << 31, LN_BWD_ROWS = (1L << 31) / 4;
static int stae_ln_check(const char* what, int64_t M, int32_t D, float eps, long m_bound) {
    REGT_CHECK_ARG(D >= 32 && D % 32 == 0 && D <= regt::STAE_MAX_DIM, "%s: D must be a multiple of 32 in [32, %d], got %d", what,
                   regt::STAE_MAX_DIM, D);
    REGT_CHECK_ARG(M >= 1 && M < m_bound, "%s: M must be in [1, %s), got %ld", what, m_bound == LN_FWD_ROWS ? "2^31" : "2^31 / 4", (long)M);
    REGT_CHECK_ARG(eps > 0.f, "%s: eps must be > 0, got %g", what, (double)eps);
    return REGT_OK;
}

int32_t regt_stae_add_layernorm(const float* residual, const float* y, const float* gamma, const float* beta, float eps, int64_t M, int32_t D,
                                float* out, regt_stream_t st) {
    REGT_CHECK_ARG(residual && y && gamma && beta && out, "regt_stae_add_layernorm: NULL pointer");
    if (int rc = stae_ln_check("regt_stae_add_layernorm", M, D, eps, LN_FWD_ROWS)) return rc;
    return regt::launch_stae_add_layernorm(residual, y, gamma, beta, eps, (long)M, D, out, (hipStream_t)st);
}


size_t regt_stae_add_layernorm_backward_scratch_floats(int64_t M, int32_t D) {
    if (stae_ln_check("regt_stae_add_layernorm_backward_scratch_floats", M, D, 1.f, LN_BWD_ROWS)) return 0;
    return regt::stae_add_layernorm_bwd_scratch_floats((long)M, D);
}

int32_t regt_stae_add_layernorm_backward(const float* residual, const float* y, const float* gamma, const float* dout, float eps, int64_t M,
                                         int32_t D, float* dz, float* dgamma, float* dbeta, float* scratch, regt_stream_t st) {
    REGT_CHECK_ARG(residual && y && gamma && dout && dz && dgamma && dbeta && scratch, "regt_stae_add_layernorm_backward: NULL pointer");
    if (int rc = stae_ln_check("regt_stae_add_layernorm_backward", M, D, eps, LN_BWD_ROWS)) return rc;
    REGT_CHECK_ARG(al16(residual) && al16(y) && al16(gamma) && al16(dout) && al16(dz) && al16(dgamma) && al16(dbeta) && al16(scratch),
                   "regt_stae_add_layernorm_backward: every pointer must be 16-byte aligned");
    REGT_CHECK_ARG(dz != residual && dz != y && dz != dout, "regt_stae_add_layernorm_backward: dz must not alias residual, y or dout");
    return regt::launch_stae_add_layernorm_bwd(residual, y, gamma, dout, eps, (long)M, D, dz, dgamma, dbeta, scratch, (hipStream_t)st);
}

// ---- whole-model training: the embedding, the output projection and keep-bit dropout folded into add+LayerNorm ----------------------

int32_t regt_stae_embed(const regt_stae_dims* d, const float* x, const float* const* params, float* out, regt_stream_t st) {
    regt::StaeDims s;
    if (int rc = stae_check("regt_stae_embed", d, &s)) return rc;
    REGT_CHECK_ARG(x && out && params, "regt_stae_embed: x, out or the parameter table is NULL");
    if (int rc = stae_embed_table_check("regt_stae_embed", "head", s, reinterpret_cast<const void* const*>(params))) return rc;
    return regt::launch_stae_embed(s, x, params, out, (hipStream_t)st);
}

size_t regt_stae_embed_backward_scratch_floats(const regt_stae_dims* d) {
    regt::StaeDims s;
    if (stae_check("regt_stae_embed_backward_scratch_floats", d, &s)) return 0;
    if (regt::stae_embed_bwd_partial_floats(s) > regt::STAE_EMBED_BWD_MAX_LDS) {
        regt::set_error("regt_stae_embed_backward_scratch_floats: the input projection and the two tables exceed %d floats",
                        regt::STAE_EMBED_BWD_MAX_LDS);
        return 0;
    }
    return regt::stae_embed_bwd_scratch_floats(s);
}

int32_t regt_stae_embed_backward(const regt_stae_dims* d, const float* x, const float* dx0, float* const* grads, float* scratch,
                                 regt_stream_t st) {
    regt::StaeDims s;
    if (int rc = stae_check("regt_stae_embed_backward", d, &s)) return rc;
    REGT_CHECK_ARG(x && dx0 && grads && scratch, "regt_stae_embed_backward: x, dx0, the gradient table or scratch is NULL");
    if (int rc = stae_embed_table_check("regt_stae_embed_backward", "gradient", s, reinterpret_cast<const void* const*>(grads))) return rc;
    return regt::launch_stae_embed_bwd(s, x, dx0, grads, scratch, (hipStream_t)st);
}

int32_t regt_stae_output_proj(const regt_stae_dims* d, const float* x, const float* w, const float* bias, float* out, regt_stream_t st) {
    regt::StaeDims s;
    if (int rc = stae_check("regt_stae_output_proj", d, &s)) return rc;
    REGT_CHECK_ARG(x && w && bias && out, "regt_stae_output_proj: NULL pointer");
    return regt::launch_stae_output_proj(s, x, w, bias, out, (hipStream_t)st);
}

size_t regt_stae_output_proj_backward_scratch_floats(const regt_stae_dims* d) {
    regt::StaeDims s;
    if (stae_check("regt_stae_output_proj_backward_scratch_floats", d, &s)) return 0;
    return regt::stae_output_proj_bwd_scratch_floats(s);
}

int32_t regt_stae_output_proj_backward(const regt_stae_dims* d, const float* x, const float* w, const float* dout, int64_t sb, int64_t so,
                                       int64_t sn, int64_t sc, float* dx, float* dw, float* db, float* scratch, regt_stream_t st) {
    regt::StaeDims s;
    if (int rc = stae_check("regt_stae_output_proj_backward", d, &s)) return rc;
    REGT_CHECK_ARG(x && w && dout && dw && db && scratch, "regt_stae_output_proj_backward: NULL pointer (only dx may be NULL)");
    REGT_CHECK_ARG(sb >= 0 && so >= 0 && sn >= 0 && sc >= 0, "regt_stae_output_proj_backward: dout strides must be >= 0, got %ld, %ld, %ld, %ld",
                   (long)sb, (long)so, (long)sn, (long)sc);
    REGT_CHECK_ARG(dx != x, "regt_stae_output_proj_backward: dx must not alias x");
    return regt::launch_stae_output_proj_bwd(s, x, w, dout, (long)sb, (long)so, (long)sn, (long)sc, dx, dw, db, scratch, (hipStream_t)st);
}

static int stae_drop_check(const char* what, const void* keep, float p) {
    REGT_CHECK_ARG(p >= 0.f && p < 1.f, "%s: p must be in [0, 1), got %g", what, (double)p);
    REGT_CHECK_ARG((reinterpret_cast<uintptr_t>(keep) & 3) == 0, "%s: keep must be 4-byte aligned", what);
    return REGT_OK;
}

int32_t regt_stae_drop_add_layernorm(const float* residual, const float* y, const uint32_t* keep, float p, const float* gamma,
                                     const float* beta, float eps, int64_t M, int32_t D, float* out, regt_stream_t st) {
    if (int rc = stae_drop_check("regt_stae_drop_add_layernorm", keep, p)) return rc;
    if (!keep) return regt_stae_add_layernorm(residual, y, gamma, beta, eps, M, D, out, st);
    REGT_CHECK_ARG(residual && y && gamma && beta && out, "regt_stae_drop_add_layernorm: NULL pointer");
    if (int rc = stae_ln_check("regt_stae_drop_add_layernorm", M, D, eps, LN_FWD_ROWS)) return rc;
    return regt::launch_stae_drop_add_layernorm(residual, y, keep, 1.0f / (1.0f - p), gamma, beta, eps, (long)M, D, out, (hipStream_t)st);
}

size_t regt_stae_drop_add_layernorm_backward_scratch_floats(int64_t M, int32_t D) {
    if (stae_ln_check("regt_stae_drop_add_layernorm_backward_scratch_floats", M, D, 1.f, LN_BWD_ROWS)) return 0;
    return regt::stae_add_layernorm_bwd_scratch_floats((long)M, D);
}

int32_t regt_stae_drop_add_layernorm_backward(const float* residual, const float* y, const uint32_t* keep, float p, const float* gamma,
                                              const float* dout, float eps, int64_t M, int32_t D, float* dz, float* dy, float* dgamma,
                                              float* dbeta, float* scratch, regt_stream_t st) {
    if (int rc = stae_drop_check("regt_stae_drop_add_layernorm_backward", keep, p)) return rc;
    if (!keep) return regt_stae_add_layernorm_backward(residual, y, gamma, dout, eps, M, D, dz, dgamma, dbeta, scratch, st);
    REGT_CHECK_ARG(residual && y && gamma && dout && dz && dy && dgamma && dbeta && scratch, "regt_stae_drop_add_layernorm_backward: NULL pointer");
    if (int rc = stae_ln_check("regt_stae_drop_add_layernorm_backward", M, D, eps, LN_BWD_ROWS)) return rc;
    REGT_CHECK_ARG(al16(residual) && al16(y) && al16(gamma) && al16(dout) && al16(dz) && al16(dy) && al16(dgamma) && al16(dbeta) && al16(scratch),
                   "regt_stae_drop_add_layernorm_backward: every float pointer must be 16-byte aligned");
    REGT_CHECK_ARG(dz != residual && dz != y && dz != dout && dy != residual && dy != y && dy != dout && dy != dz,
                   "regt_stae_drop_add_layernorm_backward: dz and dy must not alias an input or each other");
    return regt::launch_stae_add_layernorm_bwd(residual, y, gamma, dout, eps, (long)M, D, dz, dgamma, dbeta, scratch, (hipStream_t)st, keep,
                                               1.0f / (1.0f - p), dy);
}

}  // extern "C"
