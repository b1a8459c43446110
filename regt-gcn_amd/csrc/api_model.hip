// Entry points of the RegT-GCN / TemporalGCN step: checks, layout and format of the call, then api_step.hip eagerly or as a captured graph.
#include "api_internal.h"

namespace regt { namespace {

// q crosses from regt_forward to regt_backward: remember per workspace how the forward stored it, so that a mode change in
// between is caught instead of misread.
std::mutex g_qfmt_mu;
std::unordered_map<const void*, int> g_qfmt;
void note_q_format(const void* ws, int bf16) {
    std::lock_guard<std::mutex> lk(g_qfmt_mu);
    if (g_qfmt.size() > 4096) g_qfmt.clear();
    g_qfmt[ws] = bf16;
}
int q_format(const void* ws) {
    std::lock_guard<std::mutex> lk(g_qfmt_mu);
    auto it = g_qfmt.find(ws);
    return it == g_qfmt.end() ? 0 : it->second;
}

int check_ptrs(const regt_params* p, const regt_dims& d, bool cell_only = false) {
    REGT_CHECK_ARG(p != nullptr, "params is NULL");
    bool ok = p->attention && p->head1_w && p->head1_b && p->head2_w && p->head2_b;
    if (!cell_only) ok = ok && p->cheb_w0 && p->cheb_w1 && p->cheb_bias;
    for (int k = 0; k < 3; ++k) ok = ok && p->conv_lin_w[k] && p->conv_bias[k] && p->gate_w[k] && p->gate_b[k];
    if (d.regional && !cell_only) ok = ok && p->region_w && p->region_b;
    REGT_CHECK_ARG(ok, "params: a required tensor pointer is NULL");
    return REGT_OK;
}

}}  // namespace regt::(anonymous)

using namespace regt;

extern "C" {

static int32_t forward_common(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const float* x,
                              const float* xp_ext, int32_t x_rows, float* pred, float* hidden, void* ws, size_t ws_bytes,
                              regt_stream_t st, bool xp_is_bf16 = false) {
    TRY(check_dims(dims));
    CallScope call(dims);
    REGT_CHECK_ARG(graph && graph->rowptr && graph->col && graph->val && (graph->node_region || graph->overlap), "regt_forward: graph incomplete");
    TRY(check_ptrs(params, *dims));
    const bool no_head = (dims->flags & REGT_DIMS_NO_HEAD) != 0;
    REGT_CHECK_ARG(!no_head || !xp_ext, "regt_forward_packed: REGT_DIMS_NO_HEAD is for regt_forward / regt_backward");
    REGT_CHECK_ARG((x || xp_ext) && (pred || no_head) && hidden && ws, "regt_forward: NULL pointer");
    REGT_CHECK_ARG(al16(x) && al16(xp_ext) && al16(hidden) && al16(ws),
                   "regt_forward: x, hidden and workspace must be 16-byte aligned");
    REGT_CHECK_ARG(!xp_ext || x_rows >= dims->N, "regt_forward_packed: x_rows=%d < N=%d", x_rows, dims->N);
    hipStream_t hs = (hipStream_t)st;
    int fmt = forward_format(*dims, *graph, xp_ext ? x_rows : dims->N, xp_ext && !xp_is_bf16, xp_is_bf16);
    REGT_CHECK_ARG(!xp_is_bf16 || (fmt & FMT_XBF), "regt_forward_packed_bf16: bf16 input rows need REGT_GEMM_MODE=bf16 and a shape the fused "
                   "forward covers (C = 256, F = 64, node-disjoint regions, merged operator)");
    Layout L;
    if (dims->flags & REGT_DIMS_FORWARD_ONLY) {
        L = forward_only_layout(*dims, *graph, xp_ext != nullptr, x_rows, xp_is_bf16, (char*)ws, &fmt);
        REGT_CHECK_ARG(ws_bytes >= L.bytes, "regt_forward (REGT_DIMS_FORWARD_ONLY): workspace %zu < required %zu bytes (%s)", ws_bytes, L.bytes,
                       xp_ext ? "regt_forward_only_packed_workspace_bytes" : "regt_forward_only_workspace_bytes");
        fmt |= FMT_FWDONLY;
    } else {
        L = make_layout(*dims, graph->n_chunks, graph->overlap, (char*)ws);
        REGT_CHECK_ARG(ws_bytes >= L.bytes, "regt_forward: workspace %zu < required %zu bytes", ws_bytes, L.bytes);
    }
    note_q_format(ws, fmt | (xp_ext ? FMT_PACKED : 0));
    if (!graphs_wanted((long)dims->N * dims->T))
        return forward_impl(*dims, *graph, *params, x, xp_ext, x_rows, pred, hidden, L, hs, false, nullptr, fmt);
    // the snapshot changes every step: pack it with a plain launch, replay everything behind it
    if (!xp_ext) {
        if (fmt & FMT_XBF) TRY(launch_pack_x_bf16(x, L.Xp, dims->N, dims->F, dims->T, hs));
        else TRY(launch_pack_x(x, L.Xp, dims->N, dims->F, dims->T, hs));
    } else if ((fmt & FMT_XBF) && !(fmt & FMT_XCALLER)) {
        TRY(launch_cvt_rows_bf16(xp_ext, L.Xp, (long)x_rows * dims->T * dims->F, hs));
    }
    unsigned long long key = hash_bytes(dims, sizeof(*dims), 0xcbf29ce484222325ull);
    key = hash_bytes(graph, sizeof(*graph), key);
    key = hash_bytes(params, sizeof(*params), key);
    const void* ptrs[6] = {xp_ext, pred, hidden, ws, (const void*)(long)x_rows, (const void*)(long)fmt};
    key = hash_bytes(ptrs, sizeof(ptrs), key);
    const regt_dims dd = *dims; const regt_graph gg = *graph; const regt_params pp = *params;
    return run_maybe_graphed(g_fwd_graphs, key, hs, [=](hipStream_t s) {
        return forward_impl(dd, gg, pp, x, xp_ext, x_rows, pred, hidden, L, s, /*skip_pack=*/true, nullptr, fmt);
    });
}

int32_t regt_forward(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const float* x, float* pred,
                     float* hidden, void* ws, size_t ws_bytes, regt_stream_t st) {
    REGT_CHECK_ARG(x != nullptr, "regt_forward: x is NULL");
    return forward_common(dims, graph, params, x, nullptr, 0, pred, hidden, ws, ws_bytes, st);
}

int32_t regt_forward_packed(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const float* x_packed,
                            int32_t x_rows, float* pred, float* hidden, void* ws, size_t ws_bytes, regt_stream_t st) {
    REGT_CHECK_ARG(x_packed != nullptr, "regt_forward_packed: x_packed is NULL");
    return forward_common(dims, graph, params, nullptr, x_packed, x_rows, pred, hidden, ws, ws_bytes, st);
}

int32_t regt_forward_packed_bf16(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const void* x_packed_bf16,
                                 int32_t x_rows, float* pred, float* hidden, void* ws, size_t ws_bytes, regt_stream_t st) {
    REGT_CHECK_ARG(x_packed_bf16 != nullptr, "regt_forward_packed_bf16: x_packed is NULL");
    return forward_common(dims, graph, params, nullptr, static_cast<const float*>(x_packed_bf16), x_rows, pred, hidden, ws, ws_bytes, st, true);
}

int32_t regt_backward(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const regt_grads* grads,
                      const float* dpred, const float* dhidden, const float* hidden, const float* x_packed, void* ws,
                      size_t ws_bytes, regt_stream_t st) {
    TRY(check_dims(dims));
    CallScope call(dims);
    REGT_CHECK_ARG(graph && graph->rowptr && (graph->node_region || graph->overlap), "regt_backward: graph incomplete");
    TRY(check_ptrs(params, *dims));
    const bool no_head = (dims->flags & REGT_DIMS_NO_HEAD) != 0;
    REGT_CHECK_ARG(grads && (dpred || no_head) && hidden && ws, "regt_backward: NULL pointer");
    REGT_CHECK_ARG(!no_head || (dhidden && al16(dhidden)), "regt_backward (REGT_DIMS_NO_HEAD): dhidden is the whole upstream gradient: it must be "
                   "given, 16-byte aligned");
    REGT_CHECK_ARG(!no_head || !x_packed, "regt_backward: REGT_DIMS_NO_HEAD does not combine with a packed input");
    {
        const regt_grads& g = *grads;
        bool ok = g.cheb_w0 && g.cheb_w1 && g.cheb_bias && (no_head || (g.head1_w && g.head1_b && g.head2_w && g.head2_b));
        for (int k = 0; k < 3; ++k) ok = ok && g.conv_lin_w[k] && g.conv_bias[k] && g.gate_w[k] && g.gate_b[k];
        if (dims->regional) ok = ok && g.region_w && g.region_b;
        REGT_CHECK_ARG(ok, "regt_backward: a required gradient pointer is NULL (only `attention` may be NULL)");
    }
    const int qbf = q_format(ws);
    REGT_CHECK_ARG(!(qbf & FMT_FWDONLY), "regt_backward: the last forward on this workspace ran with REGT_DIMS_FORWARD_ONLY and kept no activations; "
                   "run the forward without that flag on a workspace of regt_workspace_bytes");
    Layout L = make_layout(*dims, graph->n_chunks, graph->overlap, (char*)ws);
    REGT_CHECK_ARG(ws_bytes >= L.bytes, "regt_backward: workspace %zu < required %zu bytes", ws_bytes, L.bytes);
    hipStream_t hs = (hipStream_t)st;
    REGT_CHECK_ARG((qbf & FMT_QBF) == (bf16_intermediates(*dims) ? 1 : 0),
                   "regt_backward: the GEMM arithmetic changed since the forward on this workspace (another regt_dims.arith, or regt_set_gemm_mode between forward and backward)");
    REGT_CHECK_ARG(!(qbf & FMT_XCALLER) || x_packed, "regt_backward: the forward ran on the caller's bf16 packed input; pass the same buffer as x_packed");
    if (!graphs_wanted((long)dims->N * dims->T))
        return backward_impl(*dims, *graph, *params, *grads, dpred, dhidden, hidden, x_packed, L, hs, qbf);
    unsigned long long key = hash_bytes(dims, sizeof(*dims), 0x84222325cbf29ce4ull);
    key = hash_bytes(graph, sizeof(*graph), key);
    key = hash_bytes(params, sizeof(*params), key);
    key = hash_bytes(grads, sizeof(*grads), key);
    const void* ptrs[6] = {dpred, dhidden, hidden, x_packed, ws, (const void*)(long)qbf};
    key = hash_bytes(ptrs, sizeof(ptrs), key);
    const regt_dims dd = *dims; const regt_graph gg = *graph; const regt_params pp = *params; const regt_grads gr = *grads;
    return run_maybe_graphed(g_bwd_graphs, key, hs, [=](hipStream_t s) {
        return backward_impl(dd, gg, pp, gr, dpred, dhidden, hidden, x_packed, L, s, qbf);
    });
}

/* ---- TGCN cell + attention + head on a caller-supplied hidden input (regtgcn.h) --------------------------------- */
int32_t regt_cell_forward(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const float* x,
                          const float* h_in, float* pred, float* hidden, void* ws, size_t ws_bytes, regt_stream_t st) {
    TRY(check_dims(dims));
    CallScope call(dims);
    REGT_CHECK_ARG(dims->regional == 0, "regt_cell_forward: dims.regional must be 0");
    REGT_CHECK_ARG(!(dims->flags & REGT_DIMS_NO_HEAD), "regt_cell_forward: REGT_DIMS_NO_HEAD is for regt_forward / regt_backward");
    REGT_CHECK_ARG(graph && graph->rowptr && graph->col && graph->val && !graph->overlap, "regt_cell_forward: graph incomplete");
    TRY(check_ptrs(params, *dims, true));
    REGT_CHECK_ARG(x && h_in && pred && hidden && ws, "regt_cell_forward: NULL pointer");
    REGT_CHECK_ARG(al16(x) && al16(h_in) && al16(hidden) && al16(ws), "regt_cell_forward: x, h_in, hidden and workspace must be 16-byte aligned");
    int fmt = bf16_intermediates(*dims) ? FMT_QBF : 0;
    Layout L;
    if (dims->flags & REGT_DIMS_FORWARD_ONLY) {
        L = make_layout_fwd(*dims, 0, false, dims->N, (char*)ws);
        REGT_CHECK_ARG(ws_bytes >= L.bytes, "regt_cell_forward (REGT_DIMS_FORWARD_ONLY): workspace %zu < required %zu bytes (regt_forward_only_workspace_bytes)",
                       ws_bytes, L.bytes);
        fmt |= FMT_FWDONLY;
    } else {
        L = make_layout(*dims, 0, 0, (char*)ws);
        REGT_CHECK_ARG(ws_bytes >= L.bytes, "regt_cell_forward: workspace %zu < required %zu bytes", ws_bytes, L.bytes);
    }
    note_q_format(ws, fmt);
    return forward_impl(*dims, *graph, *params, x, nullptr, 0, pred, hidden, L, (hipStream_t)st, false, h_in, fmt);
}

int32_t regt_cell_backward(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const regt_grads* grads,
                           const float* dpred, const float* dhidden, const float* hidden, const float* h_in, float* dh_in,
                           void* ws, size_t ws_bytes, regt_stream_t st) {
    TRY(check_dims(dims));
    CallScope call(dims);
    REGT_CHECK_ARG(dims->regional == 0, "regt_cell_backward: dims.regional must be 0");
    REGT_CHECK_ARG(!(dims->flags & REGT_DIMS_NO_HEAD), "regt_cell_backward: REGT_DIMS_NO_HEAD is for regt_forward / regt_backward");
    REGT_CHECK_ARG(graph && graph->rowptr && !graph->overlap, "regt_cell_backward: graph incomplete");
    TRY(check_ptrs(params, *dims, true));
    REGT_CHECK_ARG(grads && dpred && hidden && h_in && dh_in && ws, "regt_cell_backward: NULL pointer");
    REGT_CHECK_ARG(al16(h_in) && al16(dh_in), "regt_cell_backward: h_in and dh_in must be 16-byte aligned");
    {
        const regt_grads& g = *grads;
        bool ok = g.head1_w && g.head1_b && g.head2_w && g.head2_b;
        for (int k = 0; k < 3; ++k) ok = ok && g.conv_lin_w[k] && g.conv_bias[k] && g.gate_w[k] && g.gate_b[k];
        REGT_CHECK_ARG(ok, "regt_cell_backward: a required gradient pointer is NULL (only `attention` may be NULL)");
    }
    const int qbf = q_format(ws);
    REGT_CHECK_ARG(!(qbf & FMT_FWDONLY), "regt_cell_backward: the last forward on this workspace ran with REGT_DIMS_FORWARD_ONLY and kept no activations; "
                   "run the forward without that flag on a workspace of regt_workspace_bytes");
    Layout L = make_layout(*dims, 0, 0, (char*)ws);
    REGT_CHECK_ARG(ws_bytes >= L.bytes, "regt_cell_backward: workspace %zu < required %zu bytes", ws_bytes, L.bytes);
    REGT_CHECK_ARG((qbf & FMT_QBF) == (bf16_intermediates(*dims) ? 1 : 0),
                   "regt_cell_backward: the GEMM arithmetic changed since the forward on this workspace");
    return backward_impl(*dims, *graph, *params, *grads, dpred, dhidden, hidden, nullptr, L, (hipStream_t)st, qbf, h_in, dh_in);
}

/* ---- one TGCN cell step, no attention, no head, differentiable in x and H (regtgcn.h) ---------------------------- */
namespace {
// The step's own layout (training or forward-only) followed by what the cell-only calls add: the one attention logit whose softmax is
// exactly 1, the zero hidden input of a call without h_in, and dAx (N, F) of the backward.
struct TgcnLayout { Layout L; float *logit, *h0, *dAx; size_t bytes; };
TgcnLayout tgcn_layout(const regt_dims& d, bool fwd_only, char* base) {
    TgcnLayout t{};
    t.L = fwd_only ? make_layout_fwd(d, 0, false, d.N, base) : make_layout(d, 0, 0, base);
    size_t off = t.L.bytes;
    auto take = [&](size_t nbytes) {
        float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += (nbytes + 255) & ~(size_t)255;
        return p;
    };
    t.logit = take(4);
    t.h0 = take((size_t)d.N * d.C * 4);
    if (!fwd_only) t.dAx = take((size_t)d.N * d.F * 4);
    t.bytes = off;
    return t;
}
// the caller's dims as the step pipeline takes them: T = 1, no head (R, O, H1 are ignored: any positive value sizes the same arithmetic)
int tgcn_dims(const regt_dims* dims, const char* what, regt_dims* out) {
    REGT_CHECK_ARG(dims != nullptr, "%s: dims is NULL", what);
    regt_dims d = *dims;
    d.R = 1; d.O = 1; d.H1 = 4;
    TRY(check_dims(&d));
    REGT_CHECK_ARG(d.T == 1, "%s: dims.T=%d must be 1 (one cell step)", what, d.T);
    REGT_CHECK_ARG(d.regional == 0, "%s: dims.regional must be 0", what);
    d.flags |= REGT_DIMS_NO_HEAD;
    *out = d;
    return REGT_OK;
}
// (inside a CallScope: gemm_mode() is this call's arithmetic)
int tgcn_refuse_bf16(const char* what) {
    REGT_CHECK_ARG(gemm_mode() != 2, "%s: the bf16 arithmetic is not covered (fp32 and bf16x3 are); pass dims.arith = REGT_ARITH_FP32 or "
                   "REGT_ARITH_BF16X3", what);
    return REGT_OK;
}
int tgcn_check_params(const regt_params* p, const char* what) {
    REGT_CHECK_ARG(p != nullptr, "%s: params is NULL", what);
    bool ok = true;
    for (int k = 0; k < 3; ++k) ok = ok && p->conv_lin_w[k] && p->conv_bias[k] && p->gate_w[k] && p->gate_b[k];
    REGT_CHECK_ARG(ok, "%s: params: conv_lin_w, conv_bias, gate_w and gate_b must all be given", what);
    return REGT_OK;
}
}  // namespace

size_t regt_tgcn_workspace_bytes(const regt_dims* dims) {
    regt_dims d;
    if (tgcn_dims(dims, "regt_tgcn_workspace_bytes", &d)) return 0;
    CallScope call(&d);
    if (tgcn_refuse_bf16("regt_tgcn_workspace_bytes")) return 0;
    return tgcn_layout(d, (d.flags & REGT_DIMS_FORWARD_ONLY) != 0, nullptr).bytes;
}

int32_t regt_tgcn_forward(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const float* x, const float* h_in,
                          float* h_out, void* ws, size_t ws_bytes, regt_stream_t st) {
    regt_dims d;
    TRY(tgcn_dims(dims, "regt_tgcn_forward", &d));
    CallScope call(&d);
    TRY(tgcn_refuse_bf16("regt_tgcn_forward"));
    REGT_CHECK_ARG(graph && graph->rowptr && graph->col && graph->val && !graph->overlap, "regt_tgcn_forward: graph incomplete");
    TRY(tgcn_check_params(params, "regt_tgcn_forward"));
    REGT_CHECK_ARG(x && h_out && ws, "regt_tgcn_forward: NULL pointer");
    REGT_CHECK_ARG(al16(x) && al16(h_in) && al16(h_out) && al16(ws), "regt_tgcn_forward: x, h_in, h_out and workspace must be 16-byte aligned");
    const bool fwd_only = (d.flags & REGT_DIMS_FORWARD_ONLY) != 0;
    const TgcnLayout t = tgcn_layout(d, fwd_only, (char*)ws);
    REGT_CHECK_ARG(ws_bytes >= t.bytes, "regt_tgcn_forward: workspace %zu < required %zu bytes (regt_tgcn_workspace_bytes)", ws_bytes, t.bytes);
    note_q_format(ws, fwd_only ? FMT_FWDONLY : 0);
    hipStream_t hs = (hipStream_t)st;
    TRY(launch_zero_f32(t.logit, 1, hs));            // softmax of one logit: probability exactly 1
    if (!h_in) TRY(launch_zero_f32(t.h0, (long)d.N * d.C, hs));
    regt_params p = *params;
    p.attention = t.logit;
    return forward_impl(d, *graph, p, x, nullptr, 0, nullptr, h_out, t.L, hs, false, h_in ? h_in : t.h0, fwd_only ? FMT_FWDONLY : 0);
}

int32_t regt_tgcn_backward(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const regt_grads* grads,
                           const float* dh_out, const float* h_in, const float* h_out, const int32_t* t_rowptr, const int32_t* t_col,
                           const float* t_val, float* dx, float* dh_in, void* ws, size_t ws_bytes, regt_stream_t st) {
    regt_dims d;
    TRY(tgcn_dims(dims, "regt_tgcn_backward", &d));
    CallScope call(&d);
    TRY(tgcn_refuse_bf16("regt_tgcn_backward"));
    REGT_CHECK_ARG(!(d.flags & REGT_DIMS_FORWARD_ONLY), "regt_tgcn_backward: REGT_DIMS_FORWARD_ONLY is for the forward");
    REGT_CHECK_ARG(graph && graph->rowptr && !graph->overlap, "regt_tgcn_backward: graph incomplete");
    TRY(tgcn_check_params(params, "regt_tgcn_backward"));
    REGT_CHECK_ARG(grads && dh_out && h_out && ws, "regt_tgcn_backward: NULL pointer");
    {
        bool ok = true;
        for (int k = 0; k < 3; ++k) ok = ok && grads->conv_lin_w[k] && grads->conv_bias[k] && grads->gate_w[k] && grads->gate_b[k];
        REGT_CHECK_ARG(ok, "regt_tgcn_backward: grads: conv_lin_w, conv_bias, gate_w and gate_b must all be given");
    }
    REGT_CHECK_ARG(!dx || (t_rowptr && t_col && t_val), "regt_tgcn_backward: dx needs the transposed operator (t_rowptr, t_col, t_val)");
    REGT_CHECK_ARG(!dx || d.F <= 64, "regt_tgcn_backward: dx covers F <= 64 (F=%d)", d.F);
    REGT_CHECK_ARG(al16(dx) && al16(dh_in) && al16(h_out) && al16(h_in) && al16(dh_out) && al16(ws),
                   "regt_tgcn_backward: dx, dh_in, h_out, h_in, dh_out and workspace must be 16-byte aligned");
    const int fmt = q_format(ws);
    REGT_CHECK_ARG(!(fmt & FMT_FWDONLY), "regt_tgcn_backward: the last forward on this workspace ran with REGT_DIMS_FORWARD_ONLY and kept no "
                   "activations; run the forward without that flag on a workspace of regt_tgcn_workspace_bytes");
    const TgcnLayout t = tgcn_layout(d, false, (char*)ws);
    REGT_CHECK_ARG(ws_bytes >= t.bytes, "regt_tgcn_backward: workspace %zu < required %zu bytes (regt_tgcn_workspace_bytes)", ws_bytes, t.bytes);
    hipStream_t hs = (hipStream_t)st;
    regt_params p = *params;
    p.attention = t.logit;
    regt_grads g = *grads;
    g.attention = nullptr;                           // the logit is no parameter: its gradient is not formed
    // (h_in == NULL: the forward's zero hidden input is still in the workspace; dh_in == NULL: the data gradients still need the array)
    TRY(backward_impl(d, *graph, p, g, nullptr, dh_out, h_out, nullptr, t.L, hs, fmt, h_in ? h_in : t.h0, dh_in ? dh_in : t.L.dh));
    if (!dx) return REGT_OK;
    {
        PROF("cell_dx", hs);
        TRY(launch_cell_dx(t.L.dzr, t.L.dhp, t.L.Gzr, t.L.Gh, t.dAx, d.N, d.C, d.F, hs));
    }
    PROF("spmm_dx", hs);
    return launch_spmm_csr(t_rowptr, t_col, t_val, t.dAx, dx, d.N, d.N, d.F, 1, hs);
}

/* ---- whole-model input gradient dL/dx behind regt_backward (regtgcn.h) ------------------------------------------------- */
namespace {
// the call's own scratch: dAX, dXd, dLX, (M, F) each -- the step's workspace layout is not touched
struct InputGradLayout { float *dAX, *dXd, *dLX; size_t bytes; };
InputGradLayout input_grad_layout(const regt_dims& d, char* base) {
    InputGradLayout s{};
    const size_t piece = ((size_t)d.N * d.T * d.F * 4 + 255) & ~(size_t)255;
    s.dAX = base ? reinterpret_cast<float*>(base) : nullptr;
    s.dXd = base ? reinterpret_cast<float*>(base + piece) : nullptr;
    s.dLX = base ? reinterpret_cast<float*>(base + 2 * piece) : nullptr;
    s.bytes = 3 * piece;
    return s;
}
// what both entry points refuse from the dims alone (inside a CallScope)
int input_grad_dims(const regt_dims* dims, const char* what) {
    REGT_CHECK_ARG(gemm_mode() != 2, "%s: the bf16 arithmetic is not covered (fp32 and bf16x3 are); pass dims.arith = REGT_ARITH_FP32 or "
                   "REGT_ARITH_BF16X3", what);
    REGT_CHECK_ARG(!(dims->flags & REGT_DIMS_FORWARD_ONLY), "%s: REGT_DIMS_FORWARD_ONLY is for the forward", what);
    REGT_CHECK_ARG(dims->F <= 64, "%s: dx covers a (padded) feature width F <= 64 (F=%d)", what, dims->F);
    return REGT_OK;
}
}  // namespace

size_t regt_input_gradient_scratch_bytes(const regt_dims* dims) {
    if (check_dims(dims)) return 0;
    CallScope call(dims);
    if (input_grad_dims(dims, "regt_input_gradient_scratch_bytes")) return 0;
    return input_grad_layout(*dims, nullptr).bytes;
}

int32_t regt_input_gradient(const regt_dims* dims, const regt_graph* graph, const regt_params* params, const int32_t* t_rowptr,
                            const int32_t* t_col, const float* t_val_a, const float* t_val_l, float* dx, void* ws, size_t ws_bytes,
                            void* scratch, size_t scratch_bytes, regt_stream_t st) {
    TRY(check_dims(dims));
    CallScope call(dims);
    const regt_dims& d = *dims;
    TRY(input_grad_dims(dims, "regt_input_gradient"));
    REGT_CHECK_ARG(graph != nullptr, "regt_input_gradient: graph is NULL");
    REGT_CHECK_ARG(!graph->overlap, "regt_input_gradient: overlapping regions (graph.overlap = 1) are not covered: one Laplacian per region has no "
                   "merged transposed operator");
    const int fmt = q_format(ws);
    REGT_CHECK_ARG(!(fmt & FMT_FWDONLY), "regt_input_gradient: the last forward on this workspace ran with REGT_DIMS_FORWARD_ONLY and kept no "
                   "activations; run regt_forward without that flag and regt_backward first");
    REGT_CHECK_ARG(!(fmt & FMT_PACKED), "regt_input_gradient: the last forward on this workspace read packed rows (regt_forward_packed): the gradient "
                   "of halo rows needs an exchange that is not covered");
    REGT_CHECK_ARG(!(fmt & (FMT_QBF | FMT_XBF)), "regt_input_gradient: the last forward on this workspace ran in the bf16 arithmetic, which is not covered");
    REGT_CHECK_ARG(!d.regional || d.R == 1 || graph->node_region, "regt_input_gradient: graph.node_region is NULL");
    TRY(check_ptrs(params, d));
    REGT_CHECK_ARG(t_rowptr && t_col && t_val_a && t_val_l, "regt_input_gradient: dx needs the transposed merged operator (t_rowptr, t_col, t_val_a, "
                   "t_val_l)");
    REGT_CHECK_ARG(dx && ws && scratch, "regt_input_gradient: NULL pointer");
    REGT_CHECK_ARG(al16(dx) && al16(ws) && al16(scratch) && al16(params->cheb_w0) && al16(params->cheb_w1),
                   "regt_input_gradient: dx, workspace, scratch and the Chebyshev weights must be 16-byte aligned");
    const Layout L = make_layout(d, graph->n_chunks, 0, (char*)ws);
    REGT_CHECK_ARG(ws_bytes >= L.bytes, "regt_input_gradient: workspace %zu < required %zu bytes (regt_workspace_bytes)", ws_bytes, L.bytes);
    const InputGradLayout s = input_grad_layout(d, (char*)scratch);
    REGT_CHECK_ARG(scratch_bytes >= s.bytes, "regt_input_gradient: scratch %zu < required %zu bytes (regt_input_gradient_scratch_bytes)", scratch_bytes,
                   s.bytes);
    hipStream_t hs = (hipStream_t)st;
    const int C = d.C, F = d.F;
    const bool tcol = (fmt & FMT_TCOLLAPSE) != 0;
    // (regt_backward's last writers of dzr, dhp and dh are its data gradients; the weight gradients, the slab reduction and the
    // compositions behind them only read the three, so they are still what the data gradients left)
    ModelDxArgs a{};
    a.A[0] = L.dzr; a.K[0] = 2 * C;
    a.A[1] = L.dhp; a.K[1] = C;
    a.A[2] = L.dh;  a.K[2] = C;          // ds, the embedding's pre-activation gradient; collapsed TemporalGCN: dh without the gates' term
    a.B[0][0] = L.Gzr;
    a.B[1][0] = L.Gh;
    if (tcol) { a.B[0][1] = L.P0zr; a.B[0][2] = L.P1zr; }
    a.B[2][1] = d.regional ? L.A0 : params->cheb_w0;
    a.B[2][2] = d.regional ? L.Aall : params->cheb_w1;
    if (d.regional && d.R > 1) { a.node_region = graph->node_region; a.Breg = L.Aall; a.breg_stride = (long)C * F; }
    a.out[0] = s.dAX; a.out[1] = s.dXd; a.out[2] = s.dLX;
    a.M = (long)d.N * d.T; a.F = F; a.T = d.T; a.R = d.R;
    {
        PROF("model_dx", hs);
        TRY(launch_model_dx(a, hs));
    }
    PROF("spmm_dx", hs);
    return launch_spmm_dual_t(t_rowptr, t_col, t_val_a, t_val_l, s.dAX, s.dLX, s.dXd, dx, d.N, F, d.T, hs);
}

/* ---- streaming inference: attention-weighted window sum over cached cell outputs + head (regtgcn.h) ---- */
// workspace: the T attention probabilities (a fixed 255-float region: the size does not depend on T), then the head's (rows x H1) activation
static const size_t WINDOW_PROBS_BYTES = 1024;
static size_t window_ws_bytes(long rows, int H1) { return WINDOW_PROBS_BYTES + (((size_t)rows * H1 * sizeof(float) + 255) & ~(size_t)255); }

int32_t regt_window_chunk(int32_t windows) { return window_chunk(windows); }

size_t regt_window_workspace_bytes(int32_t N, int32_t C, int32_t H1, int32_t O, int32_t windows) {
    if (!(N > 0 && C > 0 && H1 > 0 && O > 0 && windows > 0 && (long)N * windows <= INT_MAX)) {
        set_error("regt_window_workspace_bytes: N, C, H1, O, windows must be positive and windows * N below 2^31 (N=%d C=%d H1=%d O=%d windows=%d)",
                  N, C, H1, O, windows);
        return 0;
    }
    return window_ws_bytes((long)N * windows, H1);
}

int32_t regt_window_forward(const float* ring, int32_t ring_len, int32_t first_slot, int32_t windows, int32_t N, int32_t T, int32_t C,
                            int32_t O, int32_t H1, const float* attention, const float* head1_w, const float* head1_b,
                            const float* head2_w, const float* head2_b, float* pred, float* hidden, void* ws, size_t ws_bytes,
                            regt_stream_t st) {
    REGT_CHECK_ARG(ring && attention && head1_w && head1_b && head2_w && head2_b && pred && hidden && ws, "regt_window_forward: NULL pointer");
    REGT_CHECK_ARG(N > 0 && C > 0 && O > 0 && H1 > 0 && T > 0 && windows > 0 && ring_len > 0,
                   "regt_window_forward: ring_len, windows, N, T, C, O, H1 must be positive (ring_len=%d windows=%d N=%d T=%d C=%d O=%d H1=%d)",
                   ring_len, windows, N, T, C, O, H1);
    REGT_CHECK_ARG(C % 4 == 0, "regt_window_forward: C=%d must be a multiple of 4", C);
    REGT_CHECK_ARG(T <= 255, "regt_window_forward: T=%d exceeds 255 periods", T);
    REGT_CHECK_ARG(ring_len >= T, "regt_window_forward: ring_len=%d < T=%d", ring_len, T);
    REGT_CHECK_ARG(first_slot >= 0 && first_slot < ring_len, "regt_window_forward: first_slot=%d outside [0, ring_len=%d)", first_slot, ring_len);
    REGT_CHECK_ARG(windows == 1 || (long)windows + T - 1 <= ring_len,
                   "regt_window_forward: windows=%d of T=%d periods would wrap onto themselves in a ring of %d slots (only a single window may use all of it)",
                   windows, T, ring_len);
    REGT_CHECK_ARG((long)N * windows <= INT_MAX, "regt_window_forward: windows * N too large");
    REGT_CHECK_ARG(windows <= WINDOW_MAX_CHUNKS * WINDOW_WC, "regt_window_forward: windows=%d exceeds the %d one call covers", windows,
                   WINDOW_MAX_CHUNKS * WINDOW_WC);
    REGT_CHECK_ARG(al16(ring) && al16(hidden) && al16(ws), "regt_window_forward: ring, hidden and workspace must be 16-byte aligned");
    const size_t need = window_ws_bytes((long)N * windows, H1);
    REGT_CHECK_ARG(ws_bytes >= need, "regt_window_forward: workspace %zu < required %zu bytes (regt_window_workspace_bytes)", ws_bytes, need);
    hipStream_t hs = (hipStream_t)st;
    float* probs = static_cast<float*>(ws);
    float* y1 = reinterpret_cast<float*>(static_cast<char*>(ws) + WINDOW_PROBS_BYTES);
    {
        PROF("window_sum", hs);
        TRY(launch_softmax_small(attention, probs, T, hs));      // the launch regt_forward's own attention weights come from
        TRY(launch_window_sum(ring, probs, hidden, ring_len, first_slot, windows, N, T, C, hs));
    }
    // the head of regt_forward's tail, on windows * N rows
    regt_dims d{};
    d.N = N * windows; d.T = T; d.C = C; d.O = O; d.H1 = H1;
    regt_params p{};
    p.head1_w = head1_w; p.head1_b = head1_b; p.head2_w = head2_w; p.head2_b = head2_b;
    return head_forward(d, p, hidden, y1, pred, hs);
}

/* ---- streamed training: the backward of regt_window_forward (regtgcn.h) ---- */
namespace {
// workspace: the T probabilities (WINDOW_PROBS_BYTES), the head's activation y1 and its gradient d1 (rows x H1 each), dhidden (rows x C),
// the head's four gradients of this call (delivered to the caller's tensors in one launch: written or added), the slabs of the head's
// weight gradients (make_layout's head terms), the attention gradient's partial rows (one per workgroup)
struct WindowBwdLayout {
    float *probs, *y1, *d1, *dhidden, *g1w, *g1b, *g2w, *g2b, *slab, *partial;
    long slab_floats;
    size_t bytes;
};
WindowBwdLayout window_bwd_layout(long rows, int windows, int N, int C, int H1, int O, int T, char* base) {
    WindowBwdLayout L{};
    size_t off = 0;
    auto take = [&](size_t nbytes) {
        float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += (nbytes + 255) & ~(size_t)255;
        return p;
    };
    L.probs = take(WINDOW_PROBS_BYTES);
    L.y1 = take((size_t)rows * H1 * 4);
    L.d1 = take((size_t)rows * H1 * 4);
    L.dhidden = take((size_t)rows * C * 4);
    L.g1w = take((size_t)H1 * C * 4);
    L.g1b = take((size_t)H1 * 4);
    L.g2w = take((size_t)O * H1 * 4);
    L.g2b = take((size_t)O * 4);
    const HeadChunks hc = head_chunks(rows, H1, C);
    L.slab_floats = (long)hc.n1 * ((long)H1 * C + H1 + (long)O * H1 + O) + (long)hc.n2 * ((long)O * H1 + O) + 16 * 64;
    L.slab = take((size_t)L.slab_floats * 4);
    L.partial = take((size_t)window_attgrad_blocks(windows, N, C) * T * 4);
    L.bytes = off;
    return L;
}
bool window_bwd_dims_ok(int N, int C, int H1, int O, int windows, int T) {
    return N > 0 && C > 0 && H1 > 0 && O > 0 && windows > 0 && T > 0 && C % 4 == 0 && T <= WINDOW_BWD_MAX_T && (long)N * windows <= INT_MAX &&
           (long)windows + T - 1 <= (long)WINDOW_MAX_CHUNKS * WINDOW_WC;
}
}  // namespace

int32_t regt_window_backward_max_t(void) { return WINDOW_BWD_MAX_T; }

size_t regt_window_backward_workspace_bytes(int32_t N, int32_t C, int32_t H1, int32_t O, int32_t windows, int32_t T) {
    if (!window_bwd_dims_ok(N, C, H1, O, windows, T)) {
        set_error("regt_window_backward_workspace_bytes: N, C, H1, O, windows, T must be positive, C a multiple of 4, T <= %d and windows * N below 2^31 "
                  "(N=%d C=%d H1=%d O=%d windows=%d T=%d)", WINDOW_BWD_MAX_T, N, C, H1, O, windows, T);
        return 0;
    }
    return window_bwd_layout((long)N * windows, windows, N, C, H1, O, T, nullptr).bytes;
}

int32_t regt_window_backward(const float* ring, int32_t ring_len, int32_t first_slot, int32_t windows, int32_t N, int32_t T, int32_t C,
                             int32_t O, int32_t H1, const float* attention, const float* head1_w, const float* head1_b,
                             const float* head2_w, const float* head2_b, const float* hidden, const float* dpred, float* dring,
                             int32_t accumulate, float* d_attention, float* d_head1_w, float* d_head1_b, float* d_head2_w,
                             float* d_head2_b, void* ws, size_t ws_bytes, regt_stream_t st) {
    REGT_CHECK_ARG(ring && attention && head1_w && head1_b && head2_w && head2_b && hidden && dpred && dring && d_attention && d_head1_w &&
                   d_head1_b && d_head2_w && d_head2_b && ws, "regt_window_backward: NULL pointer");
    REGT_CHECK_ARG(N > 0 && C > 0 && O > 0 && H1 > 0 && T > 0 && windows > 0 && ring_len > 0,
                   "regt_window_backward: ring_len, windows, N, T, C, O, H1 must be positive (ring_len=%d windows=%d N=%d T=%d C=%d O=%d H1=%d)",
                   ring_len, windows, N, T, C, O, H1);
    REGT_CHECK_ARG(C % 4 == 0, "regt_window_backward: C=%d must be a multiple of 4", C);
    REGT_CHECK_ARG(T <= WINDOW_BWD_MAX_T, "regt_window_backward: T=%d exceeds the %d periods the backward covers (regt_window_backward_max_t)", T,
                   WINDOW_BWD_MAX_T);
    REGT_CHECK_ARG(ring_len >= T, "regt_window_backward: ring_len=%d < T=%d", ring_len, T);
    REGT_CHECK_ARG(first_slot >= 0 && first_slot < ring_len, "regt_window_backward: first_slot=%d outside [0, ring_len=%d)", first_slot, ring_len);
    REGT_CHECK_ARG((long)windows + T - 1 <= ring_len,
                   "regt_window_backward: windows=%d of T=%d periods would wrap onto themselves in a ring of %d slots", windows, T, ring_len);
    REGT_CHECK_ARG((long)N * windows <= INT_MAX, "regt_window_backward: windows * N too large");
    REGT_CHECK_ARG((long)windows + T - 1 <= (long)WINDOW_MAX_CHUNKS * WINDOW_WC, "regt_window_backward: windows=%d exceeds the %d one call covers",
                   windows, WINDOW_MAX_CHUNKS * WINDOW_WC - T + 1);
    REGT_CHECK_ARG(al16(ring) && al16(hidden) && al16(dring) && al16(ws),
                   "regt_window_backward: ring, hidden, dring and workspace must be 16-byte aligned");
    const long rows = (long)N * windows;
    const WindowBwdLayout L = window_bwd_layout(rows, windows, N, C, H1, O, T, static_cast<char*>(ws));
    REGT_CHECK_ARG(ws_bytes >= L.bytes, "regt_window_backward: workspace %zu < required %zu bytes (regt_window_backward_workspace_bytes)", ws_bytes,
                   L.bytes);
    hipStream_t hs = (hipStream_t)st;
    regt_dims d{};
    d.N = (int)rows; d.T = T; d.C = C; d.O = O; d.H1 = H1;
    regt_params p{};
    p.head1_w = head1_w; p.head1_b = head1_b; p.head2_w = head2_w; p.head2_b = head2_b;
    regt_grads gr{};
    gr.head1_w = L.g1w; gr.head1_b = L.g1b; gr.head2_w = L.g2w; gr.head2_b = L.g2b;
    TRY(launch_softmax_small(attention, L.probs, T, hs));
    {   // y1 = relu(linear1(relu(hidden))): the first layer of head_forward, recomputed
        EpiBiasAct e{L.y1, H1, head1_b, ACT_RELU, 0.f};
        PROF("head_fwd", hs);
        TRY(launch_gemm_bias_act(one_seg(make_seg(hidden, C, head1_w, nullptr, C, INT_MAX, C, true, SEG_RELU_A)), (int)rows, H1, e, hs));
    }
    ReduceQueue rq(L.slab, L.slab_floats, hs);
    TRY(head_backward(d, p, gr, dpred, nullptr, hidden, L.y1, L.d1, L.dhidden, rq, hs));
    TRY(rq.flush());
    {
        DeliverArgs a{};
        a.count = 4; a.accumulate = accumulate ? 1 : 0;
        a.src[0] = L.g1w; a.dst[0] = d_head1_w; a.n[0] = (long)H1 * C;
        a.src[1] = L.g1b; a.dst[1] = d_head1_b; a.n[1] = H1;
        a.src[2] = L.g2w; a.dst[2] = d_head2_w; a.n[2] = (long)O * H1;
        a.src[3] = L.g2b; a.dst[3] = d_head2_b; a.n[3] = O;
        TRY(launch_deliver(a, hs));
    }
    {
        PROF("window_adjoint", hs);
        TRY(launch_window_adjoint(L.dhidden, L.probs, dring, ring_len, first_slot, windows, N, T, C, accumulate ? 1 : 0, hs));
    }
    PROF("window_attgrad", hs);
    return launch_window_attgrad(ring, L.dhidden, L.probs, L.partial, d_attention, ring_len, first_slot, windows, N, T, C, accumulate ? 1 : 0, hs);
}

}  // extern "C"
