// The zero-hidden cell (GraphSAGE / GAT models of the reference): the GRU at H = 0 on gate inputs the caller supplies, then the step's head.
#include "api_internal.h"

namespace regt { namespace {

int check_cell0(const regt_dims* d, const regt_cell0_args* a) {
    REGT_CHECK_ARG(d && a, "regt_cell0: NULL dims / args");
    REGT_CHECK_ARG(d->N > 0 && d->T > 0 && d->C > 0 && d->O > 0 && d->H1 > 0 && d->C % 4 == 0 && d->T <= 255, "regt_cell0: bad dims");
    REGT_CHECK_ARG((long)d->N * d->T < (1L << 31), "regt_cell0: N*T too large");
    REGT_CHECK_ARG(a->kz > 0 && a->kh > 0 && a->a_z && a->a_h && a->gz && a->gh && a->cz && a->ch && a->attention && a->head1_w &&
                   a->head1_b && a->head2_w && a->head2_b, "regt_cell0: a required pointer is NULL");
    return REGT_OK;
}
regt_params head_params(const regt_cell0_args& a) {
    regt_params p{};
    p.head1_w = a.head1_w; p.head1_b = a.head1_b; p.head2_w = a.head2_w; p.head2_b = a.head2_b;
    return p;
}
}}  // namespace regt::(anonymous)

using namespace regt;

extern "C" {

int32_t regt_cell0_forward(const regt_dims* dims, const regt_cell0_args* args, float* pred, float* hidden, void* ws, size_t ws_bytes,
                           regt_stream_t st_) {
    TRY(check_cell0(dims, args));
    CallScope call(dims);
    REGT_CHECK_ARG(pred && hidden && ws && al16(hidden) && al16(ws), "regt_cell0_forward: NULL / unaligned pointer");
    const regt_dims& d = *dims;
    const regt_cell0_args& a = *args;
    Layout0 L = make_layout0(d, a.kz, a.kh, (char*)ws);
    REGT_CHECK_ARG(ws_bytes >= L.bytes, "regt_cell0_forward: workspace %zu < required %zu bytes", ws_bytes, L.bytes);
    hipStream_t st = (hipStream_t)st_;
    const long M = (long)d.N * d.T;
    TRY(launch_softmax_small(a.attention, L.probs, d.T, st));
    for (int k = 0; k < 2; ++k) {      // Z = sigmoid(a_z gz^T + cz), H~ = tanh(a_h gh^T + ch)
        const int kk = k ? a.kh : a.kz;
        EpiBiasAct e{k ? L.Ht : L.Z, d.C, k ? a.ch : a.cz, k ? ACT_TANH : ACT_SIGMOID, 0.f};
        PROF(k ? "cell0_candidate" : "cell0_gate", st);
        TRY(launch_gemm_bias_act(one_seg(make_seg(k ? a.a_h : a.a_z, kk, k ? a.gh : a.gz, nullptr, kk, INT_MAX, kk, true)), M, d.C, e, st));
    }
    {
        PROF("cell0_blend", st);
        TRY(launch_blend0_fwd(L.Z, L.Ht, L.probs, hidden, d.N, d.T, d.C, st));
    }
    return head_forward(d, head_params(a), hidden, L.y1, pred, st);
}

int32_t regt_cell0_backward(const regt_dims* dims, const regt_cell0_args* args, const regt_cell0_grads* grads, const float* dpred,
                            const float* dhidden, const float* hidden, void* ws, size_t ws_bytes, regt_stream_t st_) {
    TRY(check_cell0(dims, args));
    CallScope call(dims);
    REGT_CHECK_ARG(grads && dpred && hidden && ws, "regt_cell0_backward: NULL pointer");
    const regt_cell0_grads& g = *grads;
    REGT_CHECK_ARG(g.gz && g.gh && g.cz && g.ch && g.head1_w && g.head1_b && g.head2_w && g.head2_b,
                   "regt_cell0_backward: a required gradient pointer is NULL (only attention, a_z, a_h may be NULL)");
    const regt_dims& d = *dims;
    const regt_cell0_args& a = *args;
    Layout0 L = make_layout0(d, a.kz, a.kh, (char*)ws);
    REGT_CHECK_ARG(ws_bytes >= L.bytes, "regt_cell0_backward: workspace %zu < required %zu bytes", ws_bytes, L.bytes);
    hipStream_t st = (hipStream_t)st_;
    const int N = d.N, T = d.T, C = d.C;
    const long M = (long)N * T;
    ReduceQueue rq(L.slab, L.slab_floats, st);
    regt_grads hg{};
    hg.head1_w = g.head1_w; hg.head1_b = g.head1_b; hg.head2_w = g.head2_w; hg.head2_b = g.head2_b;
    TRY(head_backward(d, head_params(a), hg, dpred, dhidden, hidden, L.y1, L.d1, L.dOH, rq, st));
    {   // dhp = g (1-Z)(1-H~^2), dzp = -g H~ Z (1-Z), g = p_t dOH: the GRU backward head with h = 0
        CellBwdArgs c{L.dOH, L.probs, L.Z, nullptr, L.Ht, L.dhp, L.dzp, L.dp_partial, N, T, C, L.cb_npb};
        c.ldz = C; c.lddz = C;
        PROF("cell_bwd", st);
        TRY(launch_cell_bwd(c, st));
        if (g.attention) TRY(launch_att_bwd(L.dp_partial, L.cb_blocks, L.probs, g.attention, T, st));
    }
    TRY(wgrad_full(rq, "wgrad_gz", L.dzp, C, C, a.a_z, a.kz, a.kz, 0, M, L.kchunk, L.nchunks, g.gz, a.kz, g.cz, st));
    TRY(wgrad_full(rq, "wgrad_gh", L.dhp, C, C, a.a_h, a.kh, a.kh, 0, M, L.kchunk, L.nchunks, g.gh, a.kh, g.ch, st));
    TRY(rq.flush());
    for (int k = 0; k < 2; ++k) {      // optional input gradients: da = dpre G  (M x C) (C x k)
        float* da = k ? g.a_h : g.a_z;
        if (!da) continue;
        const int kk = k ? a.kh : a.kz;
        EpiBiasAct e{da, kk, nullptr, ACT_NONE, 0.f};
        PROF("cell0_dinput", st);
        TRY(launch_gemm_bias_act(one_seg(make_seg(k ? L.dhp : L.dzp, C, k ? a.gh : a.gz, nullptr, kk, INT_MAX, C, false)), M, kk, e, st));
    }
    return REGT_OK;
}

}  // extern "C"
