"""The STAEformer self-attention layer's backward on the GPU: the attention backward and the add+LayerNorm backward entry points
against the float64 restatement with autograd (tests/stae_layer_math.py), functional.STAEAttentionFunction on strided windows, and
nn.SelfAttentionLayer against the reference's own output and gradients (tests/golden/golden_stae_layer.npz) and against the
restatement.

Bars (tests/stae_layer_bars.py, values imported from grad_bars.py): forward values and lse 1e-5 + 4 x the fp32 restatement's gap; every
gradient block REL[class] x the block's own float64 scale, an ill-conditioned block 4 x the fp32 restatement's error, a zero block
exactly zero.  tests/test_stae_backward_cpu.py proves on the host that the golden has no ill-conditioned block and this file's cases
at most 5 %.  Every case's restatement is computed once on the host (stae_layer_bars caches it); the runners that put a case on the
GPU live there too (tools/stae_backward_bars.py shares them)."""
import pytest
import torch

from conftest import load_npz
from stae_layer_bars import (ATTN_CASES, DEV, LARGE_SCORE_CASES, LAYER_3D_SHAPE, LAYER_SHAPES, LN_CASES, assert_blocks, attention_buffers,
                             attention_case, attention_grad_dicts, attention_grads_of, forward_bar, layer_case, layernorm_case,
                             layernorm_grad_dicts, make_layer, run_attention, run_layer_backward, run_layernorm, stack_case, stack_layer_grads)
from stae_layer_math import key_bias_scale, layer_grads
from staeformer_math import golden_state_dict

pytestmark = pytest.mark.gpu


# ---- attention ----------------------------------------------------------------------------------------------------------------------

def _check_attention(length, axis, heads, batch, q_scale=1.0):
    case, r64, r32 = attention_case(length, axis, heads, batch, q_scale)
    what = f"attention backward L {length} axis {axis} heads {heads} B {batch}" + (f" q x {q_scale:g}" if q_scale != 1.0 else "")
    out, out_inf, lse, (gbuf,) = run_attention(case, heads, axis)
    m = out.shape[0]
    assert torch.equal(out, out_inf), what + ": the training forward's out differs from the inference entry's"
    forward_bar(out, r64[0].reshape(m, -1), r32[0].reshape(m, -1), what + ": out")
    forward_bar(lse, r64[1].reshape(m, heads), r32[1].reshape(m, heads), what + ": lse")
    return assert_blocks(attention_grads_of(gbuf, case, heads), attention_grad_dicts(r64), attention_grad_dicts(r32), what, axis=axis)


@pytest.mark.parametrize("length,axis,heads,batch", ATTN_CASES)
def test_attention_backward(length, axis, heads, batch):
    _check_attention(length, axis, heads, batch)


@pytest.mark.parametrize("length,axis,heads,batch", LARGE_SCORE_CASES)
def test_attention_backward_with_large_scores(length, axis, heads, batch):
    """q scaled by 30: the scores reach the hundreds; the probabilities are rebuilt from lse, never from an unshifted exp."""
    case, _, _ = attention_case(length, axis, heads, batch, 30.0)
    q0, k0 = case["q"][..., :32], case["k"][..., :32]
    scores = torch.einsum("blnd,bmnd->bnlm" if axis == 1 else "btld,btmd->btlm", q0, k0) / 32 ** 0.5
    assert float(scores.abs().max()) > 100
    _check_attention(length, axis, heads, batch, 30.0)


@pytest.mark.parametrize("length,axis,heads,batch", [(65, 1, 4, 3), (65, 2, 4, 3), (33, 2, 1, 1)])
def test_attention_backward_is_bit_reproducible(length, axis, heads, batch):
    case, _, _ = attention_case(length, axis, heads, batch)
    _, _, _, (g1, g2) = run_attention(case, heads, axis, runs=2)
    assert torch.equal(g1, g2)


# ---- functional.STAEAttentionFunction -------------------------------------------------------------------------------------------------

def _function_case(length, axis, heads, batch):
    """The case's Q | K | V buffer as ONE leaf that requires grad, q, k, v its strided windows; dout a strided window too."""
    case, r64, r32 = attention_case(length, axis, heads, batch)
    buf, _, _, _, dout = attention_buffers(case, heads)
    b, t, n = case["shape"]
    d, m = 32 * heads, b * t * n
    leaf = torch.nan_to_num(buf, nan=0.0).requires_grad_(True)             # (the padding's gradient must come back as exactly 0)
    return case, r64, r32, leaf, [leaf[:m, i * d:(i + 1) * d] for i in range(3)], dout, (b, t, n, d, m)


@pytest.mark.parametrize("length,axis,heads,batch", [(33, 1, 4, 3), (65, 2, 4, 1), (2, 2, 1, 3)])
def test_attention_function_on_strided_windows(length, axis, heads, batch):
    """q, k, v are windows of one leaf buffer, the upstream gradient arrives strided: out and dq | dk | dv against the restatement,
    nothing but the three windows of the leaf receives a gradient."""
    from regtgcn_amd.functional import STAEAttentionFunction
    case, r64, r32, leaf, (q, k, v), dout, (b, t, n, d, m) = _function_case(length, axis, heads, batch)
    what = f"STAEAttentionFunction L {length} axis {axis} heads {heads} B {batch}"
    out = STAEAttentionFunction.apply(q, k, v, b, t, n, heads, axis)
    assert out.requires_grad
    out.backward(dout)
    torch.cuda.synchronize()
    forward_bar(out, r64[0].reshape(m, d), r32[0].reshape(m, d), what + ": out")
    g = leaf.grad.cpu()
    assert bool((g[m:] == 0).all()) and bool((g[:, 3 * d:] == 0).all())
    got = {name: g[:m, i * d:(i + 1) * d].reshape(b, t, n, d) for i, name in enumerate(("dq", "dk", "dv"))}
    assert_blocks(got, attention_grad_dicts(r64), attention_grad_dicts(r32), what, axis=axis)


def test_attention_function_with_some_inputs_needing_no_gradient():
    """Only v, then only q and k, require grad: the others' gradients are None, the wanted ones are the full backward's bits."""
    from regtgcn_amd.functional import STAEAttentionFunction
    length, axis, heads, batch = 33, 2, 4, 1
    case, r64, r32, leaf, (q, k, v), dout, (b, t, n, d, m) = _function_case(length, axis, heads, batch)
    out = STAEAttentionFunction.apply(q, k, v, b, t, n, heads, axis)
    full = torch.autograd.grad(out, (q, k, v), dout)
    for needs in ((False, False, True), (True, True, False)):
        ins = [z.detach().requires_grad_(need) for z, need in zip((q, k, v), needs)]
        o = STAEAttentionFunction.apply(*ins, b, t, n, heads, axis)
        assert torch.equal(o, out)
        o.backward(dout)
        for z, need, want in zip(ins, needs, full):
            assert (z.grad is not None) == need
            if need:
                assert torch.equal(z.grad, want)
    got = {name: gz.cpu().reshape(b, t, n, d) for name, gz in zip(("dq", "dk", "dv"), full)}
    assert_blocks(got, attention_grad_dicts(r64), attention_grad_dicts(r32), "STAEAttentionFunction, torch.autograd.grad", axis=axis)


def test_attention_function_without_gradients_is_the_inference_entry():
    from regtgcn_amd import ops
    from regtgcn_amd.functional import STAEAttentionFunction
    length, axis, heads, batch = 33, 1, 4, 3
    case, _, _, leaf, (q, k, v), _, (b, t, n, d, m) = _function_case(length, axis, heads, batch)
    want = ops.stae_attention(q.detach(), k.detach(), v.detach(), b, t, n, heads, axis)
    with torch.no_grad():
        a = STAEAttentionFunction.apply(q, k, v, b, t, n, heads, axis)
    c = STAEAttentionFunction.apply(q.detach(), k.detach(), v.detach(), b, t, n, heads, axis)       # grad mode on, nothing requires grad
    assert not a.requires_grad and not c.requires_grad and c.grad_fn is None
    assert torch.equal(a, want) and torch.equal(c, want)
    assert torch.equal(STAEAttentionFunction.apply(q, k, v, b, t, n, heads, axis), want)              # the training forward: the same bits


# ---- add + LayerNorm ------------------------------------------------------------------------------------------------------------------

def _check_layernorm(m, d, kind="normal"):
    case, r64, r32 = layernorm_case(m, d, kind)
    what = f"add_layernorm backward M {m} D {d} {kind}"
    out, grads = run_layernorm(case)
    forward_bar(out, r64[0], r32[0], what + ": out")
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()), what
    return assert_blocks(grads, layernorm_grad_dicts(r64), layernorm_grad_dicts(r32), what)


@pytest.mark.parametrize("m,d", LN_CASES)
def test_add_layernorm_backward(m, d):
    _check_layernorm(m, d)


@pytest.mark.parametrize("d", [32, 256])
def test_add_layernorm_backward_constant_row_is_finite(d):
    """Row 0 of residual + y is constant: variance 0, rstd = 1 / sqrt(eps)."""
    _check_layernorm(65, d, "constant_row")


def test_add_layernorm_backward_does_not_divide_by_gamma():
    """Every third gamma is 0: x^ is recomputed from residual and y, never as (out - beta) / gamma."""
    _check_layernorm(65, 128, "gamma_zeros")


def test_add_layernorm_backward_is_bit_reproducible():
    case, _, _ = layernorm_case(1000, 256)
    _, a = run_layernorm(case)
    _, b = run_layernorm(case)
    assert all(torch.equal(a[k], b[k]) for k in a)


# ---- the layer ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 2])
def test_layer_matches_reference_golden(dim):
    """Output and all 17 gradients of the reference's SelfAttentionLayer (fp32, CPU) as recorded; ref32 of the conditioned assertion
    is the reference's own fp32 result, want64 the float64 restatement."""
    g = load_npz("golden_stae_layer.npz")
    sd = golden_state_dict(g)
    x, dout = torch.from_numpy(g["x"]), torch.from_numpy(g["dout"])
    mod = make_layer(sd, int(g["model_dim"]), int(g["num_heads"]), int(g["feed_forward_dim"]))
    out, grads = run_layer_backward(mod, x, dim, dout)
    o64, g64 = layer_grads(sd, x, dim, dout)
    ref_out = torch.from_numpy(g[f"dim{dim}__out"])
    ref = {k: torch.from_numpy(g[f"dim{dim}__grad__{k}"]) for k in g64}
    forward_bar(out, o64, ref_out, f"golden layer dim {dim}: out")
    ill, _, _ = assert_blocks(grads, g64, ref, f"golden layer dim {dim}", scales={"attn.FC_K.bias": key_bias_scale(sd, x, dim, dout)})
    assert not ill, ill


@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("b,t,n", LAYER_SHAPES)
def test_layer_matches_restatement(b, t, n, axis):
    case, r64, r32 = layer_case(b, t, n, axis)
    mod = make_layer(case["sd"])
    out, grads = run_layer_backward(mod, case["x"], axis, case["dout"])
    what = f"layer B {b} T {t} N {n} axis {axis}"
    forward_bar(out, r64[0], r32[0], what + ": out")
    assert_blocks(grads, r64[1], r32[1], what, scales=case["scales"])
    with torch.no_grad():
        assert torch.equal(mod(case["x"].to(DEV), dim=axis), out), what + ": no_grad output differs from the training-mode output"


@pytest.mark.parametrize("dim", [1, -2])
def test_layer_on_three_dimensional_input(dim):
    """x (B, L, D) with dim = 1 / -2 is (B, 1, L, D) along the nodes: output and all 17 gradients against the restatement, and the
    bits of the four-dimensional call."""
    b, n = LAYER_3D_SHAPE
    case, r64, r32 = layer_case(b, 1, n, 2)
    mod = make_layer(case["sd"])
    out, grads = run_layer_backward(mod, case["x"][:, 0], dim, case["dout"][:, 0])
    assert tuple(out.shape) == (b, n, case["x"].shape[-1]) and tuple(grads["x"].shape) == tuple(out.shape)
    what = f"layer on (B, L, D) = ({b}, {n}, D), dim {dim}"
    forward_bar(out, r64[0][:, 0], r32[0][:, 0], what + ": out")
    got = dict(grads, x=grads["x"][:, None])
    assert_blocks(got, r64[1], r32[1], what, scales=case["scales"])
    out4, grads4 = run_layer_backward(mod, case["x"], 2, case["dout"])
    assert torch.equal(out4[:, 0], out) and all(torch.equal(got[k], grads4[k]) for k in grads4)


def test_layer_with_dropout_refuses_training_mode_and_runs_in_eval():
    case, _, _ = layer_case(2, 5, 7, 1)
    mod = make_layer(case["sd"], dropout=0.1)
    x = case["x"].to(DEV)
    with pytest.raises(NotImplementedError, match="dropout"):
        mod(x, dim=1)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="dropout"):
        mod(x, dim=1)
    out, grads = run_layer_backward(mod.eval(), case["x"], 1, case["dout"])           # eval(): dropout is the identity, gradients flow
    ref_out, ref_grads = run_layer_backward(make_layer(case["sd"]), case["x"], 1, case["dout"])
    assert torch.equal(out, ref_out) and all(torch.equal(grads[k], ref_grads[k]) for k in ref_grads)


def test_two_layer_stack_passes_dx_on():
    """Temporal then spatial, as STAEformer stacks them: the first layer's parameters receive their gradients through the second
    layer's dx."""
    case, (o64, g64), (o32, g32) = stack_case()
    mods = [make_layer(sd) for sd in case["sds"]]
    xr = case["x"].to(DEV).requires_grad_(True)
    out = mods[1](mods[0](xr, dim=1), dim=2)
    out.backward(case["dout"].to(DEV))
    got = {"x": xr.grad}
    for i, mod in enumerate(mods):
        got.update({f"{i}.{k}": p.grad for k, p in mod.named_parameters()})
    forward_bar(out, o64, o32, "two-layer stack: out")
    for i in (0, 1):
        assert_blocks(stack_layer_grads(got, i), stack_layer_grads(g64, i), stack_layer_grads(g32, i), f"two-layer stack: layer {i}",
                      scales=case["scales"][i])
    assert_blocks({"x": got["x"]}, {"x": g64["x"]}, {"x": g32["x"]}, "two-layer stack: x")


@pytest.mark.parametrize("in_backward", [False, True])
def test_layer_accumulates_gradients_over_two_backward_calls(in_backward):
    from regtgcn_amd.functional import set_grad_accumulation_in_backward
    case, _, _ = layer_case(2, 5, 7, 1)
    mod = make_layer(case["sd"])
    _, once = run_layer_backward(mod, case["x"], 1, case["dout"])
    once = {k: v.clone() for k, v in once.items()}
    prev = set_grad_accumulation_in_backward(in_backward)
    try:
        mod.zero_grad(set_to_none=True)
        for _ in range(2):
            mod(case["x"].to(DEV), dim=1).backward(case["dout"].to(DEV))
    finally:
        set_grad_accumulation_in_backward(prev)
    for k, p in mod.named_parameters():
        assert torch.equal(p.grad, once[k] + once[k]), (k, in_backward)           # g + g is exact in fp32


def test_layer_forward_is_one_layer_of_the_inference_sequence():
    """nn.STAEformer with one temporal and one spatial layer computes embed -> layer_t -> layer_s -> output_proj in regt_stae_forward;
    the trainable layers on the same weights, between the same embedding and projection restated on the host, are held to the
    forward bar against the restatement, and so is their direct difference from regt_stae_forward's output."""
    import regtgcn_amd as R
    from staeformer_math import embed, staeformer
    torch.manual_seed(11)
    full = R.STAEformer(num_nodes=7, in_steps=5, out_steps=2, tod_embedding_dim=0, num_layers=1, dropout=0).to(DEV).eval()
    x = torch.rand(2, 5, 7, 3)
    sd = {k: v.detach().cpu() for k, v in full.state_dict().items()}
    layers = []
    for kind in ("t", "s"):
        pre = f"attn_layers_{kind}.0."
        layers.append(make_layer({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, full.model_dim, full.num_heads,
                                 full.feed_forward_dim).eval())
    with torch.no_grad():
        want = full(x.to(DEV)).cpu()
        h = embed(sd, x, dtype=torch.float32, clamp=True).to(DEV)
        h = layers[1](layers[0](h, dim=1), dim=2).cpu()
    rows = h.transpose(1, 2).reshape(2, 7, -1)
    got = (rows @ sd["output_proj.weight"].T + sd["output_proj.bias"]).view(2, 7, 2, 1).transpose(1, 2)
    r64, r32 = staeformer(sd, x, 2, clamp=True), staeformer(sd, x, 2, dtype=torch.float32, clamp=True)
    forward_bar(got, r64, r32, "layers vs restatement")
    gap = float((r32.double() - r64).abs().max())
    err = float((got - want).abs().max())
    print(f"layers vs regt_stae_forward: max |difference| {err:.3g} (bar {1e-5 + 4 * gap:.3g})")
    assert err <= 1e-5 + 4 * gap, (err, gap)


def test_staeformer_itself_still_refuses_grad_mode():
    import regtgcn_amd as R
    torch.manual_seed(3)
    mod = R.STAEformer(num_nodes=7, in_steps=4, out_steps=2, tod_embedding_dim=0, num_layers=1, dropout=0).to(DEV)
    x = torch.rand(2, 4, 7, 3, device=DEV)
    with pytest.raises(NotImplementedError, match="inference only"):
        mod(x)
    with pytest.raises(NotImplementedError, match="inference only"):
        mod.eval()(x.clone().requires_grad_(True))
