"""Bars, blocks and shared cases of the STAEformer self-attention layer's backward tests (test helper only).

Bars are those of grad_bars.py (REL, CAP, ill_conditioned, imported, not restated); this file only maps the layer's names to a class
and to blocks, which grad_bars.grad_class / grad_blocks do for the older models' names.

Classes:  ``attention`` -- dq, dk, dv and everything upstream of them in the layer (attn.FC_Q / FC_K / FC_V and the input x): the
softmax backward is a difference of nearly equal sums.  ``norm`` -- dz, dgamma, dbeta of add+LayerNorm and everything whose gradient
comes back through a LayerNorm backward (attn.out_proj, feed_forward.*, ln1.*, ln2.*).
Blocks:  dq / dk / dv per (sequence, head); row gradients (dz, x) per 64 rows; weight gradients per 32 x 32 quadrant; vectors whole.
A well-conditioned block is held to REL[class] x max|want64_block|, an ill-conditioned one (grad_bars.ill_conditioned: the fp32
restatement's own error takes more than CAP / 4 of the block's scale) to 4 x max|ref32 - want64| with no floor, a block that is exactly
zero in float64 must be exactly zero.  One block has no scale of its own: the gradient of attn.FC_K.bias is identically zero in exact
arithmetic (stae_layer_math.key_bias_scale), so float64 returns 1e-16-sized residue for it; it is held to REL x the magnitude of the rows it
sums, max_col sum_rows |dK|, which the float64 restatement alone gives.  Forward values and lse: 1e-5 + 4 x the fp32-vs-float64 gap of the restatement on the same inputs.

The cases of tests/test_gpu_stae_backward.py are built here, so that tests/test_stae_backward_cpu.py can prove on the host, with the
fp32 restatement in the kernels' place, that none of the golden's blocks and at most 5 % of the GPU file's blocks are ill-conditioned.
Seeds and scales: attention cases draw standard normal q, k, v, dout from seed 1000 axis + 10 L + heads + 100 batch (the large-score
case: seed 77, q x 30); add+LayerNorm cases standard normal from seed 7 M + D, gamma = 1 + 0.5 (u - 0.5), dout standard normal; layer
cases seed 31 (B + T + N) + axis with the parameters of ``layer_state`` (seed 5: default initialisers, biases and LayerNorm
parameters perturbed as in the goldens), x and dout standard normal; the (B, L, D) case is layer_case(2, 1, 33, axis 2); the two-layer
stack seed 404 with the parameters of seeds 5 and 6."""
import functools

import torch

from grad_bars import CAP, REL, ill_conditioned
from stae_layer_math import LAYER_KEYS, add_layernorm_grads, attention_grads, key_bias_scale, layer_forward, layer_grads

K_GAP = 4
ROWS = 64
QUAD = 32
assert all(REL[c] <= CAP[c] for c in ("attention", "norm", "default"))


def grad_class(name: str) -> str:
    if name in ("dq", "dk", "dv", "x") or name.startswith(("attn.FC_Q.", "attn.FC_K.", "attn.FC_V.")):
        return "attention"
    return "norm"


def blocks(name: str, t: torch.Tensor, axis=None):
    """[(label, flat tensor)] of one gradient.  dq / dk / dv: (B, T, N, D) with ``axis``; x / dz: (..., D) rows; weights 2-D; vectors 1-D."""
    if name in ("dq", "dk", "dv"):
        b, tt, n, d = t.shape
        z = t.transpose(1, 2) if axis == 1 else t                    # (B, S, L, D)
        z = z.reshape(z.shape[0], z.shape[1], z.shape[2], d // QUAD, QUAD)
        return [(f"{name}[b {i}, seq {s}, head {h}]", z[i, s, :, h].reshape(-1)) for i in range(z.shape[0]) for s in range(z.shape[1])
                for h in range(d // QUAD)]
    if t.dim() == 1:
        return [(name, t)]
    if name in ("x", "dz"):
        r = t.reshape(-1, t.shape[-1])
        return [(f"{name}[rows {a}:{min(a + ROWS, r.shape[0])}]", r[a:a + ROWS].reshape(-1)) for a in range(0, r.shape[0], ROWS)]
    assert t.dim() == 2, (name, tuple(t.shape))
    return [(f"{name}[{a}:{a + QUAD}, {c}:{c + QUAD}]", t[a:a + QUAD, c:c + QUAD].reshape(-1)) for a in range(0, t.shape[0], QUAD)
            for c in range(0, t.shape[1], QUAD)]


def block_rows(got, want64, ref32, axis=None, scales=None):
    """[(label, class, err, scale, gap)] over every block of every gradient in ``want64`` (dicts name -> tensor).  ``scales``: name ->
    the scale of a whole-tensor block where its own float64 maximum is none (attn.FC_K.bias, stae_layer_math.key_bias_scale)."""
    rows = []
    for name, want in want64.items():
        w = want.detach().cpu().double()
        g, r = got[name].detach().cpu().double(), ref32[name].detach().cpu().double()
        assert g.shape == w.shape == r.shape, (name, tuple(g.shape), tuple(w.shape), tuple(r.shape))
        for (label, eb), (_, wb), (_, gb) in zip(blocks(name, (g - w).abs(), axis), blocks(name, w.abs(), axis), blocks(name, (r - w).abs(), axis)):
            scale = scales[name] if scales and name in scales else float(wb.max())
            rows.append((label, grad_class(name), float(eb.max()), scale, float(gb.max())))
    return rows


def assert_blocks(got, want64, ref32, what, axis=None, rel=REL, scales=None):
    """The conditioned assertion of grad_bars.assert_grads_conditioned on this layer's blocks.  Returns (labels of the ill-conditioned
    blocks, number of blocks, {class: worst err / scale over the well-conditioned blocks})."""
    bad, ill, worst = [], [], {}
    rows = block_rows(got, want64, ref32, axis, scales)
    for label, cls, err, scale, gap in rows:
        if ill_conditioned(cls, scale, gap):
            ill.append(label)
            if not err <= K_GAP * gap:
                bad.append(f"{label} [{cls}, ill-conditioned: fp32 restatement off by {gap / scale:.3e} of scale]: max|err| {err:.3e} > {K_GAP} x {gap:.3e}")
        else:
            if scale > 0:
                worst[cls] = max(worst.get(cls, 0.0), err / scale)
            if not err <= rel[cls] * scale:             # (NaN fails; scale 0 demands err 0)
                bad.append(f"{label} [{cls}]: max|err| {err:.3e} vs scale {scale:.3e}: ratio {err / scale if scale > 0 else float('inf'):.3e} > {rel[cls]:.3e}")
    print(f"{what}: {len(rows)} blocks, {len(ill)} ill-conditioned, worst ratio " + ", ".join(f"{c} {v:.3e} (bar {rel[c]:.3e})" for c, v in sorted(worst.items())))
    assert not bad, f"{what}: {len(bad)} gradient block(s) off their own scale:\n  " + "\n  ".join(bad[:40])
    return ill, len(rows), worst


def forward_bar(got, r64, r32, what):
    """|got - r64| <= 1e-5 + K_GAP * max|r32 - r64| (the bar of test_gpu_staeformer.py)."""
    got, r64 = got.detach().cpu().double(), r64.double()
    gap = float((r32.double() - r64).abs().max())
    err = float((got - r64).abs().max())
    print(f"{what}: max |error| {err:.3g}, fp32 restatement gap {gap:.3g}, K needed {err / max(gap, 1e-30):.2f} (bar K_GAP = {K_GAP} + 1e-5)")
    assert torch.isfinite(got).all(), what
    assert err <= 1e-5 + K_GAP * gap, (what, err, gap)


# ---- cases ----------------------------------------------------------------------------------------------------------------------

ATTN_LENGTHS, ATTN_HEADS, ATTN_BATCHES = (1, 2, 31, 32, 33, 65), (1, 4), (1, 3)
ATTN_CASES = [(length, axis, heads, batch) for length in ATTN_LENGTHS for axis in (1, 2) for heads in ATTN_HEADS for batch in ATTN_BATCHES]
LARGE_SCORE_CASES = [(65, 1, 4, 2), (65, 2, 4, 2)]
LN_CASES = [(m, d) for m in (1, 63, 64, 65, 1000) for d in (32, 128, 256)]
LAYER_SHAPES = [(1, 1, 1), (2, 5, 7), (1, 12, 33), (2, 3, 65)]
LAYER_DIM, LAYER_HEADS, LAYER_FF = 128, 4, 256


def attention_shape(length, axis, batch):
    """The other extent is small and odd, so that the sequence count is no multiple of a workgroup's four waves."""
    return (batch, length, 5) if axis == 1 else (batch, 7, length)


@functools.lru_cache(maxsize=None)
def attention_case(length, axis, heads, batch, q_scale=1.0):
    """q, k, v, dout (B, T, N, D) on the host with the float64 and fp32 restatements: dict of tensors and the two result tuples
    (out, lse, dq, dk, dv)."""
    b, t, n = attention_shape(length, axis, batch)
    d = 32 * heads
    gen = torch.Generator().manual_seed(77 if q_scale != 1.0 else 1000 * axis + 10 * length + heads + 100 * batch)
    q, k, v, dout = (torch.randn(b, t, n, d, generator=gen) for _ in range(4))
    q = q * q_scale
    r64 = attention_grads(q, k, v, axis, dout)
    r32 = attention_grads(q, k, v, axis, dout, dtype=torch.float32)
    return {"q": q, "k": k, "v": v, "dout": dout, "shape": (b, t, n)}, r64, r32


@functools.lru_cache(maxsize=None)
def layernorm_case(m, d, kind="normal"):
    """kind: "normal", "constant_row" (row 0 of residual + y is constant: variance 0) or "gamma_zeros" (every third gamma is 0)."""
    gen = torch.Generator().manual_seed(7 * m + d)
    res, y, dout = (torch.randn(m, d, generator=gen) for _ in range(3))
    gamma = 1.0 + 0.5 * (torch.rand(d, generator=gen) - 0.5)
    beta = 0.4 * (torch.rand(d, generator=gen) - 0.5)
    if kind == "constant_row":
        res[0], y[0] = 1.5, -0.25
    if kind == "gamma_zeros":
        gamma[::3] = 0.0
    r64 = add_layernorm_grads(res, y, gamma, beta, dout)
    r32 = add_layernorm_grads(res, y, gamma, beta, dout, dtype=torch.float32)
    return {"residual": res, "y": y, "gamma": gamma, "beta": beta, "dout": dout}, r64, r32


def layer_state(model_dim=LAYER_DIM, ff=LAYER_FF, seed=5):
    """A 16-entry state_dict in the reference's order: nn.Linear's default initialiser, biases and LayerNorm parameters perturbed."""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for key in LAYER_KEYS:
        mod, kind = key.rsplit(".", 1)
        fan_out, fan_in = {"feed_forward.0": (ff, model_dim), "feed_forward.2": (model_dim, ff)}.get(mod, (model_dim, model_dim))
        if mod.startswith("ln"):
            sd[key] = (1.0 if kind == "weight" else 0.0) + 0.5 * (torch.rand(model_dim, generator=gen) - 0.5)
        elif kind == "weight":
            sd[key] = (torch.rand(fan_out, fan_in, generator=gen) * 2 - 1) / fan_in ** 0.5
        else:
            sd[key] = 0.4 * (torch.rand(fan_out, generator=gen) - 0.5)
    return sd


@functools.lru_cache(maxsize=None)
def layer_case(b, t, n, axis):
    gen = torch.Generator().manual_seed(31 * (b + t + n) + axis)
    x, dout = torch.randn(b, t, n, LAYER_DIM, generator=gen), torch.randn(b, t, n, LAYER_DIM, generator=gen)
    sd = layer_state()
    r64 = layer_grads(sd, x, axis, dout)
    r32 = layer_grads(sd, x, axis, dout, dtype=torch.float32)
    return {"x": x, "dout": dout, "sd": sd, "scales": {"attn.FC_K.bias": key_bias_scale(sd, x, axis, dout)}}, r64, r32


LAYER_3D_SHAPE = (2, 33)         # x (B, L, D) with dim=1: the same arithmetic as layer_case(B, 1, L, axis=2)


@functools.lru_cache(maxsize=None)
def stack_case():
    """Two layers, temporal then spatial, on (2, 5, 7): x, dout, the two state_dicts, and per dtype (out, gradients) with the names
    "x", "0.<key>", "1.<key>"; scales: attn.FC_K.bias of each layer from its own input and upstream gradient."""
    b, t, n = 2, 5, 7
    gen = torch.Generator().manual_seed(404)
    x, dout = torch.randn(b, t, n, LAYER_DIM, generator=gen), torch.randn(b, t, n, LAYER_DIM, generator=gen)
    sds = [layer_state(seed=5), layer_state(seed=6)]

    def oracle(dtype):
        x0 = x.detach().to(dtype).requires_grad_(True)             # (detach: .to() of the same dtype is the tensor itself)
        ps = [{k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()} for sd in sds]
        h = layer_forward(ps[0], x0, 1, dtype=dtype)
        o = layer_forward(ps[1], h, 2, dtype=dtype)
        leaves = {"x": x0, "h": h, **{f"{i}.{k}": v for i, p in enumerate(ps) for k, v in p.items()}}
        return o.detach(), h.detach(), dict(zip(leaves, torch.autograd.grad(o, list(leaves.values()), dout.to(dtype))))

    (o64, h64, g64), (o32, _, g32) = oracle(torch.float64), oracle(torch.float32)
    scales = [{"attn.FC_K.bias": key_bias_scale(sds[0], x, 1, g64["h"])}, {"attn.FC_K.bias": key_bias_scale(sds[1], h64, 2, dout)}]
    return {"x": x, "dout": dout, "sds": sds, "scales": scales}, (o64, g64), (o32, g32)


def stack_layer_grads(grads, i):
    """The gradients of layer i of a stack_case dictionary under their state_dict names."""
    return {k[2:]: v for k, v in grads.items() if k.startswith(f"{i}.")}


def attention_grad_dicts(res):
    return {"dq": res[2], "dk": res[3], "dv": res[4]}


def layernorm_grad_dicts(res):
    return {"dz": res[1], "dgamma": res[2], "dbeta": res[3]}


# ---- runners on the GPU (tests/test_gpu_stae_backward.py and tools/stae_backward_bars.py) -----------------------------------------

DEV = "cuda:0"
SENTINEL = -777.0
NAN = float("nan")


def attention_buffers(case, heads):
    """Q | K | V as strided windows of one (M + 3, 3 D + 8) device buffer whose padding columns and tail rows hold NaN, and dout as a
    window of a NaN-filled (M + 2, D + 8) buffer: (buffer, q, k, v, dout)."""
    b, t, n = case["shape"]
    d, m = 32 * heads, b * t * n
    buf = torch.full((m + 3, 3 * d + 8), NAN)
    for i, name in enumerate(("q", "k", "v")):
        buf[:m, i * d:(i + 1) * d] = case[name].reshape(m, d)
    buf = buf.to(DEV)
    dobuf = torch.full((m + 2, d + 8), NAN, device=DEV)
    dobuf[1:m + 1, 4:4 + d] = case["dout"].reshape(m, d).to(DEV)
    return (buf,) + tuple(buf[:m, i * d:(i + 1) * d] for i in range(3)) + (dobuf[1:m + 1, 4:4 + d],)


def run_attention(case, heads, axis, runs=1):
    """The training forward and the backward on the windows of attention_buffers; out is a window of a NaN-filled (M + 2, D + 8)
    buffer, dq | dk | dv windows of a sentinel-filled (M + 2, 3 D + 12) buffer.  Returns (out, out of the inference entry, lse,
    [gradient buffer per run])."""
    from regtgcn_amd import ops
    b, t, n = case["shape"]
    d, m = 32 * heads, b * t * n
    _, q, k, v, dout = attention_buffers(case, heads)
    obuf = torch.full((m + 2, d + 8), NAN, device=DEV)
    out, lse = ops.stae_attention_train(q, k, v, b, t, n, heads, axis, out=obuf[1:m + 1, 4:4 + d])
    out_inf = ops.stae_attention(q, k, v, b, t, n, heads, axis)
    gbufs = []
    for _ in range(runs):
        gbuf = torch.full((m + 2, 3 * d + 12), SENTINEL, device=DEV)
        ops.stae_attention_backward(q, k, v, out, dout, lse, b, t, n, heads, axis, grads=gbuf[1:m + 1, 4:])
        gbufs.append(gbuf)
    torch.cuda.synchronize()
    return out, out_inf, lse, gbufs


def attention_grads_of(gbuf, case, heads):
    """dq, dk, dv (B, T, N, D) out of run_attention's gradient buffer; everything outside the three windows must still be the
    sentinel, everything inside finite."""
    b, t, n = case["shape"]
    d, m = 32 * heads, b * t * n
    g = gbuf.cpu()
    assert bool((g[0] == SENTINEL).all()) and bool((g[m + 1] == SENTINEL).all())
    assert bool((g[:, :4] == SENTINEL).all()) and bool((g[:, 4 + 3 * d:] == SENTINEL).all())
    win = g[1:m + 1, 4:4 + 3 * d]
    assert bool(torch.isfinite(win).all())
    return {name: win[:, i * d:(i + 1) * d].reshape(b, t, n, d) for i, name in enumerate(("dq", "dk", "dv"))}


def run_layernorm(case):
    from regtgcn_amd import ops
    c = {k: v.to(DEV) for k, v in case.items()}
    out = ops.stae_add_layernorm(c["residual"], c["y"], c["gamma"], c["beta"])
    dz, dg, db = ops.stae_add_layernorm_backward(c["residual"], c["y"], c["gamma"], c["dout"])
    torch.cuda.synchronize()
    return out, {"dz": dz, "dgamma": dg, "dbeta": db}


def make_layer(sd, model_dim=LAYER_DIM, heads=LAYER_HEADS, ff=LAYER_FF, dropout=0):
    import regtgcn_amd as R
    mod = R.SelfAttentionLayer(model_dim, feed_forward_dim=ff, num_heads=heads, dropout=dropout)
    mod.load_state_dict(sd, strict=True)
    return mod.to(DEV).train()


def run_layer_backward(mod, x, dim, dout):
    """-> (out, {"x": dx, <state_dict key>: gradient})."""
    xr = x.to(DEV).requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    out = mod(xr, dim=dim)
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    grads = {"x": xr.grad}
    grads.update({k: p.grad for k, p in mod.named_parameters()})
    return out.detach(), grads
