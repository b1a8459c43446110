"""The whole STAEformer restated in plain torch for TRAINING (test helper only): staeformer_math.py's forward with an optional keep
mask on each dropout site, float64 by default, fp32 on request; gradients come by autograd.  The two table indices are clamped into
their tables (what the kernels do).  Dropout sits where the reference has it (models/STAEformer.py:98-104):

    H = LN1(X + keep1 * A / (1 - p));   out = LN2(H + keep2 * F / (1 - p))

Sites are numbered as nn.draw_stae_keep draws them: the temporal layers first, then the spatial ones, dropout1 before dropout2.
Keep masks travel as the project's words, int32 (sites, M, D / 32), bit j of word w keeps column 32 w + j, rows (b T + t) N + n."""
import torch

from stae_layer_math import key_bias_scale  # noqa: F401  (re-exported for the bars)
from staeformer_math import add_layernorm, attention, embed


def unpack_keep(words: torch.Tensor, d: int) -> torch.Tensor:
    """int32 (..., D / 32) -> bool (..., D)."""
    w = words.to(torch.int64) & 0xFFFFFFFF
    bits = (w.unsqueeze(-1) >> torch.arange(32)) & 1
    return bits.reshape(*words.shape[:-1], d).bool()


def pack_keep(mask: torch.Tensor) -> torch.Tensor:
    """bool (..., D) -> int32 (..., D / 32), bytewise as nn.draw_stid_keep packs."""
    m = mask.reshape(*mask.shape[:-1], mask.shape[-1] // 8, 8).to(torch.uint8)
    weights = (2 ** torch.arange(8)).to(torch.uint8)
    return (m * weights).sum(-1, dtype=torch.uint8).view(torch.int32)


def drop_add_layernorm(residual, y, keep, p, gamma, beta, eps=1e-5, dtype=torch.float64):
    """keep: bool (M, D) or None."""
    y = y.to(dtype)
    if keep is not None:
        y = y * keep.to(dtype) / (1.0 - p)
    return add_layernorm(residual, y, gamma, beta, eps, dtype)


def layer(p, pre, x, axis, keep1=None, keep2=None, drop=0.0, eps=1e-5, dtype=torch.float64):
    """x (B, T, N, D); keep1 / keep2 bool (B, T, N, D) or None."""
    c = lambda z: z.to(dtype)
    lin = lambda z, name: z @ c(p[f"{pre}.{name}.weight"]).T + c(p[f"{pre}.{name}.bias"])
    a = attention(lin(x, "attn.FC_Q"), lin(x, "attn.FC_K"), lin(x, "attn.FC_V"), axis, dtype)
    x = drop_add_layernorm(x, lin(a, "attn.out_proj"), keep1, drop, p[f"{pre}.ln1.weight"], p[f"{pre}.ln1.bias"], eps, dtype)
    f = lin(torch.relu(lin(x, "feed_forward.0")), "feed_forward.2")
    return drop_add_layernorm(x, f, keep2, drop, p[f"{pre}.ln2.weight"], p[f"{pre}.ln2.bias"], eps, dtype)


def layer_prefixes(p):
    out = []
    for kind, axis in (("t", 1), ("s", 2)):
        i = 0
        while f"attn_layers_{kind}.{i}.ln1.weight" in p:
            out.append((f"attn_layers_{kind}.{i}", axis))
            i += 1
    return out


def staeformer_train(p, x, out_steps, output_dim=1, keep=None, drop=0.0, dtype=torch.float64, eps=1e-5, taps=None):
    """out (B, out_steps, N, output_dim); ``keep`` int32 words (sites, M, D / 32) or None.  ``taps``: a list that receives every
    layer's input (B, T, N, D), for the key-bias scales."""
    b, t, n, _ = x.shape
    h = embed(p, x, dtype, clamp=True)
    d = h.shape[-1]
    for i, (pre, axis) in enumerate(layer_prefixes(p)):
        k1 = k2 = None
        if keep is not None:
            k1, k2 = (unpack_keep(keep[2 * i + j], d).reshape(b, t, n, d) for j in (0, 1))
        if taps is not None:
            taps.append(h)
        h = layer(p, pre, h, axis, k1, k2, drop, eps, dtype)
    if taps is not None:
        taps.append(h)
    rows = h.transpose(1, 2).reshape(b, n, t * d)
    out = rows @ p["output_proj.weight"].to(dtype).T + p["output_proj.bias"].to(dtype)
    return out.view(b, n, out_steps, output_dim).transpose(1, 2)


def window_losses(out, y):
    """run.py:184 / :186 per snapshot: mean((out - y) ** 2) with out (B, O, N, C) against y (B, N, O) broadcast as run.py does."""
    return ((out - y.to(out.dtype).unsqueeze(1)) ** 2).mean(dim=(1, 2, 3))


def model_grads(sd, x, out_steps, output_dim=1, keep=None, drop=0.0, dtype=torch.float64, dout=None, y=None):
    """-> (out, per-snapshot losses or None, {state_dict key: gradient}).  The scalar differentiated is sum(out * dout), or, with
    ``y``, the sum of run.py's per-snapshot losses."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    out = staeformer_train(p, x, out_steps, output_dim, keep, drop, dtype)
    losses = None
    if y is not None:
        losses = window_losses(out, y)
        scalar = losses.sum()
    else:
        scalar = (out * dout.to(dtype)).sum()
    grads = torch.autograd.grad(scalar, list(p.values()))
    return out.detach(), None if losses is None else losses.detach(), dict(zip(p, grads))


def key_bias_scales(sd, x, out_steps, output_dim=1, keep=None, drop=0.0, dout=None, y=None):
    """{'<layer>.attn.FC_K.bias': max_col sum_rows |dK|} in float64 for every layer: the scale of a gradient that is identically zero
    in exact arithmetic (stae_layer_math.key_bias_scale).  The key bias of each layer is handed over as one row per position."""
    p = {k: v.detach().double() for k, v in sd.items()}
    b, t, n, _ = x.shape
    d = p["attn_layers_t.0.ln1.weight"].shape[0]
    rows = {}
    for pre, _ in layer_prefixes(p):
        key = f"{pre}.attn.FC_K.bias"
        rows[key] = p[key].expand(b, t, n, d).clone().requires_grad_(True)
        p[key] = rows[key]
    out = staeformer_train(p, x, out_steps, output_dim, keep, drop)
    scalar = window_losses(out, y).sum() if y is not None else (out * dout.double()).sum()
    grads = torch.autograd.grad(scalar, list(rows.values()))
    return {k: float(g.abs().reshape(-1, d).sum(0).max()) for k, g in zip(rows, grads)}
