"""STAEformer (Liu et al., CIKM 2023, "Spatio-Temporal Adaptive Embedding Makes Vanilla Transformer SOTA for Traffic Forecasting")
restated in plain torch for inference (dropout is the identity), float64 by default, from the paper's definition and the shapes of
the module's parameters.  With rows m = (b, t, n) of D = model_dim floats:

    X_0   = [x[..., :input_dim] Win^T + bin | tod_emb[idx_tod] | dow_emb[idx_dow] | node_emb[n] | adaptive[t, n]]
            idx_tod = trunc(x[..., 1] * steps_per_day), idx_dow = trunc(x[..., 2]); a block whose table is absent is left out
    layer : A = attention(X Wq^T + bq, X Wk^T + bk, X Wv^T + bv, axis) Wo^T + bo;   X = LN1(X + A)
            X = LN2(X + relu(X W1^T + b1) W2^T + b2)
            num_layers layers along the time axis (axis 1), then num_layers along the node axis (axis 2)
    out[b, o, n, c] = sum_{t, d} X[b, t, n, d] Wout[o * output_dim + c, t * D + d] + bout

attention: heads of 32 columns, softmax(Q_h K_h^T / sqrt(32)) V_h over the positions of the axis.  ``clamp=True`` clamps the two
table indices into their tables (what the kernels do where the reference would raise)."""
import numpy as np
import torch

HEAD = 32


def encode_bf16(t: torch.Tensor) -> np.ndarray:
    """bf16-exact float32 values as the two byte planes of their bf16 patterns, uint8 (2, *shape): [0] sign and exponent, [1] the
    rest.  The golden files store the parameters this way (a plane of like bytes compresses far better than interleaved floats)."""
    bits = t.detach().contiguous().numpy().view(np.uint32)
    assert not (bits & 0xFFFF).any(), "not bf16-exact"
    return np.stack([(bits >> 24).astype(np.uint8), ((bits >> 16) & 0xFF).astype(np.uint8)])


def decode_bf16(planes: np.ndarray) -> torch.Tensor:
    bits = (planes[0].astype(np.uint32) << 24) | (planes[1].astype(np.uint32) << 16)
    return torch.from_numpy(bits.view(np.float32).copy())


def golden_state_dict(g) -> dict:
    """{name: float32 tensor} in state_dict order from a golden file's ``state_dict_keys`` and ``p__<name>`` byte planes."""
    return {str(k): decode_bf16(g[f"p__{k}"]) for k in g["state_dict_keys"]}


def attention(q, k, v, axis, dtype=torch.float64):
    """q, k, v (B, T, N, 32 * heads); self-attention along axis 1 (time) or 2 (nodes), heads of 32 columns."""
    b, t, n, d = q.shape
    def heads(z):
        z = z.to(dtype)
        if axis == 1:
            z = z.transpose(1, 2)                                   # (B, N, T, D): the sequence is the second-to-last axis
        return z.reshape(z.shape[0], z.shape[1], z.shape[2], d // HEAD, HEAD).transpose(2, 3)     # (B, S, H, L, 32)
    qh, kh, vh = heads(q), heads(k), heads(v)
    p = torch.softmax(qh @ kh.transpose(-1, -2) / HEAD ** 0.5, dim=-1)
    o = (p @ vh).transpose(2, 3).reshape(qh.shape[0], qh.shape[1], qh.shape[3], d)
    return o.transpose(1, 2) if axis == 1 else o


def add_layernorm(residual, y, gamma, beta, eps=1e-5, dtype=torch.float64):
    z = residual.to(dtype) + y.to(dtype)
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    return (z - mean) / torch.sqrt(var + eps) * gamma.to(dtype) + beta.to(dtype)


def table_indices(x, steps_per_day, days_per_week, clamp=False):
    """(idx_tod, idx_dow) as the module forms them from float32 x (truncation toward zero), optionally clamped into the tables."""
    tod = (x[..., 1] * steps_per_day).long() if x.shape[-1] > 1 else None
    dow = x[..., 2].long() if x.shape[-1] > 2 else None
    if clamp:
        tod = None if tod is None else tod.clamp(0, steps_per_day - 1)
        dow = None if dow is None else dow.clamp(0, days_per_week - 1)
    return tod, dow


def embed(p, x, dtype=torch.float64, clamp=False):
    c = lambda z: z.to(dtype)
    b, t, n, _ = x.shape
    win = c(p["input_proj.weight"])
    parts = [c(x)[..., :win.shape[1]] @ win.T + c(p["input_proj.bias"])]
    tod, dow = table_indices(x, p["tod_embedding.weight"].shape[0] if "tod_embedding.weight" in p else 1,
                             p["dow_embedding.weight"].shape[0] if "dow_embedding.weight" in p else 1, clamp)
    if "tod_embedding.weight" in p:
        parts.append(c(p["tod_embedding.weight"])[tod])
    if "dow_embedding.weight" in p:
        parts.append(c(p["dow_embedding.weight"])[dow])
    if "node_emb" in p:
        parts.append(c(p["node_emb"]).expand(b, t, n, -1))
    if "adaptive_embedding" in p:
        parts.append(c(p["adaptive_embedding"]).expand(b, t, n, -1))
    return torch.cat(parts, dim=-1)


def layer(p, pre, x, axis, eps=1e-5, dtype=torch.float64):
    c = lambda z: z.to(dtype)
    lin = lambda z, name: z @ c(p[f"{pre}.{name}.weight"]).T + c(p[f"{pre}.{name}.bias"])
    a = attention(lin(x, "attn.FC_Q"), lin(x, "attn.FC_K"), lin(x, "attn.FC_V"), axis, dtype)
    x = add_layernorm(x, lin(a, "attn.out_proj"), p[f"{pre}.ln1.weight"], p[f"{pre}.ln1.bias"], eps, dtype)
    f = lin(torch.relu(lin(x, "feed_forward.0")), "feed_forward.2")
    return add_layernorm(x, f, p[f"{pre}.ln2.weight"], p[f"{pre}.ln2.bias"], eps, dtype)


def staeformer(p, x, out_steps, output_dim=1, dtype=torch.float64, clamp=False, eps=1e-5):
    """out (B, out_steps, N, output_dim) for x (B, T, N, F); ``p`` maps the state_dict names to tensors."""
    b, t, n, _ = x.shape
    h = embed(p, x, dtype, clamp)
    for kind, axis in (("t", 1), ("s", 2)):
        i = 0
        while f"attn_layers_{kind}.{i}.ln1.weight" in p:
            h = layer(p, f"attn_layers_{kind}.{i}", h, axis, eps, dtype)
            i += 1
    rows = h.transpose(1, 2).reshape(b, n, t * h.shape[-1])
    out = rows @ p["output_proj.weight"].to(dtype).T + p["output_proj.bias"].to(dtype)
    return out.view(b, n, out_steps, output_dim).transpose(1, 2)
