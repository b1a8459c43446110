"""One STAEformer self-attention layer and its two non-dense ops restated in plain torch WITH their gradients (autograd does the
differentiation), float64 by default, fp32 on request.  Test helper only; the forward formulas are those of staeformer_math.py:

    attention      O = softmax(Q_h K_h^T / sqrt(32)) V_h per head of 32 columns along the axis; lse = logsumexp of the scaled scores
    add_layernorm  LayerNorm(residual + y) gamma + beta, biased variance
    layer          A = attention(X Wq^T + bq, X Wk^T + bk, X Wv^T + bv) Wo^T + bo;  H = LN1(X + A);  out = LN2(H + relu(H W1^T + b1) W2^T + b2)

Every function takes an upstream gradient ``dout`` and returns the forward value(s) and the gradients of ``sum(out * dout)``."""
import torch

from staeformer_math import HEAD, add_layernorm, attention, layer

LAYER_KEYS = [f"attn.{n}.{w}" for n in ("FC_Q", "FC_K", "FC_V", "out_proj") for w in ("weight", "bias")] + \
             [f"feed_forward.{i}.{w}" for i in (0, 2) for w in ("weight", "bias")] + [f"ln{i}.{w}" for i in (1, 2) for w in ("weight", "bias")]


def attention_lse(q, k, axis, dtype=torch.float64):
    """(B, T, N, heads): log sum_j exp(q_i . k_j / sqrt(32)) per position and head."""
    b, t, n, d = q.shape
    def heads(z):
        z = z.to(dtype)
        if axis == 1:
            z = z.transpose(1, 2)
        return z.reshape(z.shape[0], z.shape[1], z.shape[2], d // HEAD, HEAD).transpose(2, 3)     # (B, S, H, L, 32)
    lse = torch.logsumexp(heads(q) @ heads(k).transpose(-1, -2) / HEAD ** 0.5, dim=-1).transpose(2, 3)      # (B, S, L, H)
    return lse.transpose(1, 2) if axis == 1 else lse


def attention_grads(q, k, v, axis, dout, dtype=torch.float64):
    """q, k, v, dout (B, T, N, D) -> (out, lse, dq, dk, dv)."""
    q, k, v = (z.detach().to(dtype).requires_grad_(True) for z in (q, k, v))
    out = attention(q, k, v, axis, dtype)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), dout.to(dtype))
    return out.detach(), attention_lse(q.detach(), k.detach(), axis, dtype), dq, dk, dv


def add_layernorm_grads(residual, y, gamma, beta, dout, eps=1e-5, dtype=torch.float64):
    """-> (out, dz, dgamma, dbeta); dz is the gradient of residual and of y alike."""
    residual, y, gamma, beta = (z.detach().to(dtype).requires_grad_(True) for z in (residual, y, gamma, beta))
    out = add_layernorm(residual, y, gamma, beta, eps, dtype)
    dz, dy, dg, db = torch.autograd.grad(out, (residual, y, gamma, beta), dout.to(dtype))
    assert torch.equal(dz, dy)
    return out.detach(), dz, dg, db


def layer_forward(sd, x, axis, eps=1e-5, dtype=torch.float64):
    """sd: the layer's 16-entry state_dict; x (B, T, N, D)."""
    return layer({f"l.{k}": v for k, v in sd.items()}, "l", x.to(dtype), axis, eps, dtype)


def layer_grads(sd, x, axis, dout, eps=1e-5, dtype=torch.float64):
    """-> (out, {"x": dx, <state_dict key>: gradient, ...}), 17 gradients."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    x = x.detach().to(dtype).requires_grad_(True)
    out = layer_forward(p, x, axis, eps, dtype)
    names = ["x"] + list(p)
    grads = torch.autograd.grad(out, [x] + list(p.values()), dout.to(dtype))
    return out.detach(), dict(zip(names, grads))


def key_bias_scale(sd, x, axis, dout, eps=1e-5):
    """max over columns of sum_rows |dK[row, col]| in float64, dK the gradient of the key projection's output.  The gradient of
    attn.FC_K.bias is sum_rows dK, and that sum is identically ZERO in exact arithmetic: adding one vector to every key shifts all
    scores of a query alike, which the softmax does not see (sum_j dS_ij = 0).  Whatever an implementation returns for it is the
    rounding residue of a fully cancelling sum, so its own maximum is no scale; the magnitude of what is summed is.
    The restatement is staeformer_math.layer itself: the key bias is handed to it as one row per position (it broadcasts the same
    way), and the gradient of that per-row bias is dK."""
    p = {k: v.detach().double() for k, v in sd.items()}
    x = x.detach().double()
    rows = p["attn.FC_K.bias"].expand(*x.shape[:-1], -1).clone().requires_grad_(True)
    p["attn.FC_K.bias"] = rows
    (dk,) = torch.autograd.grad(layer_forward(p, x, axis, eps), rows, dout.double())
    return float(dk.abs().reshape(-1, dk.shape[-1]).sum(0).max())
