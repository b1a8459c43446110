"""One step of the TGCN cell (models/utils.py:163-203) and its full backward, restated from the formulas: test helper only.

    ax = A_hat x                          conv_k = ax W_k^T + b_k                       k = z, r, h
    z = sigmoid([conv_z | h] U_z^T + u_z)     r = sigmoid([conv_r | h] U_r^T + u_r)     h~ = tanh([conv_h | h * r] U_h^T + u_h)
    h' = z * h + (1 - z) * h~

Backward from d = dL/dh', hand-written (no autograd), in the dtype of its inputs -- float64 is the reference, float32 its restatement:

    dp_h = d (1 - z) (1 - h~^2)           dp_z = d (h - h~) z (1 - z)                   dq = dp_h U_h[:, C:]
    dp_r = dq h r (1 - r)                 dh = d z + dq r + dp_z U_z[:, C:] + dp_r U_r[:, C:]
    dU_k = dp_k^T [conv_k | h or h * r]   du_k = colsum dp_k                            dconv_k = dp_k U_k[:, :C]
    dW_k = dconv_k^T ax                   db_k = colsum dconv_k
    dAx = sum_k dconv_k W_k  (= sum_k dp_k G_k, G_k = U_k[:, :C] W_k)                   dx = A_hat^T dAx

Parameters carry the cell's own names (``conv_z.lin.weight`` (C, F), ``conv_z.bias`` (C), ``linear_z.weight`` (C, 2C), ``linear_z.bias``
(C), likewise r and h); A_hat is a dense (N, N) matrix -- the shapes of the tests are small.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from oracle import graph_ops as G

GATES = ("z", "r", "h")
NAMES = [f"conv_{k}.lin.weight" for k in GATES] + [f"conv_{k}.bias" for k in GATES] + [f"linear_{k}.weight" for k in GATES] + \
        [f"linear_{k}.bias" for k in GATES]


def dense_from_edges(ei: torch.Tensor, ew: Optional[torch.Tensor], n: int, dtype=torch.float64) -> torch.Tensor:
    """A_hat (N, N) from the oracle's gcn_norm in ``dtype``: row = target, column = source."""
    src, dst, w = G.gcn_norm_edges(ei, None if ew is None else ew.to(dtype), n, dtype)
    a = torch.zeros(n, n, dtype=dtype)
    a.index_put_((dst, src), w, accumulate=True)
    return a


def dense_from_csr(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, n: int, dtype=torch.float64) -> torch.Tensor:
    """A_hat (N, N) from a prepared operator's own CSR (the normalisation is not under test where this is used)."""
    rp = rowptr.long().cpu()
    rows = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    a = torch.zeros(n, n, dtype=dtype)
    a.index_put_((rows, col.long().cpu()), val.cpu().to(dtype), accumulate=True)
    return a


def step(p: Dict[str, torch.Tensor], a: torch.Tensor, x: torch.Tensor, h: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
    """{"out": h', and what the backward reads}; ``h`` None = zeros."""
    c = p["conv_z.bias"].numel()
    if h is None:
        h = torch.zeros(x.shape[0], c, dtype=x.dtype)
    ax = a @ x
    conv = {k: ax @ p[f"conv_{k}.lin.weight"].t() + p[f"conv_{k}.bias"] for k in GATES}
    z = torch.sigmoid(torch.cat([conv["z"], h], 1) @ p["linear_z.weight"].t() + p["linear_z.bias"])
    r = torch.sigmoid(torch.cat([conv["r"], h], 1) @ p["linear_r.weight"].t() + p["linear_r.bias"])
    q = h * r
    ht = torch.tanh(torch.cat([conv["h"], q], 1) @ p["linear_h.weight"].t() + p["linear_h.bias"])
    return {"out": z * h + (1 - z) * ht, "ax": ax, "conv": conv, "z": z, "r": r, "q": q, "ht": ht, "h": h}


def backward(p: Dict[str, torch.Tensor], a: torch.Tensor, s: Dict, d: torch.Tensor):
    """(dx (N, F), dh (N, C), {name: gradient}) from the step's record ``s`` and d = dL/dh'."""
    c = p["conv_z.bias"].numel()
    z, r, q, ht, h, ax, conv = s["z"], s["r"], s["q"], s["ht"], s["h"], s["ax"], s["conv"]
    dp = {"h": d * (1 - z) * (1 - ht * ht), "z": d * (h - ht) * (z * (1 - z))}
    dq = dp["h"] @ p["linear_h.weight"][:, c:]
    dp["r"] = dq * h * (r * (1 - r))
    dh = d * z + dq * r + dp["z"] @ p["linear_z.weight"][:, c:] + dp["r"] @ p["linear_r.weight"][:, c:]
    g: Dict[str, torch.Tensor] = {}
    dax = torch.zeros_like(ax)
    for k in GATES:
        right = q if k == "h" else h
        g[f"linear_{k}.weight"] = dp[k].t() @ torch.cat([conv[k], right], 1)
        g[f"linear_{k}.bias"] = dp[k].sum(0)
        dconv = dp[k] @ p[f"linear_{k}.weight"][:, :c]
        g[f"conv_{k}.lin.weight"] = dconv.t() @ ax
        g[f"conv_{k}.bias"] = dconv.sum(0)
        dax = dax + dconv @ p[f"conv_{k}.lin.weight"]
    return a.t() @ dax, dh, g


def unroll(p: Dict[str, torch.Tensor], a: torch.Tensor, xs, h0: torch.Tensor):
    """H_t = cell(xs[t], H_{t-1}) from h0, loss (H_last ** 2).sum(): (H_last, dh0, [dx_t], {name: gradient}) by the hand-written backward."""
    recs, h = [], h0
    for x in xs:
        recs.append(step(p, a, x, h))
        h = recs[-1]["out"]
    d = 2 * h
    dxs, grads = [None] * len(xs), {n: torch.zeros_like(p[n]) for n in NAMES}
    for t in range(len(xs) - 1, -1, -1):
        dxs[t], d, g = backward(p, a, recs[t], d)
        for n in NAMES:
            grads[n] = grads[n] + g[n]
    return h, d, dxs, grads
