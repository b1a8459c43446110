"""References, fp32 restatement and bar of the window sum's backward (csrc/window_bwd.hip, regt_window_backward).  Test helper only.

The entry point takes ``ring``, the forward's ``hidden`` and ``dpred``; it runs the head's backward, which leaves dhidden, and then

    dring[slot(j)] (+)= sum_{w : 0 <= j - w < T} prob[j - w] * dhidden[w]          slot(j) = (first_slot + j) % ring_len
    d_attention    (+)= prob * (dprob - sum_q prob[q] dprob[q]),   dprob[p] = sum_{w, n, c} dhidden[w, n, c] * ring[slot(w + p), n, c]

Float64 reference (``reference64``): autograd through ``window_bars.reference64`` plus the head, L = sum(pred * dpred), with the
``hidden`` the call is given taken in place of the window sum's value (two stages: the head's backward on the given hidden, exactly --
its zeros decide ReLU masks --, then dhidden pushed through the window sum to ring and attention).  It returns dring, d_attention, the four head gradients, dhidden and the
statistic's denominator sum |terms| (+ |carried value| under accumulate).

Inputs (``inputs``).  ring and attention are window_bars.inputs'.  The head and everything that feeds it are chosen so that the head's
backward is EXACT in fp32 whatever the summation order: ``hidden`` in multiples of 1/4, linear1 in multiples of 1/8, linear2 and
``dpred`` in multiples of 1/4 and 1/8, every partial sum a multiple of 2^-8 below 2^15.  So dhidden on the device IS float32(dhidden64)
and the bar of dring measures the adjoint kernel alone, as window_bars' measures the forward kernel alone on an exact ring; the head's
weight gradients are still held to op_bars' wgrad bars (which they then meet exactly), and d_attention -- a dot product with the
real-valued ring -- to grad_bars.REL["attention"].  The end-to-end gradients on real weights are tests/test_gpu_stream_train.py's.

The fp32 RESTATEMENT (``restatement32``) follows the kernel's stated order: window_bars.softmax32, then every covered slot's accumulator
starts from the value dring holds (accumulate) or from 0 and receives its windows in ASCENDING window order, one fused multiply-add
each (window_bars._fma32).  d_attention is restated as fp32 dot products and the fp32 softmax backward.

Bar of dring, derived exactly as window_bars.bar_table: 4 x the restatement's worst ratio against sum |terms| over CASES, rounded up to
a power of two, capped by grad_bars.CAP["default"].  tests/test_window_bwd_cpu.py recomputes the table on the host;
profiles/window_bwd_bars.txt holds it:

    case (N, C, T, ring_len, first_slot, windows)      worst restatement r
    (7, 16, 1, 1, 0, 1)                                4.88e-08
    (7, 16, 6, 6, 4, 1)                                1.55e-07
    (129, 132, 12, 12, 11, 1)                          3.28e-07
    (43, 256, 12, 40, 3, 29)                           3.31e-07
    (5, 128, 17, 64, 0, 48)                            2.64e-07
    (3, 64, 4, 9, 0, 6)                                1.92e-07
    (3, 8, 5, 21, 2, 17)                               9.37e-08
    (3, 8, 6, 10, 7, 3)                                1.04e-07
    (3, 8, 5, 20, 18, 12)                              1.65e-07
    (3, 8, 5, 21, 2, 13)                               1.47e-07
    (2, 16, 32, 40, 9, 5)                              2.04e-07
    worst 3.31e-07  x 4, rounded up: 2 ** -19 (1.91e-06)

The value comes from the restatement on the CPU, never from the kernel's output.  Planted corruptions (``corrupt=``): the first window
of a slot dropped, ``prob`` indexed by p + 1, the accumulator started from 0 despite ``accumulate``, the slot index not wrapped (a slot
past the ring is never written), the softmax backward's mean term missing.  Each breaks its bar on at least one case.
"""
from __future__ import annotations

import math

import torch

import grad_bars
import op_bars
import window_bars as W

MAX_T = 32       # regt_window_backward_max_t(), checked by tests/test_window_bwd_cpu.py
WC = W.WC
H1, O = 128, 3

# (N, C, T, ring_len, first_slot, windows): window_bars.CASES within the backward's T limit, then the backward's own edges
CASES = [c for c in W.CASES if c[2] <= MAX_T] + [
    (3, 8, 6, 10, 7, 3),                 # windows < T, wrapping
    (3, 8, 5, 20, 18, WC - 4),           # windows + T - 1 == WC: one full chunk of slots
    (3, 8, 5, 21, 2, WC - 3),            # windows + T - 1 == WC + 1: a full chunk and a chunk of one
    (2, 16, 32, 40, 9, 5),               # T at the limit
]
CORRUPTIONS = ("drop_first", "prob_shift", "no_carry", "no_wrap", "no_mean")
BAR_DRING = min(2.0 ** -19, grad_bars.CAP["default"])


def inputs(case, seed: int = 0):
    """dict: ring, att (window_bars.inputs), hidden (windows, N, C), dpred (windows, N, O), the head l1w, l1b, l2w, l2b and ``carried``
    (ring_len, N, C), what dring holds before an accumulating call; fp32 on the CPU."""
    n, c, t, ring_len, _, windows = case
    ring, att = W.inputs(case, seed)
    g = torch.Generator().manual_seed(4000 + seed + 5 * n + 11 * c + 29 * t + ring_len + 3 * windows)
    q = lambda shape, lo, hi, div: torch.randint(lo, hi + 1, shape, generator=g).float() / div
    return {"ring": ring, "att": att, "hidden": q((windows, n, c), -8, 8, 4.0), "dpred": q((windows, n, O), -8, 8, 8.0),
            "l1w": q((H1, c), -4, 4, 8.0), "l1b": q((H1,), -4, 4, 8.0), "l2w": q((O, H1), -4, 4, 4.0), "l2b": q((O,), -4, 4, 4.0),
            "carried": torch.randn(ring_len, n, c, generator=g)}


def covered(case):
    """Ring slots of the windows + T - 1 covered steps, in step order."""
    _, _, t, ring_len, first, windows = case
    return (first + torch.arange(windows + t - 1)) % ring_len


def reference64(x, case, accumulate: bool = False):
    """dict of float64 tensors: dring (ring_len, N, C; untouched slots hold ``carried`` under accumulate, else 0), den (same shape),
    d_att, d_l1w, d_l1b, d_l2w, d_l2b, dhidden."""
    n, c, t, ring_len, first, windows = case
    leaf = {k: x[k].double().requires_grad_(True) for k in ("ring", "att", "l1w", "l1b", "l2w", "l2b")}
    hidden = x["hidden"].double().requires_grad_(True)                        # the given hidden, exactly (its zeros decide ReLU masks)
    y1 = torch.relu(torch.relu(hidden) @ leaf["l1w"].t() + leaf["l1b"])
    pred = y1 @ leaf["l2w"].t() + leaf["l2b"]
    (pred * x["dpred"].double()).sum().backward()
    dh = hidden.grad
    summed, _ = W.reference64(leaf["ring"], leaf["att"], case)
    (summed * dh).sum().backward()                                            # ... and the window sum's gradient path behind it
    prob = torch.softmax(x["att"].double(), dim=0)
    den = torch.zeros(ring_len, n, c, dtype=torch.float64)
    sl = W.slots(case)
    for w in range(windows):
        for p in range(t):
            den[sl[w, p]] += (prob[p] * dh[w]).abs()
    dring = leaf["ring"].grad.clone()
    if accumulate:
        cov = covered(case)
        dring = x["carried"].double().clone()
        dring[cov] += leaf["ring"].grad[cov]
        den[cov] += x["carried"].double()[cov].abs()
    return {"dring": dring, "den": den, "d_att": leaf["att"].grad, "d_l1w": leaf["l1w"].grad, "d_l1b": leaf["l1b"].grad,
            "d_l2w": leaf["l2w"].grad, "d_l2b": leaf["l2b"].grad, "dhidden": dh}


def restatement32(x, dhidden64, case, accumulate: bool = False, corrupt=None):
    """(dring (ring_len, N, C), d_att (T)) in the kernels' stated fp32 arithmetic on the CPU; slots the call does not cover keep
    ``carried`` (accumulate) or NaN.  ``corrupt``: one of CORRUPTIONS."""
    n, c, t, ring_len, first, windows = case
    dh = dhidden64.float()
    assert torch.equal(dh.double(), dhidden64), "the head's backward is not exact on these inputs"
    prob = torch.cat([W.softmax32(x["att"]), torch.zeros(1)])
    out = x["carried"].clone() if accumulate else torch.full((ring_len, n, c), float("nan"))
    for j in range(windows + t - 1):
        s = first + j
        if corrupt == "no_wrap" and s >= ring_len:
            continue
        s %= ring_len
        acc = x["carried"][s].clone() if accumulate and corrupt != "no_carry" else torch.zeros(n, c)
        ws = [w for w in range(windows) if 0 <= j - w < t]
        for w in (ws[1:] if corrupt == "drop_first" else ws):
            p = j - w
            acc = W._fma32(prob[p + 1] if corrupt == "prob_shift" else prob[p], dh[w], acc)
        out[s] = acc
    sl = W.slots(case)
    dprob = torch.stack([(dh * x["ring"][sl[:, p]]).sum(dtype=torch.float32) for p in range(t)])
    pr = prob[:t]
    mean = torch.zeros(()) if corrupt == "no_mean" else (pr * dprob).sum()
    return out, pr * (dprob - mean)


def dring_ratio(got, ref, case) -> float:
    """The statistic over the covered slots; every other slot must be bit-identical to the reference's (untouched)."""
    cov = covered(case)
    return op_bars._ratio((got[cov].double() - ref["dring"][cov]).abs(), ref["den"][cov])


def att_ratio(d_att, ref) -> float:
    """max |d_att - want64| / max |want64|, held to grad_bars.REL["attention"]."""
    scale = float(ref["d_att"].abs().max())
    err = float((d_att.double() - ref["d_att"]).abs().max())
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


def bar_table():
    """[(case, worst restatement r)] over both accumulate settings, and the bar they give."""
    rows = []
    for case in CASES:
        x = inputs(case)
        worst = 0.0
        for acc in (False, True):
            ref = reference64(x, case, acc)
            worst = max(worst, dring_ratio(restatement32(x, ref["dhidden"], case, acc)[0], ref, case))
        rows.append((case, worst))
    top = max(r for _, r in rows)
    return rows, min(2.0 ** math.ceil(math.log2(op_bars.ORDER_FACTOR * top)), grad_bars.CAP["default"])


def head_operands(x):
    """(relu(hidden), y1, d1) in float64, rows flattened: the operands of the head's two weight gradients, dW1 = d1^T relu(hidden) and
    dW2 = dpred^T y1 (exactly representable in fp32 on these inputs)."""
    c = x["hidden"].shape[-1]
    a1 = torch.relu(x["hidden"].double()).reshape(-1, c)
    z1 = a1 @ x["l1w"].double().t() + x["l1b"].double()
    y1 = torch.relu(z1)
    d1 = (x["dpred"].double().reshape(-1, O) @ x["l2w"].double()) * (z1 > 0)
    return a1, y1, d1
