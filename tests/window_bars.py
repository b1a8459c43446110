"""Per-element bar for the attention-weighted window sum over a ring of cell outputs (csrc/window.hip, regt_window_forward).

Test helper only (like op_bars.py).  For ONE output element the statistic is that of op_bars.py,

    r = |got - want64| / sum_p |prob_p * ring[(first_slot + w + p) % ring_len, n, c]|

with ``want64`` and the probabilities formed in float64 from the same fp32 inputs (softmax of the fp32 logits in float64).  An all-zero
denominator demands an exact 0, a NaN fails (op_bars._ratio).

The fp32 RESTATEMENT follows the kernel's stated order: the softmax as the library's small launch computes it (fp32 max, exp of the
difference summed in index order, one division per entry), then every element accumulated p = 0, 1, .., T - 1 with a fused
multiply-add, starting from 0.  The fused multiply-add is emulated as float32(float64(prob) * float64(value) + float64(acc)): the
product is exact in float64, and the second rounding can differ from a true fma only where the float64 sum lies within 2^-29 of an fp32
rounding boundary -- by one ulp, far below what the bar measures.

Bar.  4 x the worst r of the restatement over CASES (4: the allowance of op_bars.py), rounded up to a power of two, capped by
grad_bars.CAP["default"].  tests/test_window_bars_cpu.py recomputes the table on the host; profiles/window_bars.txt holds it:

    case (N, C, T, ring_len, first_slot, windows)      worst restatement r
    (7, 16, 1, 1, 0, 1)                                0.00e+00
    (7, 16, 6, 6, 4, 1)                                1.66e-07
    (129, 132, 12, 12, 11, 1)                          3.63e-07
    (43, 256, 12, 40, 3, 29)                           4.08e-07
    (5, 128, 17, 64, 0, 48)                            3.30e-07
    (2, 128, 255, 255, 200, 1)                         3.55e-07
    (3, 64, 4, 9, 0, 6)                                1.53e-07
    (3, 8, 5, 21, 2, 17)                               9.98e-08
    worst 4.08e-07  x 4, rounded up: 2 ** -19 (1.91e-06)

The value comes from the restatement on the CPU, never from the kernel's output.  Planted corruptions (``corrupt=``): the last period
dropped, ``prob`` indexed by p + 1, the slot index not wrapped (a slot past the ring reads nothing), window 1 of a chunk taking window
0's accumulator.  Each exceeds the bar on at least one case (tests/test_window_bars_cpu.py).

Inputs: ring values are randn scaled per slot by a power of two between 2^-4 and 2^4, attention logits uniform in [-3, 3].

The head's bar (``pred_ratio``).  pred = W2 relu(W1 relu(hidden) + b1) + b2 is two linear layers on the window sum.  With
den_h the statistic's denominator of hidden, den_1 = relu(|hidden64|) |W1|^T + |b1| and den_2 = y1_64 |W2|^T + |b2| (op_bars'
linear denominators on the float64 activations), relu being 1-Lipschitz, an implementation whose layers each meet their bar is within

    BAR["linear"] * (den_2 + den_1 |W2|^T)  +  BAR_WINDOW * (den_h |W1|^T) |W2|^T

of the float64 head on the float64 hidden; ``pred_ratio`` is the error over that allowance and must stay <= 1.  This is wider than
op_bars.linear_ratio's bar applied to the last layer alone (BAR["linear"] * den_2): the entry point hands out neither y1 nor a hidden
that is exact, so the bar of each stage is carried through the layers behind it.
"""
from __future__ import annotations

import math

import torch

import grad_bars
import op_bars

WC = 16      # windows per thread of the chunked kernel: regt_window_chunk(2), checked by tests/test_stream_cpu.py

# (N, C, T, ring_len, first_slot, windows)
CASES = [
    (7, 16, 1, 1, 0, 1),                 # T = 1
    (7, 16, 6, 6, 4, 1),                 # a single window wrapping mid-window
    (129, 132, 12, 12, 11, 1),           # ragged tile, C % 4
    (43, 256, 12, 40, 3, 29),            # windows > 2 T
    (5, 128, 17, 64, 0, 48),
    (2, 128, 255, 255, 200, 1),          # T = 255
    (3, 64, 4, 9, 0, 6),                 # windows + T - 1 == ring_len exactly
    (3, 8, 5, 21, 2, WC + 1),            # windows == WC + 1: a full chunk and a chunk of one
]
CORRUPTIONS = ("drop_last", "prob_shift", "no_wrap", "neighbour_acc")
BAR_WINDOW = min(2.0 ** -19, grad_bars.CAP["default"])


def inputs(case, seed: int = 0):
    """(ring (ring_len, N, C), attention (T)) fp32 on the CPU."""
    n, c, t, ring_len, _, _ = case
    g = torch.Generator().manual_seed(1000 + seed + 7 * n + 13 * c + 31 * t + ring_len)
    scale = 2.0 ** torch.randint(-4, 5, (ring_len, 1, 1), generator=g).float()
    ring = torch.randn(ring_len, n, c, generator=g) * scale
    att = torch.rand(t, generator=g) * 6.0 - 3.0
    return ring.contiguous(), att


def slots(case):
    """(windows, T) ring slot of period p of window w."""
    _, _, t, ring_len, first, windows = case
    w = torch.arange(windows).view(-1, 1)
    p = torch.arange(t).view(1, -1)
    return (first + w + p) % ring_len


def reference64(ring, att, case):
    """(want64 (windows, N, C), sum_p |prob_p ring term|) in float64."""
    prob = torch.softmax(att.double(), dim=0)
    terms = prob.view(1, -1, 1, 1) * ring.double()[slots(case)]           # (windows, T, N, C)
    return terms.sum(dim=1), terms.abs().sum(dim=1)


def softmax32(att):
    """The library's small softmax launch in fp32: max, exp(x - max) summed in index order, one division per entry."""
    att = att.float()
    mx = att.max()
    e = torch.exp(att - mx)
    s = torch.zeros((), dtype=torch.float32)
    for v in e:
        s = s + v
    return e / s


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def restatement32(ring, att, case, corrupt=None):
    """The kernel's stated arithmetic in fp32 on the CPU; ``corrupt``: one of CORRUPTIONS."""
    _, _, t, ring_len, first, windows = case
    prob = torch.cat([softmax32(att), torch.zeros(1)])
    acc = torch.zeros(windows, *ring.shape[1:], dtype=torch.float32)
    w = torch.arange(windows)
    for p in range(t - 1 if corrupt == "drop_last" else t):
        s = first + w + p
        pr = prob[p + 1] if corrupt == "prob_shift" else prob[p]
        if corrupt == "no_wrap":
            v = torch.where((s < ring_len).view(-1, 1, 1), ring[s.clamp_max(ring_len - 1)], torch.zeros(()))
        else:
            v = ring[s % ring_len]
        acc = _fma32(pr, v, acc)
    if corrupt == "neighbour_acc" and windows > 1:
        acc[1] = acc[0]
    return acc


def ratio(got, want64, den) -> float:
    return op_bars._ratio((got.double() - want64).abs(), den)


def bar_table():
    """[(case, worst restatement r)] and the bar they give."""
    rows = []
    for case in CASES:
        ring, att = inputs(case)
        want, den = reference64(ring, att, case)
        rows.append((case, ratio(restatement32(ring, att, case), want, den)))
    worst = max(r for _, r in rows)
    return rows, min(2.0 ** math.ceil(math.log2(op_bars.ORDER_FACTOR * worst)), grad_bars.CAP["default"])


def head_inputs(c: int, h1: int = 128, o: int = 3, seed: int = 0):
    g = torch.Generator().manual_seed(77 + seed + c)
    return (torch.randn(h1, c, generator=g) / math.sqrt(c), torch.randn(h1, generator=g) * 0.1,
            torch.randn(o, h1, generator=g) / math.sqrt(h1), torch.randn(o, generator=g) * 0.1)


def pred_ratio(pred, want64, den_h, l1w, l1b, l2w, l2b) -> float:
    """max |pred - head64(want64)| over the allowance derived in the module docstring (<= 1 passes).  ``want64``, ``den_h``: the
    float64 hidden and its denominator, (rows, C)."""
    w1, b1, w2, b2 = (x.double() for x in (l1w, l1b, l2w, l2b))
    a1 = torch.relu(want64)
    y1 = torch.relu(a1 @ w1.t() + b1)
    den1 = a1 @ w1.abs().t() + b1.abs()
    want = y1 @ w2.t() + b2
    den2 = y1 @ w2.abs().t() + b2.abs()
    allow = op_bars.BAR["linear"] * (den2 + den1 @ w2.abs().t()) + BAR_WINDOW * ((den_h @ w1.abs().t()) @ w2.abs().t())
    return op_bars._ratio((pred.double() - want).abs(), allow)
