"""Gradient bars relative to each tensor's OWN scale.

Test helper only (like fused_math.py).  The parity tests of the whole backward pass compare with
``assert_allclose(..., atol=1e-5, rtol=1e-4)``; the losses are means over n x o predictions, so the gradients of the reset
gate, of the attention vector and of the Chebyshev ``lins.1`` weight at many regions have maxima of 1e-5 .. 1e-4 and that
``atol`` alone decides the assertion (it accepts errors of 15 .. 70 % of such a tensor's scale).  Here every block that a
separate launch produces is held to

    max|got - want64| <= REL[class] * max|want64_block|

where ``want64`` is the float64 oracle gradient.  A block whose float64 gradient is exactly zero (the dead reset gate of the
zero-hidden models) must be exactly zero.

Blocks (``grad_blocks``): ``linear_{z,r,h}.weight`` (C, 2C) splits into its column halves (the conv half and the hidden half
come from different launches and differ in scale by ~100x); ``tgnn.linear.weight`` (C, R*C) splits into its R region
blocks; everything else is one block.

Classes: ``attention`` (the softmax backward of ``_attention`` is a difference of nearly equal sums over all n x C hidden
elements, so its fp32 error relative to the RESULT is larger than that of a plain dot product) and ``default``.

    REL = {"default": 2 ** -15 (3.05e-5), "attention": 2 ** -14 (6.10e-5)}

How they were set: the worst ratio max|hip - want64| / max|want64| measured on the MI355X over every case and block of
tests/test_gpu_grad_scale.py, under both fp32-storage arithmetics and every switch setting, times 4 (chunk and tile
boundaries move with the CU count and the slab sizing between shapes), rounded up to a power of two.
profiles/grad_scale_bars.txt is that table (tools/grad_scale_bars.py writes it), with the fp32 oracle's own ratio next to
every entry:

    default    worst 6.0e-6  (linear_r.weight conv half, trained checkpoint on the fixture, bf16x3)   x 4 -> 2 ** -15
    attention  worst 1.13e-5 (1500 nodes x 12 periods, bf16x3, two-launch cell backward)              x 4 -> 2 ** -14

(the fp32 oracle itself: 2.6e-6 and 1.11e-5).  Independent of any measurement the values are capped -- default <= 1e-4,
attention <= 1e-3: a missing or mis-signed term moves a block by >= 1 % of its scale -- they are the same for both
arithmetics, and no block is skipped or down-weighted.  No tensor needed a class beyond these two.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Tuple

import torch

REL = {"default": 2.0 ** -15, "attention": 2.0 ** -14}
assert REL["default"] <= 1e-4 and REL["attention"] <= 1e-3

_GATE_LINEAR = re.compile(r"(^|\.)linear_[zrh]\.weight$")


def grad_class(name: str) -> str:
    return "attention" if name.endswith("_attention") else "default"


def grad_blocks(name: str, tensor: torch.Tensor, num_regions: Optional[int] = None) -> List[Tuple[str, torch.Tensor]]:
    """[(label, view)]: the blocks of one gradient that separate launches produce."""
    if tensor.dim() == 2 and _GATE_LINEAR.search(name) and tensor.shape[1] == 2 * tensor.shape[0]:
        c = tensor.shape[0]
        return [(f"{name}[:, :C] (conv half)", tensor[:, :c]), (f"{name}[:, C:] (hidden half)", tensor[:, c:])]
    if name == "tgnn.linear.weight" and tensor.dim() == 2:
        c = tensor.shape[0]
        r = tensor.shape[1] // c if num_regions is None else num_regions
        assert r * c == tensor.shape[1], (name, tuple(tensor.shape), num_regions)
        if r > 1:
            return [(f"{name}[:, region {k}]", tensor[:, k * c:(k + 1) * c]) for k in range(r)]
    return [(name, tensor)]


def block_ratios(got: Dict[str, Optional[torch.Tensor]], want64: Dict[str, Optional[torch.Tensor]], num_regions: Optional[int] = None):
    """[(name, label, class, err, scale)] over every block of every tensor that has a gradient in `want64`."""
    rows = []
    for name, want in want64.items():
        if want is None:
            continue
        g = got[name]
        assert g is not None, f"{name}: no gradient where the oracle has one"
        w = want.detach().cpu().double()
        g = g.detach().cpu().double()
        assert g.shape == w.shape, (name, tuple(g.shape), tuple(w.shape))
        for (label, gb), (_, wb) in zip(grad_blocks(name, g, num_regions), grad_blocks(name, w, num_regions)):
            rows.append((name, label, grad_class(name), float((gb - wb).abs().max()), float(wb.abs().max())))
    return rows


def assert_grads_to_scale(got, want64, rel=REL, what: str = "", num_regions: Optional[int] = None):
    """`got`, `want64`: dict name -> gradient (None = no gradient).  Every block of every tensor within rel[class] of its own
    scale; exactly zero where the float64 gradient is; no gradient where the oracle has none."""
    bad = []
    for name, want in want64.items():
        if want is None:
            g = got.get(name)
            if g is not None and float(g.abs().max()) != 0.0:
                bad.append(f"{name}: a gradient (max {float(g.abs().max()):.3e}) where the oracle has none")
    for name, label, cls, err, scale in block_ratios(got, want64, num_regions):
        if not err <= rel[cls] * scale:              # (NaN fails; scale 0 demands err 0)
            ratio = err / scale if scale > 0 else float("inf")
            bad.append(f"{label} [{cls}]: max|err| {err:.3e} vs scale {scale:.3e}: ratio {ratio:.3e} > {rel[cls]:.3e}")
    assert not bad, f"{what}: {len(bad)} gradient block(s) off their own scale:\n  " + "\n  ".join(bad)
