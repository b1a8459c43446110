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
arithmetics, and no block is skipped or down-weighted.  No tensor of the RegT-GCN path needed a class beyond these two.

The baselines (STNorm, STID, SpatialGCN; ``assert_grads_conditioned``).  Their parity tests carried the same absolute 1e-5
(13 % of the scale of STNorm's ``tn.6.beta`` on the in12_out3 golden) and held the restatement cases to the whole tensor's
maximum.  Blocks: STID ``node_emb`` by 64-node tile (the ragged last tile is a block of its own), ``time_series_emb_layer.weight``
by input step (``input_dim`` columns each), the 64 x 64 ``fc1`` / ``fc2`` and ``regression_layer`` weights by the 32 x 32
quadrant one wave accumulates; STNorm ``filter_convs`` / ``gate_convs`` weights by kernel tap and by 16-channel slice of
z = [x | TNorm(x) | SNorm(x)], ``tn.*.gamma`` / ``beta`` (per node) by wave of 64 nodes; SpatialGCN ``gcn.lins.0`` and
``gcn.lins.1`` (tensors of their own) by 16-feature accumulator.  One more class, ``norm``: STNorm's ``tn.*`` / ``sn.*``
parameters and every convolution whose gradient comes back through a normalisation's backward (``start_conv``, ``filter_convs``,
``gate_convs``, ``residual_convs``): there 1 / sqrt(var + 1e-5) multiplies the rounding of the reductions.  Everything else of
the three models is a plain dot product and keeps ``default``.

Ill-conditioned blocks are named, never skipped.  Conditioning is decided by the references alone: a block is ill-conditioned
when the fp32 restatement's own max|g32 - g64| exceeds CAP[class] / 4 of max|g64| of that block (``ill_conditioned``) -- the
case the STNorm tests' docstring records, SNorm's spread 0 under equal start_conv biases, and a ReLU that fp32 and float64 take
differently.  Such a block is held to K x max|g32 - g64| of the block (K = 4, the summation-order allowance those tests already
use) with no absolute floor, and the assertion returns their labels: none in any golden, at most 5 % of the blocks of a test
file (tests/test_baseline_bars_cpu.py proves both on the host, with the fp32 restatement in the kernels' place).

    REL["norm"] = 2 ** -10 (9.77e-4, cap 1e-3); the baselines' dot products stay in "default" (2 ** -15, cap 1e-4)

How they were set: the worst ratio max|hip - want64| / max|want64| over the well-conditioned blocks of every case of the three
test files on the MI355X, times 4, rounded up to a power of two (profiles/baseline_grad_bars.txt, tools/baseline_grad_bars.py
writes it, the fp32 restatement's own ratio next to every entry):

    default  worst 4.01e-6 (STID regression_layer.bias, n 104 b 2 l 1), 2.26e-6 (STID encoder.2.fc2.bias, same case)      x 4 -> 2 ** -15
    norm     worst 2.11e-4 (STNorm residual_convs.6.bias, n 130 b 1 t 12), 1.99e-4 (residual_convs.5.bias, same case)   x 4 -> 2 ** -10

(the fp32 restatement itself, in that run: 9.3e-7, 1.4e-6, 5.3e-5, 5.0e-5).  The first measurement had start_conv.bias at
T = 3, B = 2 on top with 2.75e-4 (fp32 restatement 6.6e-5), which x 4 is over the cap: there left padding makes SNorm's
1 / sqrt(var + 1e-5) = 316, the bias gradient is a sum of large cancelling terms, and op_accumulate of csrc/stnorm.hip carried one
running sum through all B x L x 64 rows.  It now adds each column's rows in four interleaved partial sums combined pairwise; the
block went to 9.5e-5 and left the list, the gradients stay bit-reproducible.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Tuple

import torch

REL = {"default": 2.0 ** -15, "attention": 2.0 ** -14, "norm": 2.0 ** -10}
CAP = {"default": 1e-4, "attention": 1e-3, "norm": 1e-3}          # what REL may never exceed, whatever was measured
assert all(REL[c] <= CAP[c] for c in REL)

_GATE_LINEAR = re.compile(r"(^|\.)linear_[zrh]\.weight$")
# STNorm: the normalisation parameters, and every convolution whose gradient comes back through a TNorm / SNorm backward
_NORM = re.compile(r"^((tn|sn)\.\d+\.(gamma|beta)|(start_conv|(filter|gate|residual)_convs\.\d+)\.(weight|bias))$")
_ST_GATED = re.compile(r"^(filter|gate)_convs\.\d+\.weight$")
_ST_TNORM = re.compile(r"^tn\.\d+\.(gamma|beta)$")
_STID_FC = re.compile(r"^encoder\.\d+\.fc[12]\.weight$")
_SPATIAL_LIN = re.compile(r"^gcn\.lins\.[01]\.weight$")
NODE_TILE = 64          # nodes per tile of csrc/stid.hip and per wave of csrc/stnorm.hip
HALF = 32               # a wave's quadrant of stid.hip's 64 x 64 results
SPATIAL_KB = 16         # feature columns per accumulator of csrc/spatial.hip
ST_CHANNELS = 16        # channels of one slice of STNorm's z = [x | TNorm(x) | SNorm(x)]


def grad_class(name: str) -> str:
    if name.endswith("_attention"):
        return "attention"
    return "norm" if _NORM.match(name) else "default"


def _chunks(name, tensor, dim, size, what, ragged=None):
    n = tensor.shape[dim]
    out = []
    for a in range(0, n, size):
        b = min(a + size, n)
        tag = f" ({ragged})" if ragged and b - a < size else ""
        out.append((f"{name}[{what} {a}:{b}]{tag}", tensor.narrow(dim, a, b - a)))
    return out


def grad_blocks(name: str, tensor: torch.Tensor, num_regions: Optional[int] = None, input_dim: Optional[int] = None) -> List[Tuple[str, torch.Tensor]]:
    """[(label, view)]: the blocks of one gradient that separate launches, tiles or reduction stages produce."""
    if tensor.dim() == 2 and _GATE_LINEAR.search(name) and tensor.shape[1] == 2 * tensor.shape[0]:
        c = tensor.shape[0]
        return [(f"{name}[:, :C] (conv half)", tensor[:, :c]), (f"{name}[:, C:] (hidden half)", tensor[:, c:])]
    if name == "tgnn.linear.weight" and tensor.dim() == 2:
        c = tensor.shape[0]
        r = tensor.shape[1] // c if num_regions is None else num_regions
        assert r * c == tensor.shape[1], (name, tuple(tensor.shape), num_regions)
        if r > 1:
            return [(f"{name}[:, region {k}]", tensor[:, k * c:(k + 1) * c]) for k in range(r)]
    # STID: node-embedding rows leave the backward kernel tile by tile (64 nodes, the last one ragged); a wave owns a 32 x 32
    # quadrant of every 64 x 64 weight gradient; dWe's columns are (input step, feature) pairs, step-major
    if name == "node_emb" and tensor.dim() == 2:
        return _chunks(name, tensor, 0, NODE_TILE, "nodes", "ragged last tile")
    if name == "time_series_emb_layer.weight" and tensor.dim() == 4:
        return _chunks(name, tensor, 1, input_dim or HALF, "step columns" if input_dim else "columns")
    if (_STID_FC.match(name) or name == "regression_layer.weight") and tensor.dim() == 4:
        return [(f"{lr}{lc}", bc) for lr, br in _chunks(name, tensor, 0, HALF, "out") for lc, bc in _chunks("", br, 1, HALF, "in")]
    # STNorm: the gated convolutions by kernel tap and by slice of z (x, TNorm(x), SNorm(x) differ in scale); TNorm's per-node
    # parameters by wave of 64 nodes
    if _ST_GATED.match(name) and tensor.dim() == 4:
        return [(f"{name}[tap {tap}]{lc}", bc) for tap in range(tensor.shape[3])
                for lc, bc in _chunks("", tensor[..., tap:tap + 1], 1, ST_CHANNELS, "z")]
    if _ST_TNORM.match(name) and tensor.dim() == 4:
        return _chunks(name, tensor, 2, NODE_TILE, "nodes", "ragged last wave")
    # SpatialGCN's first layer: lins.0 and lins.1 are tensors of their own; each 16-feature column group is one accumulator
    if _SPATIAL_LIN.match(name) and tensor.dim() == 2:
        return _chunks(name, tensor, 1, SPATIAL_KB, "features")
    return [(name, tensor)]


def block_ratios(got: Dict[str, Optional[torch.Tensor]], want64: Dict[str, Optional[torch.Tensor]], num_regions: Optional[int] = None,
                 input_dim: Optional[int] = None):
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
        err = (g - w).abs()
        wa = w.abs()
        for (label, eb), (_, wb) in zip(grad_blocks(name, err, num_regions, input_dim), grad_blocks(name, wa, num_regions, input_dim)):
            rows.append((name, label, grad_class(name), float(eb.max()), float(wb.max())))
    return rows


def assert_grads_to_scale(got, want64, rel=REL, what: str = "", num_regions: Optional[int] = None):
    """`got`, `want64`: dict name -> gradient (None = no gradient).  Every block of every tensor within rel[class] of its own
    scale; exactly zero where the float64 gradient is; no gradient where the oracle has none."""
    bad = _unwanted(got, want64)
    for name, label, cls, err, scale in block_ratios(got, want64, num_regions):
        if not err <= rel[cls] * scale:              # (NaN fails; scale 0 demands err 0)
            ratio = err / scale if scale > 0 else float("inf")
            bad.append(f"{label} [{cls}]: max|err| {err:.3e} vs scale {scale:.3e}: ratio {ratio:.3e} > {rel[cls]:.3e}")
    assert not bad, f"{what}: {len(bad)} gradient block(s) off their own scale:\n  " + "\n  ".join(bad)


def _unwanted(got, want64):
    bad = []
    for name, want in want64.items():
        if want is None:
            g = got.get(name)
            if g is not None and float(g.abs().max()) != 0.0:
                bad.append(f"{name}: a gradient (max {float(g.abs().max()):.3e}) where the oracle has none")
    return bad


def conditioned_rows(got, want64, ref32, num_regions: Optional[int] = None, input_dim: Optional[int] = None, allow=None):
    """[(label, class, err, scale, gap, excess)] per block: err = max|got - want64|, gap = max|ref32 - want64| (the fp32
    restatement's own error) and excess = max(|got - want64| - allow), `allow` being an optional elementwise allowance that
    the float64 reference alone derives (the ReLU decisions fp32 may take either way, tests/test_gpu_spatial.py); it is taken
    off the fp32 restatement's error too, which takes such decisions as freely as the kernels."""
    rows = []
    kw = dict(num_regions=num_regions, input_dim=input_dim)
    for name, want in want64.items():
        if want is None:
            continue
        g, r = got[name], ref32[name]
        assert g is not None, f"{name}: no gradient where the oracle has one"
        w = want.detach().cpu().double()
        assert g.shape == w.shape == r.shape, (name, tuple(g.shape), tuple(w.shape), tuple(r.shape))
        err = (g.detach().cpu().double() - w).abs()
        gap = (r.detach().cpu().double() - w).abs()
        if allow is not None and allow.get(name) is not None:       # the allowance explains the fp32 restatement's decisions as well
            al = allow[name].double().reshape(err.shape)
            exc, gap = err - al, (gap - al).clamp_min(0.0)
        else:
            exc = err
        for (label, eb), (_, wb), (_, gb), (_, xb) in zip(grad_blocks(name, err, **kw), grad_blocks(name, w.abs(), **kw),
                                                          grad_blocks(name, gap, **kw), grad_blocks(name, exc, **kw)):
            rows.append((label, grad_class(name), float(eb.max()), float(wb.max()), float(gb.max()), float(xb.max())))
    return rows


def ill_conditioned(cls: str, scale: float, gap: float) -> bool:
    """Decided by the references alone: the fp32 restatement's own error takes more than a quarter of the class's cap."""
    return scale > 0.0 and gap > CAP[cls] / 4 * scale


def assert_grads_conditioned(got, want64, ref32, k_gap: float, rel=REL, what: str = "", num_regions: Optional[int] = None,
                             input_dim: Optional[int] = None, allow=None) -> Tuple[List[str], int]:
    """The scaled assertion with the ill-conditioned blocks named.  `ref32`: the gradients of the same restatement that gave
    `want64`, evaluated in fp32.  A well-conditioned block is held to rel[class] * max|want64_block|; an ill-conditioned one
    (`ill_conditioned`) to k_gap * max|ref32 - want64| of that block with no absolute floor; a block that is exactly zero in
    float64 must be exactly zero; no gradient where the oracle has none.  Returns (labels of the ill-conditioned blocks,
    number of blocks) so that the caller can assert on them."""
    bad, ill = _unwanted(got, want64), []
    rows = conditioned_rows(got, want64, ref32, num_regions, input_dim, allow)
    for label, cls, err, scale, gap, excess in rows:
        if ill_conditioned(cls, scale, gap):
            ill.append(label)
            if not excess <= k_gap * gap:
                bad.append(f"{label} [{cls}, ill-conditioned: fp32 restatement off by {gap / scale:.3e} of scale]: max|err| {err:.3e} > "
                           f"{k_gap} x {gap:.3e}")
        elif not excess <= rel[cls] * scale:         # (NaN fails; scale 0 demands err 0)
            ratio = err / scale if scale > 0 else float("inf")
            bad.append(f"{label} [{cls}]: max|err| {err:.3e} vs scale {scale:.3e}: ratio {ratio:.3e} > {rel[cls]:.3e}")
    assert not bad, f"{what}: {len(bad)} gradient block(s) off their own scale:\n  " + "\n  ".join(bad[:40])
    return ill, len(rows)
