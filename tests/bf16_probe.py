"""Per-row and per-node bars for the bf16 arithmetic (regt_set_gemm_mode(2), BASELINE configs[4]) of the whole model step: the kernels
that exist only for it -- fused_fwd / fused_bwd_kernel (csrc/fused.hip), csrc/fused_rows.hip, cell_bwd8_kernel, the bf16-stored epilogues
of dgrad1 / dgrad2 (gemm_cell.hip), wgrad_bf16.hip and the bf16-row SpMM forms as the step uses them -- against float64 ALONE.

Test helper only (like cell_probe.py): pure torch, importable on the CPU.

Statistics (u = 2 ** -9, the unit roundoff of bf16).  ``hidden`` and ``pred`` per node row:

    ratio_n = max_c |got[n, c] - want64[n, c]| / max_c |want64[n, c]|

Parameter gradients under a NODE-LOCALISED upstream gradient: loss = (hidden * gh).sum() + (pred * gp).sum() with gh, gp nonzero on one
probe node only, so every parameter gradient is that node's T rows of dhp / dzp|drp / ds and nothing else -- a wrong tail row, a node
across a tile edge, a lost K slab or a dropped period of that node cannot hide among 18 000 other rows.  Per probe node and tensor:

    ratio = max |got - want64| / max |want64|

Probe nodes of every case (``probe_nodes``): node 0, the last node, the node whose rows straddle row 128, a node in the partial last
128-row tile, the first node of the second region, a node without in-edge (the last two nodes of every case receive no edge).  The probe
on the node without in-edge carries gp = 0: there the float64 gradients of linear1 / linear2 are exactly 0 and the device's must be too.
The same per-tensor statistic is taken once more under a dense upstream gradient (classes ``*_dense``).  ``tgnn._attention`` is a class
of its own: the softmax backward is a difference of nearly equal terms.  A row or tensor that is all 0 in float64 must be exactly 0;
a NaN fails.

References.  ``want64``: the oracle (oracle.model.regional_temporal_gcn / temporal_gcn) in float64 under autograd.  ``emu``: the same
computation in fp32 with bf16 rounding at exactly the places the docstring of tests/test_gpu_bf16.py lists, built from
fused_math.forward_fused(rnd, store, round_x): both operands of every GEMM rounded (straight-through: the weight gradients and data
gradients are products of the rounded operands); h, [Z|R], H~ and q stored as bf16 (the backward's factors z (1 - z), 1 - h~^2, R and
h - h~ read the stored values); the incoming gradient rounded where the pipeline stores it as bf16 -- dhp, dzp|drp, dh = dq R + g Z and
ds, and the head's d1, a GEMM operand twice; x rounded once where the row layout applies (``round_x``: one emulation with, one without).
The emulation is NEVER compared with the device: a composed weight on a rounding boundary flips for all rows at once, so agreement with
it is statistical (tests/test_gpu_bf16.py).  It says how far from float64 this arithmetic lands when nothing is wrong.

Bars.  A class's bar is 4 x the worst ratio of ``emu`` against ``want64`` over every well-conditioned row / tensor of every case, probe
node and both emulations, rounded up to a power of two (4: the summation-order allowance of op_bars.py / cell_probe.py).  Nothing is
taken from the kernels' output.  No bar may exceed CAP: 2 ** -4 (32 u) for everything but the attention classes, 2 ** -2 there -- the
faults this file is after (tests/test_bf16_probe_cpu.py plants them) move a node by tens of percent.  A row or tensor is ill-conditioned
when the references alone say so, gap > CAP / 4 x scale with gap the emulation's own error there (the rule of cell_probe.py); it is
named, not skipped, and held to 4 x its gap.  tests/test_bf16_probe_cpu.py recomputes the table:

    class             worst emu ratio                                   x 4, rounded up        worst HIP ratio (MI355X)
    hidden            6.95e-03  R-F64-T1, x rounded once                     2 ** -5  (3.13e-02)    6.95e-03  R-F64-T1, default forms
    pred              1.00e-02  R-F64-T12                                    2 ** -4  (6.25e-02)    1.00e-02  R-F64-T12, xbf 0
    grad              1.11e-02  R-F64-T5 node 0 linear_z.weight              2 ** -4  (6.25e-02)    1.11e-02  R-F64-T5 node 0 linear_z.weight, xbf 0
    attention         6.25e-02  R-F64-T12 node 40 (the ill-conditioned edge) 2 ** -2  (2.50e-01)    6.60e-02  R-F64-T5 node 26, default forms
    grad_dense        6.11e-03  T-F64-T1 conv_r.lin.weight                   2 ** -5  (3.13e-02)    6.09e-03  T-F64-T1 conv_r.lin.weight
    attention_dense   5.55e-02  R-F64-T5, x rounded once                     2 ** -2  (2.50e-01)    5.90e-02  R-F64-T5, default forms

(Where the device's worst row is the emulation's, to three digits, both took the same roundings there and differ by fp32 summation order
alone.  The attention classes are wide because the references say so: PRE_SHIFT makes half the channels of h nearly the same in every
period, which sharpens the cancellation of the softmax backward; its bar still sits below a dropped or misplaced period, which moves
the attention gradient of a three- or five-period probe by more than its whole scale.  profiles/bf16_bars.txt, written by
tools/bf16_bars.py from one GPU run, holds every case, form, probe node and ratio: 36 runs, all bit-identical on repetition, no row or
tensor over its bar, so no kernel changed.)

``expected_forms`` restates the host predicates of csrc/api_step.hip (bf16_intermediates, frag_shape_ok, weights_frag, xbf_ok,
fused_rows_form, step_form, data_gradients) for the default environment; runs are labelled with its result, the kernel that ran is not
read back.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

import cell_probe as CP
import fused_math as FM
import op_bars as B
from oracle import model as M

U = 2.0 ** -9
C = 256
ORDER_FACTOR = 4.0
CLASSES = ("hidden", "pred", "grad", "attention", "grad_dense", "attention_dense")
BAR = {"hidden": 2.0 ** -5, "pred": 2.0 ** -4, "grad": 2.0 ** -4, "attention": 2.0 ** -2, "grad_dense": 2.0 ** -5, "attention_dense": 2.0 ** -2}
CAP = {k: (2.0 ** -2 if k.startswith("attention") else 2.0 ** -4) for k in CLASSES}
assert all(BAR[k] <= CAP[k] for k in CLASSES)
PRE_SHIFT = 4.0          # tgnn.linear.bias of even channels + 4, of odd channels - 4: x in [0, 1) keeps the embedding's pre-activation within
#                          +-2.9 of its bias, so every element stays more than 1 away from 0 on its own side and act'(h) = 1 or 0.01
#                          by channel, in float64 as in bf16 (a flipped element would move its ds by 99 %: with T rows behind a probe's
#                          gradient that alone puts the embedding's tensors 10 .. 50 % off; tests/test_bf16_probe_cpu.py holds the margin)
GP_SCALE = 0.125         # |d1 A1| stays near u x |gh|: an element of hidden that bf16 takes to the other side of the head's relu moves
#                          that one element of dOH by about one rounding, not by the whole head term

# name -> (model, N, E, region sizes, F, T, O); the last two nodes of every case receive no edge
CASES: Dict[str, Tuple[str, int, int, Tuple[int, ...], int, int, int]] = {
    "R-F64-T12": ("RegionalTemporalGCN", 171, 900, (40, 90, 41), 64, 12, 1),    # M = 2052 = 16 x 128 + 4; node 10 straddles row 128
    "R-F32-T12": ("RegionalTemporalGCN", 43, 200, (11, 32), 32, 12, 3),         # M = 516; F = 32 rows; O = 3
    "R-F64-T5": ("RegionalTemporalGCN", 103, 500, (26, 30, 47), 64, 5, 1),      # odd T; M = 515; node 25 straddles row 128
    "R-F32-T7": ("RegionalTemporalGCN", 37, 160, (19, 18), 32, 7, 1),           # (T F) % 64 = 32: the row layout is refused; node 18 straddles
    "R-F64-T1": ("RegionalTemporalGCN", 643, 3000, (129, 300, 214), 64, 1, 1),  # one period: rows are nodes; M = 5 x 128 + 3
    "R-F64-T48": ("RegionalTemporalGCN", 7, 14, (3, 4), 64, 48, 1),             # node 1 spans the 64-row halves, node 2 straddles row 128
    "R-F32-T48": ("RegionalTemporalGCN", 7, 14, (2, 5), 32, 48, 3),
    "T-F32-T12": ("TemporalGCN", 43, 200, (), 32, 12, 1),                       # regional = 0: cell_bwd8 + dgrad1 + dgrad2 on bf16 stores
    "T-F64-T5": ("TemporalGCN", 103, 500, (), 64, 5, 3),                        # odd T: the last period is one half-wave of cell_bwd8
    "T-F64-T1": ("TemporalGCN", 131, 600, (), 64, 1, 1),
    "T-F32-T48": ("TemporalGCN", 7, 14, (), 32, 48, 1),
    "T-F64-T3": ("TemporalGCN", 45, 200, (), 64, 3, 1),                         # three rows per node: one dropped period is a third of a probe
}
OPTION_SETS: Dict[str, Dict[str, int]] = {
    "default": {},
    "fused_bwd0": {"fused_bwd": 0},                      # bf16 rows with the three data-gradient launches
    "fused_rows0": {"fused_rows": 0},                    # the 64-row fused forward everywhere
    "xbf0": {"xbf": 0, "fused_bwd": 0},                  # no bf16 rows: three launches forward and backward
    "no_rows_flag": {"no_rows_flag": 1},                 # REGT_DIMS_NO_BF16_ROWS on the call: three-launch forward, fused backward
}
DEFAULTS = {"xbf": 1, "fused_bwd": 1, "fused_rows": 1, "no_rows_flag": 0}
LIB_OPTIONS = ("xbf", "fused_bwd", "fused_rows")


def _gen(name: str, what: int) -> torch.Generator:
    return torch.Generator().manual_seed(7000 + 100 * list(CASES).index(name) + what)


def regional(name: str) -> bool:
    return CASES[name][0] == "RegionalTemporalGCN"


def region_bounds(name: str) -> List[int]:
    out = [0]
    for s in CASES[name][3]:
        out.append(out[-1] + s)
    return out


def graph(name: str):
    """(edge_index, edge_weight, [region edge_index], [region edge_weight]) -- random, seeded, no self-loop, no edge into the last two
    nodes; a region's edges are those inside its contiguous block of nodes, and the first node of every block receives one."""
    model, n, e, sizes, _f, _t, _o = CASES[name]
    g = _gen(name, 1)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n - 2, (e,), generator=g)
    bounds = region_bounds(name) if sizes else [0, n]
    assert bounds[-1] == n and all(b + 1 < n - 2 for b in bounds[:-1])
    src = torch.cat([src, torch.tensor([b + 1 for b in bounds[:-1]])])
    dst = torch.cat([dst, torch.tensor(bounds[:-1])])
    keep = src != dst
    src, dst = src[keep], dst[keep]
    ew = 0.5 + torch.rand(src.numel(), generator=g)
    ei = torch.stack([src, dst])
    if not sizes:
        return ei, ew, [ei], [ew]
    blk = torch.bucketize(torch.arange(n), torch.tensor(bounds[1:-1]), right=True)
    ri, rw = [], []
    for r in range(len(sizes)):
        m = (blk[src] == r) & (blk[dst] == r)
        ri.append(ei[:, m].contiguous())
        rw.append(ew[m].contiguous())
    return ei, None, ri, rw


def node_region(name: str) -> torch.Tensor:
    n = CASES[name][1]
    return torch.bucketize(torch.arange(n), torch.tensor(region_bounds(name)[1:-1]), right=True) if regional(name) else torch.zeros(n, dtype=torch.long)


def params(name: str) -> Dict[str, torch.Tensor]:
    model, n, _e, sizes, f, t, o = CASES[name]
    p = M.init_params(model, f, t, o, num_nodes=n, num_regions=max(1, len(sizes)), seed=31 + list(CASES).index(name), hidden=C)
    p["linear1.bias"] = p["linear1.bias"] + 1.0          # the head's inner relu is open everywhere (cell_probe.py)
    p["linear2.bias"] = p["linear2.bias"] + 1.0          # pred stays away from 0
    if model == "RegionalTemporalGCN":                   # the embedding's leaky relu: no element of its mask depends on a rounding either
        sign = torch.ones(C)
        sign[1::2] = -1.0
        p["tgnn.linear.bias"] = p["tgnn.linear.bias"] + PRE_SHIFT * sign
    p["linear1.weight"] = p["linear1.weight"] / PRE_SHIFT              # (a power of two: hidden reaches 4 here; the head's inner relu stays open)
    return p


def inputs(name: str):
    """(x (N, F, T), GH (N, C), GP (N, O)): the snapshot and the dense upstream gradient, whose rows are the probes' upstream gradients."""
    _model, n, _e, _sizes, f, t, o = CASES[name]
    g = _gen(name, 2)
    return torch.rand(n, f, t, generator=g), torch.randn(n, C, generator=g), GP_SCALE * torch.randn(n, o, generator=g)


def probe_nodes(name: str) -> Dict[str, int]:
    """label -> node, in a fixed order; one node may carry several labels (the first wins)."""
    _model, n, _e, sizes, _f, t, _o = CASES[name]
    m = n * t
    want = [("node0", 0), ("last", n - 1), ("row128", min(n - 1, 128 // t)),
            ("last-tile", min(n - 1, ((m - 1) // 128 * 128) // t + 1)), ("no-in-edge", n - 2)]
    if sizes:
        want.insert(4, ("region1", region_bounds(name)[1]))
    out: Dict[str, int] = {}
    for label, node in want:
        if node not in out.values():
            out[label] = node
    return out


def upstream(name: str, label: str):
    """(gh, gp) of one probe (``dense``: the whole GH, GP).  The probe on the node without in-edge has gp = 0."""
    _x, gh_all, gp_all = inputs(name)
    if label == "dense":                                     # (|GP|: the shifted channels of hidden are nearly the same in every node, and a
        return gh_all, gp_all.abs()                          #  sum of them under mixed signs is a cancellation that has nothing to do with a kernel)
    node = probe_nodes(name)[label]
    gh, gp = torch.zeros_like(gh_all), torch.zeros_like(gp_all)
    gh[node] = gh_all[node]
    if label != "no-in-edge":
        gp[node] = gp_all[node]
    return gh, gp


def probe_labels(name: str) -> List[str]:
    return list(probe_nodes(name)) + ["dense"]


# ---- the emulation: bf16 rounding forward and backward -----------------------------------------------------------------------------

class _Rnd(torch.autograd.Function):
    """bf16 rounding of a GEMM operand or of a stored activation; the gradient passes as it is."""
    @staticmethod
    def forward(ctx, v):
        return FM.bf16_round(v)

    @staticmethod
    def backward(ctx, g):
        return g


class _GradStore(torch.autograd.Function):
    """Identity; the incoming gradient is stored as bf16."""
    @staticmethod
    def forward(ctx, v):
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        return FM.bf16_round(g)


class _Sigmoid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v):
        y = torch.sigmoid(v)
        ctx.save_for_backward(FM.bf16_round(y))
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return g * (y * (1.0 - y))


class _Tanh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v):
        y = torch.tanh(v)
        ctx.save_for_backward(FM.bf16_round(y))
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return g * (1.0 - y * y)


class _Mul(torch.autograd.Function):
    """q = h * R in registers; the backward reads the stored R."""
    @staticmethod
    def forward(ctx, h, r):
        ctx.save_for_backward(h, FM.bf16_round(r))
        return h * r

    @staticmethod
    def backward(ctx, g):
        h, r = ctx.saved_tensors
        return g * r, g * h


class _Blend(torch.autograd.Function):
    """z h + (1 - z) h~ on the stored z and h and the h~ of the registers; the backward reads the stored h~."""
    @staticmethod
    def forward(ctx, z, h, ht):
        ctx.save_for_backward(z, h, FM.bf16_round(ht))
        return z * h + (1.0 - z) * ht

    @staticmethod
    def backward(ctx, g):
        z, h, ht = ctx.saved_tensors
        return g * (h - ht), g * z, g * (1.0 - z)


EMU_OPS = {"sigmoid": _Sigmoid.apply, "tanh": _Tanh.apply, "mul": _Mul.apply, "blend": _Blend.apply}
GRAD_STORES = ("pre", "h", "pz", "pr", "ph", "y1")          # ds, dh, dzp, drp, dhp, d1


class _RowsBackward(torch.autograd.Function):
    """Identity; the gradient of the given rows is dropped on the way back."""
    @staticmethod
    def forward(ctx, v, rows):
        ctx.rows = rows
        return v.view_as(v)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().clone()
        g.view(-1, g.shape[-1])[ctx.rows] = 0.0
        return g, None


CORRUPTIONS = ("k-slab", "swap-rows", "zero-last-row", "neighbour-period", "half-wave-period")


def corruption_site(name: str, cor: str) -> Tuple[str, int]:
    """(probe label, node) at which the planted error of ``cor`` shows in case ``name``."""
    _model, n, _e, _sizes, _f, t, _o = CASES[name]
    nodes = probe_nodes(name)
    label = {"k-slab": "row128", "swap-rows": "row128", "zero-last-row": "last", "neighbour-period": "row128", "half-wave-period": "row128"}[cor]
    if label not in nodes:                                   # (the label went to an earlier probe of the same node)
        label = next(k for k, v in nodes.items() if v == {"row128": min(n - 1, 128 // t), "last": n - 1}[label])
    return label, nodes[label]


def _corrupt_tap(name: str, cor: str):
    """The planted faults, each through forward_fused's tap (rows are m = node T + t):
    k-slab            the gate GEMMs' A operand loses k 16..31 in the 64-row tile that holds the probe node's first row
    swap-rows         the hidden input of the probe node's first row and of the row before it change places
    zero-last-row     the blended row M - 1 (the last row of the partial tile) is 0
    neighbour-period  period 0 of the probe node's blended rows is its neighbour's
    half-wave-period  the backward loses dhp and dzp of the probe node's last period (the half wave that is idle at odd T)"""
    _model, n, _e, _sizes, _f, t, _o = CASES[name]
    _label, node = corruption_site(name, cor)
    m0 = node * t

    def tap(key, v):
        if key in GRAD_STORES:
            v = _GradStore.apply(v)
        flat = v.reshape(-1, v.shape[-1]) if v.dim() == 3 else None
        if cor == "k-slab" and key == "h_operand":
            mask = torch.ones_like(flat)
            mask[m0 // 64 * 64:m0 // 64 * 64 + 64, 16:32] = 0.0
            return (flat * mask).view_as(v)
        if cor == "swap-rows" and key == "h":
            idx = torch.arange(flat.shape[0])
            idx[m0], idx[m0 - 1] = m0 - 1, m0
            return flat[idx].view_as(v)
        if cor == "zero-last-row" and key == "hn":
            mask = torch.ones_like(flat)
            mask[-1] = 0.0
            return (flat * mask).view_as(v)
        if cor == "neighbour-period" and key == "hn":
            idx = torch.arange(flat.shape[0])
            idx[m0] = m0 + t
            return flat[idx].view_as(v)
        if cor == "half-wave-period" and key in ("ph", "pz"):
            assert t % 2 == 1, "the idle half wave needs an odd T"
            return _RowsBackward.apply(v, m0 + t - 1)
        return v
    return tap


def _emu_tap(key, v):
    return _GradStore.apply(v) if key in GRAD_STORES else v


def corruption_excess(name: str, cor: str, round_x: bool = False) -> Tuple[float, str]:
    """(worst ratio / bar, where) of the emulation with ``cor`` planted, at the affected probe node alone: its rows of hidden and pred and
    the gradients of its probe."""
    ref = reference(name)
    out = emulate(name, round_x, corrupt=cor)
    label, node = corruption_site(name, cor)
    best = (0.0, "")
    for tensor in ("hidden", "pred"):
        err, scale = CP.row_stats(out[tensor], ref["want"][tensor])
        r = float(CP.row_ratio(err, scale)[node]) / BAR[tensor]
        best = max(best, (r, f"{tensor} node {node}"))
    for k, cls, r, ill in held_grads(out["grads"][label], ref, int(round_x), label)[3]:
        if not ill:
            best = max(best, (r / BAR[cls], f"{label} {k}"))
    return best


def rows_apply(name: str) -> bool:
    """Whether any option set puts the case on bf16 rows (then there is an emulation with x rounded once)."""
    return bool(expected_forms(name)["rows"])


# ---- the references of one case ------------------------------------------------------------------------------------------------------------

_REFS: Dict = {}


def _grads(pred, hidden, tensors: Dict[str, torch.Tensor], name: str) -> Dict[str, Dict[str, Optional[torch.Tensor]]]:
    out = {}
    labels = probe_labels(name)
    for i, label in enumerate(labels):
        gh, gp = upstream(name, label)
        loss = (hidden * gh.to(hidden.dtype)).sum() + (pred * gp.to(pred.dtype)).sum()
        gs = torch.autograd.grad(loss, list(tensors.values()), retain_graph=i + 1 < len(labels), allow_unused=True)
        out[label] = {k: (None if g is None else g.detach()) for k, g in zip(tensors, gs)}
    return out


def want64(name: str) -> Dict:
    """{"pred", "hidden", "grads": {probe label: {parameter: gradient | None}}} from the oracle in float64."""
    ei, ew, ri, rw = graph(name)
    x, _gh, _gp = inputs(name)
    p = {k: v.double().requires_grad_(True) for k, v in params(name).items()}
    if regional(name):
        pred, hidden = M.regional_temporal_gcn(p, x.double(), ei, ri, [w.double() for w in rw])
    else:
        pred, hidden = M.temporal_gcn(p, x.double(), ei, ew.double())
    return {"pred": pred.detach(), "hidden": hidden.detach(), "grads": _grads(pred, hidden, p, name)}


def emulate(name: str, round_x: bool, corrupt: Optional[str] = None) -> Dict:
    """The same in fp32 with the bf16 roundings of the pipeline (``corrupt``: one of CORRUPTIONS, a planted error)."""
    assert corrupt is None or corrupt in CORRUPTIONS, corrupt
    ei, ew, ri, rw = graph(name)
    x, _gh, _gp = inputs(name)
    n = CASES[name][1]
    p = {k: v.clone().requires_grad_(True) for k, v in params(name).items()}
    a, ls = FM.dense_ops(ei, ew, ri, rw, n, torch.float32)
    pred, hidden = FM.forward_fused(p, x, a, ls, regional=regional(name), rnd=_Rnd.apply, store=_Rnd.apply, round_x=round_x,
                                    tap=_emu_tap if corrupt is None else _corrupt_tap(name, corrupt), ops=EMU_OPS)
    return {"pred": pred.detach(), "hidden": hidden.detach(), "grads": _grads(pred, hidden, p, name)}


def reference(name: str) -> Dict:
    """{"want": want64, "emu": {0: ..., 1: ... where the row layout can apply}}, computed once and shared."""
    if name not in _REFS:
        _REFS[name] = {"want": want64(name), "emu": {int(rx): emulate(name, rx) for rx in ((False, True) if rows_apply(name) else (False,))}}
    return _REFS[name]


# ---- the statistics ------------------------------------------------------------------------------------------------------------------------

def klass(tensor: str, label: str = "") -> str:
    if tensor in ("hidden", "pred"):
        return tensor
    base = "attention" if tensor.endswith("_attention") else "grad"
    return base + ("_dense" if label == "dense" else "")


def tensor_stats(got: torch.Tensor, want: torch.Tensor) -> Tuple[float, float]:
    """(max |got - want64|, max |want64|); a NaN in ``got`` gives err inf."""
    err = (got.detach().cpu().double() - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    return float(err.max()), float(want.abs().max())


def _ratio(err: float, scale: float) -> float:
    return (0.0 if err == 0.0 else float("inf")) if scale == 0.0 else err / scale


def held_rows(got: torch.Tensor, ref: Dict, rx: int, tensor: str, what: str = ""):
    """``hidden`` / ``pred`` per node row.  (worst ratio over the well-conditioned rows, named rows, failures [(label, row, err, limit)])."""
    want, emu = ref["want"][tensor], ref["emu"][rx][tensor]
    err, scale = CP.row_stats(got.detach().cpu(), want)
    gap, _ = CP.row_stats(emu, want)
    ill = gap > CAP[tensor] / 4 * scale
    limit = torch.where(ill, ORDER_FACTOR * gap, BAR[tensor] * scale)
    named = [f"{what} {tensor} node {int(i)}: ill-conditioned (gap {float(gap[i]):.2e}, scale {float(scale[i]):.2e})" for i in torch.nonzero(ill).flatten()]
    ratio = CP.row_ratio(err, scale)
    worst = float(ratio[~ill].max()) if bool((~ill).any()) else 0.0
    bad = [(f"{what} {tensor}", int(i), float(err[i]), float(limit[i])) for i in torch.nonzero(~(err <= limit)).flatten()]
    return worst, named, bad


def held_grads(got: Dict[str, Optional[torch.Tensor]], ref: Dict, rx: int, label: str, what: str = ""):
    """The parameter gradients of one probe.  ({class: (worst ratio, tensor)}, named tensors, failures, [(tensor, class, ratio, ill)])."""
    want, emu = ref["want"]["grads"][label], ref["emu"][rx]["grads"][label]
    worst: Dict[str, Tuple[float, str]] = {}
    named, bad, rows = [], [], []
    for k, w in want.items():
        g = got.get(k)
        if w is None:
            if g is not None and float(g.abs().max()) != 0.0:
                bad.append((f"{what} {label} {k}: a gradient where the oracle has none", -1, float(g.abs().max()), 0.0))
            continue
        if g is None:
            bad.append((f"{what} {label} {k}: no gradient", -1, float("inf"), 0.0))
            continue
        cls = klass(k, label)
        err, scale = tensor_stats(g, w)
        gap, _ = tensor_stats(emu[k], w)
        ill = scale > 0.0 and gap > CAP[cls] / 4 * scale
        limit = ORDER_FACTOR * gap if ill else BAR[cls] * scale
        r = _ratio(err, scale)
        rows.append((k, cls, r, ill))
        if ill:
            named.append(f"{what} {label} {k}: ill-conditioned (gap {gap:.2e}, scale {scale:.2e})")
        elif r > worst.get(cls, (-1.0, ""))[0]:
            worst[cls] = (r, k)
        if not err <= limit:
            bad.append((f"{what} {label} {k} [{cls}]", -1, err, limit))
    return worst, named, bad, rows


def bar_table(cases=None) -> Dict[str, Tuple[float, str]]:
    """class -> (worst ratio of the emulations over the well-conditioned rows and tensors, where)."""
    out = {k: (0.0, "") for k in CLASSES}

    def take(cls, r, where):
        if r > out[cls][0]:
            out[cls] = (r, where)

    for name in (cases or CASES):
        ref = reference(name)
        for rx, emu in ref["emu"].items():
            for tensor in ("hidden", "pred"):
                take(tensor, held_rows(emu[tensor], ref, rx, tensor)[0], f"{name} round_x {rx}")
            for label in probe_labels(name):
                for cls, (r, k) in held_grads(emu["grads"][label], ref, rx, label)[0].items():
                    take(cls, r, f"{name} round_x {rx} {label} {k}")
    return out


def ill_share(name: str) -> Dict[str, Tuple[int, int, List[str]]]:
    """"rows" / "tensors" / "dense" -> (ill-conditioned, all, labels) by the references alone, over both emulations."""
    ref = reference(name)
    out = {"rows": [0, 0, []], "tensors": [0, 0, []], "dense": [0, 0, []]}
    for rx, emu in ref["emu"].items():
        for tensor in ("hidden", "pred"):
            named = held_rows(emu[tensor], ref, rx, tensor, f"{name} round_x {rx}")[1]
            out["rows"][0] += len(named)
            out["rows"][1] += int(ref["want"][tensor].shape[0])
            out["rows"][2] += named
        for label in probe_labels(name):
            _w, named, _b, rows = held_grads(emu["grads"][label], ref, rx, label, f"{name} round_x {rx}")
            key = "dense" if label == "dense" else "tensors"
            if key == "dense":                                # (the attention gradient is a class of its own there)
                named = [s for s in named if "_attention" not in s]
                rows = [r for r in rows if not r[0].endswith("_attention")]
            out[key][0] += len(named)
            out[key][1] += len(rows)
            out[key][2] += named
    return {k: (v[0], v[1], v[2]) for k, v in out.items()}


# ---- the dispatch, restated ----------------------------------------------------------------------------------------------------------------

def expected_forms(name_or_case, options: Optional[Dict[str, int]] = None) -> Dict[str, object]:
    """case (model, N, E, region sizes, F, T, O) or its name -> {"rows": x / A_hat x / L~ x are bf16 rows (xbf), "forward": the kernel(s) of
    the cell's forward, "weights": fragment-order bf16 copies or the fp32 ones, "backward": the data-gradient form, "node_sum_rows"}.
    Arithmetic 2, the default environment; options: xbf (1), fused_bwd (1), fused_rows (1), no_rows_flag (0: REGT_DIMS_NO_BF16_ROWS).
    Every case here has node-disjoint regions with ids sorted by node and a merged operator."""
    case = CASES[name_or_case] if isinstance(name_or_case, str) else name_or_case
    o = dict(DEFAULTS)
    o.update(options or {})
    model, n, _e, sizes, f, t, _o = case
    reg, r = model == "RegionalTemporalGCN", max(1, len(sizes))
    ibf = C % B.GBN == 0 and f % 4 == 0                                       # bf16_intermediates (gemm_mode() == 2)
    frag_shape = ibf and f % 32 == 0 and C % 128 == 0                         # frag_shape_ok
    weights_frag = frag_shape and (min(r, 128 // t + 2) + 1) * (f // 32) <= 64 and (2 * C + f) // 32 <= 64
    fused_fwd_ok = C == 256 and f in (32, 64)                                 # fused_forward_ok
    xbf = bool(o["xbf"]) and not o["no_rows_flag"] and frag_shape and reg and r > 1 and fused_fwd_ok and (t * f) % 64 == 0 and \
        n * t * f * 2 < (1 << 32) - 4096                                      # xbf_ok (own rows, packed here)
    rows_form = bool(o["fused_rows"]) and fused_fwd_ok and t <= 16 and reg    # fused_rows_form
    wfr = ibf and weights_frag and reg                                        # step_form: abf = ibf (the hidden input is the model's own)
    fused_bwd = wfr and C == 256 and bool(o["fused_bwd"])                     # data_gradients
    if xbf:
        fwd = "fused_rows_kernel" if rows_form else "fused_fwd_kernel"
    else:
        fwd = "embedding + gates + candidate" + (", bf16 stores" if ibf else "")
    return {"rows": int(xbf), "forward": fwd, "weights": "fragment-order bf16" if wfr else "fp32 [N][K]",
            "backward": "fused_bwd_kernel" if fused_bwd else "cell_bwd8 + dgrad1 + dgrad2 (bf16 stores)",
            "node_sum_rows": 16 if (ibf and rows_form) else 64}


def form_label(forms: Dict[str, object]) -> str:
    return " | ".join(f"{k} {forms[k]}" for k in ("rows", "forward", "weights", "backward", "node_sum_rows"))


def runs(name: str) -> List[str]:
    """The option sets of one case: every set whose forms differ from those of the sets before it (TemporalGCN: the default alone)."""
    out, seen = [], []
    for key, opts in OPTION_SETS.items():
        forms = expected_forms(name, opts)
        if forms not in seen:
            seen.append(forms)
            out.append(key)
    return out


# what "every bf16 form" means: (predicate over (forms, options), label); tests/test_bf16_probe_cpu.py asks for two cases each
FORMS = (
    (lambda fm, o: fm["rows"] and fm["backward"] == "fused_bwd_kernel", "fused forward with fused backward"),
    (lambda fm, o: fm["rows"] and fm["backward"].startswith("cell_bwd8"), "bf16 rows with the three data-gradient launches"),
    (lambda fm, o: not fm["rows"] and o.get("xbf") == 0, "no bf16 rows (xbf 0)"),
    (lambda fm, o: not fm["rows"] and o.get("no_rows_flag") == 1, "no bf16 rows (REGT_DIMS_NO_BF16_ROWS)"),
    (lambda fm, o: fm["forward"] == "fused_rows_kernel", "fused_rows 1"),
    (lambda fm, o: fm["forward"] == "fused_fwd_kernel" and o.get("fused_rows") == 0, "fused_rows 0"),
    (lambda fm, o: fm["forward"] == "fused_fwd_kernel" and o.get("fused_rows", 1) == 1, "the 64-row fused forward at T > 16"),
    (lambda fm, o: fm["weights"].startswith("fp32"), "regional = 0"),
)


# ---- the model on the device (tests/test_gpu_bf16_bars.py, tools/bf16_bars.py) -------------------------------------------------------------

_DEVICE: Dict = {}


def device_case(R, name: str):
    """(module, prepared graph, x) of one case on the device, shared by every option set."""
    if name not in _DEVICE:
        model, n, _e, sizes, f, t, o = CASES[name]
        ei, ew, ri, rw = graph(name)
        if regional(name):
            mod = R.RegionalTemporalGCN(node_features=f, num_nodes=n, periods=t, output_dim=o, num_regions=len(sizes), hidden_channels=C)
        else:
            mod = R.TemporalGCN(node_features=f, periods=t, output_dim=o, hidden_channels=C)
        mod.load_state_dict(params(name), strict=True)
        mod = mod.cuda()
        if regional(name):
            g = mod.prepare_graph(ei.cuda(), [i.cuda() for i in ri], [w.cuda() for w in rw])
        else:
            g = mod.prepare_graph(ei.cuda(), ew.cuda(), n)
        _DEVICE[name] = (mod, g, inputs(name)[0].cuda())
    return _DEVICE[name]


def run_hip(R, name: str, flags: int) -> Dict:
    """One forward + backward per probe: {"pred", "hidden", "grads": {label: {parameter: gradient}}, "identical": every forward gave the
    same bits and the repeated dense backward the same gradients}."""
    mod, g, x = device_case(R, name)
    mod.call_flags = flags
    out: Dict = {"grads": {}, "identical": True}
    try:
        for label in probe_labels(name) + ["dense"]:
            gh, gp = upstream(name, label)
            mod.zero_grad(set_to_none=True)
            pred, hidden = mod.forward_prepared(x, g)
            ((hidden * gh.cuda()).sum() + (pred * gp.cuda()).sum()).backward()
            torch.cuda.synchronize()
            grads = {k: (None if q.grad is None else q.grad.detach().cpu().clone()) for k, q in mod.named_parameters()}
            pred, hidden = pred.detach().cpu(), hidden.detach().cpu()
            if "pred" not in out:
                out["pred"], out["hidden"] = pred, hidden
            else:
                out["identical"] &= torch.equal(pred, out["pred"]) and torch.equal(hidden, out["hidden"])
            if label in out["grads"]:                        # the second dense run
                out["identical"] &= all((a is None and grads[k] is None) or torch.equal(a, grads[k]) for k, a in out["grads"][label].items())
            else:
                out["grads"][label] = grads
    finally:
        mod.call_flags = 0
        mod.zero_grad(set_to_none=True)
    return out


def measure(R, name: str, key: str) -> Dict:
    """One case under one option set on the device (arithmetic and switches set here and put back): every row and every probe held.
    {"forms", "ratios": [(what, class, ratio, ill)], "worst": {class: (ratio, what)}, "named", "bad", "identical"}."""
    lib = R.load_library()
    opts = dict(DEFAULTS)
    opts.update(OPTION_SETS[key])
    ref = reference(name)
    prev_mode = lib.regt_set_gemm_mode(2)
    prev = {k: lib.regt_set_option(k.encode(), opts[k]) for k in LIB_OPTIONS}
    try:
        got = run_hip(R, name, R._lib.DIMS_NO_BF16_ROWS if opts["no_rows_flag"] else 0)
    finally:
        for k in LIB_OPTIONS:
            lib.regt_set_option(k.encode(), prev[k])
        lib.regt_set_gemm_mode(prev_mode)
    forms = expected_forms(name, OPTION_SETS[key])
    rx = int(forms["rows"])
    what = f"{name} {key}"
    out = {"forms": forms, "ratios": [], "worst": {}, "named": [], "bad": [], "identical": got["identical"]}

    def take(cls, r, where):
        if r > out["worst"].get(cls, (-1.0, ""))[0]:
            out["worst"][cls] = (r, where)

    for tensor in ("hidden", "pred"):
        worst, named, bad = held_rows(got[tensor], ref, rx, tensor, what)
        out["ratios"].append((tensor, tensor, worst, False))
        take(tensor, worst, what)
        out["named"] += named
        out["bad"] += bad
    for label in probe_labels(name):
        worst, named, bad, rows = held_grads(got["grads"][label], ref, rx, label, what)
        out["ratios"] += [(f"{label} (node {probe_nodes(name).get(label, '*')}) {k}", cls, r, ill) for k, cls, r, ill in rows]
        for cls, (r, k) in worst.items():
            take(cls, r, f"{what} {label} {k}")
        out["named"] += named
        out["bad"] += bad
    return out
