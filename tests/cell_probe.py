"""Per-row bars for the GRU cell behind regt_cell_forward / regt_cell_backward (functional.CellFunction): ``hidden``, ``pred`` and the
gradient of the hidden input ``dh_in``.

Test helper only (like embed_probe.py).  ``dh_in`` (M x C, M = N T rows ordered node * T + t) is what cell_bwd, dgrad_candidate and
dgrad_gates leave with no reduction over rows in between: row m depends on that row's inputs and on its node's upstream gradient
alone, so a wrong tail row, a wrong tile edge or a lost K slab of one column tile shows in that row and nowhere else.  The statistic is
per row -- rows of ``hidden`` and ``pred`` are nodes, rows of ``dh_in`` are (node, period) pairs:

    err_m = max_c |got[m, c] - want64[m, c]|        scale_m = max_c |want64[m, c]|        ratio_m = err_m / scale_m

A row whose float64 values are all 0 must be exactly 0; a NaN fails.

References.  ``cell`` states the cell as regt_cell_forward runs it (regional = 0, R = 1: no activation on the hidden input):

    z = sigmoid(h Uz^T + ax Gz^T + cz)      r = sigmoid(h Ur^T + ax Gr^T + cr)      h~ = tanh((h * r) Uh^T + ax Gh^T + ch)
    hn = z * h + (1 - z) * h~               hidden = sum_t softmax(att)_t hn_t      pred = head(hidden)  (fused_math.forward_fused)

with the composed weights of fused_math.compose(..., regional=False) and ax = A_hat x formed in float64 from the operator's own CSR
(op_bars.csr_reference: the aggregation is not under test here).  In float64 under autograd it gives ``want64``.  ``cell32`` is the same in
fp32 with a hand-written backward (the factors z (1 - z), 1 - h~^2 as csrc/kernels.h cb_* states them) and ONE difference that matters:
the kernels do not call expf / tanhf, csrc/gemm_epilogue.h has fast_sigmoid(x) = rcp(1 + exp2(x * -log2e)) and fast_tanh(x) =
1 - 2 rcp(1 + exp2(2 x * log2e)); cell32 runs exactly those sequences in fp32 torch ops, so the bars below include the cancellation of
fast_tanh near 0 and exclude nothing else.

Probes (``params``): parameter sets from oracle.model.init_params with blocks zeroed so that one kernel's contribution stands alone in
dh_in.  ``full`` as seeded; ``blend`` Uz = Ur = Uh = 0 (dh_in = dhn * z, one product per element); ``candidate`` Uz = Ur = 0
(dh_in = dhn * z + ((dhn (1 - z) (1 - h~^2)) Uh) * r); ``gates`` Uh = 0 (drp = 0, dh_in = dhn * z + dzp Uz); ``saturated`` = full with
h_in x SAT_H and the gate biases x SAT_B: pre-activations beyond +-60 in both signs, where exp2 overflows to inf or underflows to 0
inside the fast forms -- every output must be finite and z (1 - z) may be exactly 0.  Two biases are shifted by +1 in every probe,
``linear2.bias`` (pred stays away from 0: with O = 1 a row of pred is one number) and ``linear1.bias`` (the head's inner relu is
open everywhere: no element of its mask depends on a rounding).  The upstream gradient is both dhidden and dpred, random and seeded:
loss = (hidden * gh).sum() + (pred * gp).sum().  h_in ~ 0.5 randn, x in [0, 1), seeded per case.

The head's outer relu reads ``hidden``: an element of hidden within EDGE x its row's scale of 0 in float64 may be taken on either side
by an fp32 sum, and its whole (d1 A1) term then enters or leaves dOH of that node.  The float64 reference alone decides which elements
those are; their nodes' dh_in rows are held to the reference with the masks as float64 has them OR with those elements flipped
(``want64["dh_in_alt"]``), and the rows are named.

Bars.  A class's bar is 4 x the worst ratio_m of cell32 over every well-conditioned row of every case and probe of CASES, rounded up to
a power of two (4: the summation-order allowance of op_bars.py / grad_bars.py -- tile and chunk boundaries move with the CU count).
Nothing is derived from the kernels' output; no bar may exceed grad_bars.CAP["default"] = 1e-4.  ``dh_in_blend`` is the blend probe's
class of its own.  tests/test_cell_probe_cpu.py recomputes the table:

    class         worst cell32 ratio                                   x 4, rounded up         worst HIP ratio (MI355X)
    hidden        2.44e-06  M4104-T12 saturated                        2 ** -16  (1.53e-05)    2.62e-06  M4104-T12 saturated, bf16x3
    pred          2.11e-06  M8196-T12 saturated                        2 ** -16  (1.53e-05)    1.62e-06  M8196-T12 saturated, fp32
    dh_in         7.74e-06  M8196-T12 saturated                        2 ** -14  (6.10e-05)    8.61e-06  M8196-T12 saturated, fp32, both forms
    dh_in_blend   2.70e-07  M8196-T12 blend                            2 ** -19  (1.91e-06)    3.95e-07  M510-T255 blend, fp32

(the non-saturated probes alone: hidden 3.8e-07, pred 2.1e-06, dh_in 3.9e-07; the saturated probe, whose h_in is 128 x larger under
gates that are mostly closed, sets three of the four.)  (profiles/cell_bars.txt, written by tools/cell_bars.py from one GPU run, holds every case, probe, mode and form.  No kernel was over a
bar, so none changed.)

Ill-conditioned rows are named, not skipped: a row is ill-conditioned when the references alone say so, gap_m > CAP / 4 x scale_m with
gap_m the error of cell32 in that row; it is held to 4 x gap_m with no floor and its label is returned.  Host conditions
(tests/test_cell_probe_cpu.py): no such row in any probe but ``saturated``, at most 5 % of the rows there.

``expected_forms`` restates the host predicates of csrc/api_step.hip (StepForm, data_gradients), csrc/gemm_dispatch.hip, gemm_flat.h
launch_fast and gemm_cell.hip launch_cand_vec for the cell path in the two fp32-storage arithmetics; cases are labelled with its
result, the kernel that ran is not read back.  cell_bwd8_kernel reads bf16-stored activations, which a caller-supplied fp32 hidden
input never has: the cell path cannot reach it in any arithmetic, so the cell_bwd variant is cell_bwd_kernel or none (dgrad1_gen).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

import fused_math as FM
import grad_bars as GB
import op_bars as B
from oracle import model as M

BAR = {"hidden": 2.0 ** -16, "pred": 2.0 ** -16, "dh_in": 2.0 ** -14, "dh_in_blend": 2.0 ** -19}
CAP = GB.CAP["default"]
assert all(v <= CAP for v in BAR.values())
ORDER_FACTOR = 4.0
EDGE = BAR["hidden"]             # |hidden64| <= EDGE x row scale: a result inside the bar may open or close the head's relu
SAT_H, SAT_B = 128.0, 400.0
PROBES = ("full", "blend", "candidate", "gates", "saturated")
MODES = (0, 1)
CLASSES = ("hidden", "pred", "dh_in", "dh_in_blend")
LOG2E = 1.4426950408889634

# name -> (N, E, F, T, C, O, the last two nodes receive no edge)
CASES: Dict[str, Tuple[int, int, int, int, int, int, bool]] = {
    "M7-T1": (7, 20, 8, 1, 128, 1, False),                 # one partial tile, T = 1
    "M129-T3": (43, 150, 7, 3, 132, 3, False),             # node 42 straddles row 128; F padded 7 -> 8; 4-wide second column tile
    "M132-T12": (11, 40, 32, 12, 256, 1, True),            # node 10 straddles row 128; two column tiles; no edge into nodes 9, 10
    "M144-T48": (3, 6, 8, 48, 128, 3, False),              # node 1 spans the 64-row halves 0 | 1
    "M510-T255": (2, 2, 8, 255, 128, 1, False),            # the longest window the candidate launcher accepts
    "M4104-T12": (342, 1400, 8, 12, 256, 1, False),        # 132 gate tiles (big-tile core, LDS table) over 66 candidate / dgrad tiles (small kernel)
    "M8196-T12": (683, 2800, 32, 12, 256, 1, False),       # 130 tiles at C = 256: the big-tile cores, dgrad1_gen; a 4-row tail tile
}
GEN_OPTIONS = (1, 0)              # regt_set_option("dgrad1_gen", .): the one runtime switch that selects a data-gradient form (fp32 storage)


def _gen(name: str, what: int) -> torch.Generator:
    return torch.Generator().manual_seed(1000 * list(CASES).index(name) + what)


def graph(name: str):
    """(edge_index (2, E), edge_weight (E)) -- random, seeded; with the flag no edge ends in the last two nodes."""
    n, e, _f, _t, _c, _o, tail = CASES[name]
    g = _gen(name, 1)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n - 2 if tail else n, (e,), generator=g)
    return torch.stack([src, dst]), 0.5 + torch.rand(e, generator=g)


def inputs(name: str, probe: str = "full"):
    """(x (N, F, T), h_in (M, C), gh (N, C), gp (N, O))."""
    n, _e, f, t, c, o, _ = CASES[name]
    g = _gen(name, 2)
    x = torch.rand(n, f, t, generator=g)
    h = 0.5 * torch.randn(n * t, c, generator=g)
    gh = torch.randn(n, c, generator=g)
    gp = torch.randn(n, o, generator=g)
    return x, (h * SAT_H if probe == "saturated" else h), gh, gp


def params(name: str, probe: str) -> Dict[str, torch.Tensor]:
    _n, _e, f, t, c, o, _ = CASES[name]
    p = M.init_params("TemporalGCN", f, t, o, seed=11 + list(CASES).index(name), hidden=c)
    q = "tgnn._base_tgcn."
    p["linear1.bias"] = p["linear1.bias"] + 1.0
    p["linear2.bias"] = p["linear2.bias"] + 1.0
    zero = {"full": "", "blend": "zrh", "candidate": "zr", "gates": "h", "saturated": ""}[probe]
    for k in zero:
        w = p[f"{q}linear_{k}.weight"].clone()
        w[:, c:] = 0.0
        p[f"{q}linear_{k}.weight"] = w
    if probe == "saturated":
        for k in "zrh":
            p[f"{q}linear_{k}.bias"] = p[f"{q}linear_{k}.bias"] * SAT_B
        p["linear1.weight"] = p["linear1.weight"] / SAT_H          # (a power of two: the head sees hidden at the other probes' size)
    return p


def csr_of(ei, ew, n: int):
    """A destination-sorted CSR of A_hat from the oracle's gcn_norm in fp32."""
    from oracle import graph_ops as G
    src, dst, w = G.gcn_norm_edges(ei, ew, n, torch.float32)
    order = torch.argsort(dst, stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
    return rowptr.int(), src[order].int(), w[order].contiguous()


def cpu_csr(name: str):
    """The host's stand-in for the prepared operator (the package prepares its own with the library; on the device the references
    are formed from that one)."""
    ei, ew = graph(name)
    return csr_of(ei, ew, CASES[name][0])


def aggregate64(csr, x: torch.Tensor) -> torch.Tensor:
    """ax (M, F) in float64 from the operator's own CSR."""
    n, f, t = x.shape
    rp, col, val = (v.cpu() for v in csr)
    want, _den = B.csr_reference(rp, col, val, x.permute(0, 2, 1).reshape(n, t * f).contiguous())
    return want.reshape(n * t, f)


# ---- the restatement (float64 under autograd) --------------------------------------------------------------------------------------

def cell(p, ax, h_in, att, dtype, flip=None, parts: Optional[Dict] = None):
    """(pred (N, O), hidden (N, C)) from ax (M, F), h_in (M, C) and the attention logits ``att`` (T), every tensor of ``p`` in ``dtype``.
    ``flip`` (N, C) bool: elements of the head's outer relu mask taken on the other side.  ``parts``: receives z, r, ht, hn, pre-activations."""
    t = att.numel()
    w = FM.compose(p, 1, regional=False)
    ax, h = ax.to(dtype), h_in
    pz = h @ w["Uz"].t() + ax @ w["Gz"].t() + w["cz"]
    pr = h @ w["Ur"].t() + ax @ w["Gr"].t() + w["cr"]
    z, r = torch.sigmoid(pz), torch.sigmoid(pr)
    ph = (h * r) @ w["Uh"].t() + ax @ w["Gh"].t() + w["ch"]
    ht = torch.tanh(ph)
    hn = z * h + (1 - z) * ht
    probs = torch.softmax(att, dim=0)
    n = h.shape[0] // t
    hidden = (hn.view(n, t, -1) * probs.view(1, t, 1)).sum(dim=1)
    mask = hidden.detach() > 0
    if flip is not None:
        mask = mask ^ flip
    y1 = torch.relu((hidden * mask.to(dtype)) @ p["linear1.weight"].t() + p["linear1.bias"])
    pred = y1 @ p["linear2.weight"].t() + p["linear2.bias"]
    if parts is not None:
        parts.update(z=z, r=r, ht=ht, hn=hn, pz=pz, pr=pr, ph=ph, y1=y1, probs=probs)
    return pred, hidden


# ---- the fp32 restatement: the kernels' fast forms, hand-written backward ----------------------------------------------------------------

def fast_sigmoid(x: torch.Tensor) -> torch.Tensor:
    return 1.0 / (1.0 + torch.exp2(x * torch.tensor(-LOG2E, dtype=torch.float32)))


def fast_tanh(x: torch.Tensor) -> torch.Tensor:
    return 1.0 - 2.0 * (1.0 / (1.0 + torch.exp2((2.0 * x) * torch.tensor(LOG2E, dtype=torch.float32))))


def exp_sigmoid(x: torch.Tensor) -> torch.Tensor:
    return 1.0 / (1.0 + torch.exp(-x))


def exp_tanh(x: torch.Tensor) -> torch.Tensor:
    return 1.0 - 2.0 * (1.0 / (1.0 + torch.exp(2.0 * x)))


CORRUPTIONS = ("uh-tail", "r-next-row", "one-minus-ht", "drop-blend-last-period", "dzp-uz-twice", "exp")


def cell32(p, ax32, h_in, gh, gp, corrupt: Optional[str] = None):
    """{pred, hidden, dh_in, z, dhn} in fp32.  ``corrupt``: one of CORRUPTIONS, a planted error (tests/test_cell_probe_cpu.py)."""
    assert corrupt is None or corrupt in CORRUPTIONS, corrupt
    att = p["tgnn._attention"]
    t = att.numel()
    w = FM.compose(p, 1, regional=False)
    h = h_in
    m, c = h.shape
    n = m // t
    sig, tanh = (exp_sigmoid, exp_tanh) if corrupt == "exp" else (fast_sigmoid, fast_tanh)
    z = sig(h @ w["Uz"].t() + ax32 @ w["Gz"].t() + w["cz"])
    r = sig(h @ w["Ur"].t() + ax32 @ w["Gr"].t() + w["cr"])
    ht = tanh((h * r) @ w["Uh"].t() + ax32 @ w["Gh"].t() + w["ch"])
    hn = z * h + (1.0 - z) * ht
    probs = torch.softmax(att, dim=0)
    hidden = (hn.view(n, t, c) * probs.view(1, t, 1)).sum(dim=1)
    y1 = torch.relu(torch.relu(hidden) @ p["linear1.weight"].t() + p["linear1.bias"])
    pred = y1 @ p["linear2.weight"].t() + p["linear2.bias"]
    # backward
    d1 = (gp @ p["linear2.weight"]) * (y1 > 0)
    doh = (d1 @ p["linear1.weight"]) * (hidden > 0) + gh
    dhn = (probs.view(1, t, 1) * doh.view(n, 1, c)).expand(n, t, c).reshape(m, c)
    dhp = dhn * (1.0 - z) * ((1.0 - ht) if corrupt == "one-minus-ht" else (1.0 - ht * ht))
    dzp = dhn * (h - ht) * (z * (1.0 - z))
    dq = dhp @ w["Uh"]
    if corrupt == "uh-tail":                    # one row misses the K % 32 tail of the contraction with Uh
        k0 = c - c % 32
        assert k0 < c, "uh-tail needs C % 32 != 0"
        row = min(m - 1, 77)
        dq[row] = dhp[row, :k0] @ w["Uh"][:k0]
    drp = dq * h * (r * (1.0 - r))
    rr = r
    if corrupt == "r-next-row":                 # the last row of the first 128-row tile reads the next row's r
        assert m > 128, "r-next-row needs a second row tile"
        rr = r.clone()
        rr[127] = r[128]
    blend = dhn * z
    if corrupt == "drop-blend-last-period":
        blend = blend.clone()
        blend.view(n, t, c)[:, t - 1] = 0.0
    dh = dq * rr + blend
    gate = dzp @ w["Uz"] + drp @ w["Ur"]
    if corrupt == "dzp-uz-twice":               # the first column tile's dzp Uz enters twice
        gate[:, :128] += (dzp @ w["Uz"])[:, :128]
    return {"pred": pred, "hidden": hidden, "dh_in": dh + gate, "z": z, "dhn": dhn, "drp": drp, "gate": gate, "dq": dq}


# ---- the references of one (case, probe) -------------------------------------------------------------------------------------------------

_REFS: Dict = {}


def reference(name: str, probe: str, csr=None) -> Dict:
    """{"want": {pred, hidden, dh_in, dh_in_alt | None, edge_nodes}, "r32": cell32's outputs, "parts": float64 z, r, ..., "den_blend"}.
    Computed once and shared (``csr``: the operator's CSR; default cpu_csr)."""
    key = (name, probe)
    if key in _REFS:
        return _REFS[key]
    _n, _e, _f, t, c, _o, _ = CASES[name]
    p = params(name, probe)
    x, h_in, gh, gp = inputs(name, probe)
    ax = aggregate64(cpu_csr(name) if csr is None else csr, x)
    p64 = {k: v.double() for k, v in p.items()}
    want: Dict = {}
    parts: Dict = {}

    def run(flip=None, keep=None):
        h = h_in.double().requires_grad_(True)
        pred, hidden = cell(p64, ax, h, p64["tgnn._attention"], torch.float64, flip=flip, parts=keep)
        ((hidden * gh.double()).sum() + (pred * gp.double()).sum()).backward()
        return pred.detach(), hidden.detach(), h.grad

    want["pred"], want["hidden"], want["dh_in"] = run(keep=parts)
    edge = want["hidden"].abs() <= EDGE * want["hidden"].abs().amax(dim=1, keepdim=True)
    want["edge_nodes"] = torch.nonzero(edge.any(dim=1)).flatten()
    want["dh_in_alt"] = run(flip=edge)[2] if bool(edge.any()) else None
    parts = {k: v.detach() for k, v in parts.items()}
    # sum of |terms| of one element of dhn z in the blend probe: p_t (|d1| |A1| + |gh|) z
    if probe == "blend":
        d1 = (gp.double() @ p64["linear2.weight"]) * (parts["y1"] > 0)
        den = (d1.abs() @ p64["linear1.weight"].abs()) * (want["hidden"] > 0) + gh.double().abs()
        n = den.shape[0]
        den = (parts["probs"].view(1, t, 1) * den.view(n, 1, c)).expand(n, t, c).reshape(n * t, c) * parts["z"]
    else:
        den = None
    out = {"want": want, "r32": cell32(p, ax.float(), h_in, gh, gp), "parts": parts, "den_blend": den}
    _REFS[key] = out
    return out


# ---- the statistic -----------------------------------------------------------------------------------------------------------------------

def row_stats(got: torch.Tensor, want: torch.Tensor):
    """(err_m, scale_m) in float64; a NaN in ``got`` gives err inf."""
    err = (got.double() - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    return err.amax(dim=1), want.abs().amax(dim=1)


def row_ratio(err: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """err / scale per row; a row of scale 0 demands err 0 (inf otherwise)."""
    zero = scale == 0
    r = err / torch.where(zero, torch.ones_like(scale), scale)
    return torch.where(zero & (err != 0), torch.full_like(r, float("inf")), r)


def klass(tensor: str, probe: str) -> str:
    return "dh_in_blend" if (tensor == "dh_in" and probe == "blend") else tensor


def edge_rows(ref: Dict) -> torch.Tensor:
    """Rows of dh_in whose node has an element of hidden on the head's relu edge."""
    t = ref["want"]["dh_in"].shape[0] // ref["want"]["hidden"].shape[0]
    return (ref["want"]["edge_nodes"][:, None] * t + torch.arange(t)).flatten()


def ref_rows(got: torch.Tensor, ref: Dict, tensor: str):
    """(err_m, scale_m) of ``got`` against want64; a dh_in row of a relu-edge node takes the closer of the two references."""
    err, scale = row_stats(got, ref["want"][tensor])
    if tensor == "dh_in" and ref["want"]["dh_in_alt"] is not None:
        rows = edge_rows(ref)
        err_a, scale_a = row_stats(got[rows], ref["want"]["dh_in_alt"][rows])
        closer = row_ratio(err_a, scale_a) < row_ratio(err[rows], scale[rows])
        err[rows] = torch.where(closer, err_a, err[rows])
        scale[rows] = torch.where(closer, scale_a, scale[rows])
    return err, scale


def ill_rows(ref: Dict, tensor: str) -> torch.Tensor:
    """bool per row: the references alone call the row ill-conditioned (gap_m > CAP / 4 x scale_m)."""
    gap, scale = ref_rows(ref["r32"][tensor], ref, tensor)
    return gap > CAP / 4 * scale


def held(got: torch.Tensor, ref: Dict, tensor: str, probe: str, label: str = ""):
    """Hold ``got`` to the bars, every row.  Returns (worst ratio over the well-conditioned rows, labels of the rows that were held
    to a named rule, failures [(label, row, err, limit)])."""
    bar = BAR[klass(tensor, probe)]
    err, scale = ref_rows(got, ref, tensor)
    gap, gscale = ref_rows(ref["r32"][tensor], ref, tensor)
    ill = gap > CAP / 4 * gscale
    limit = torch.where(ill, ORDER_FACTOR * gap, bar * scale)
    named = [f"{label} {tensor} row {int(i)}: ill-conditioned (gap {float(gap[i]):.2e}, scale {float(gscale[i]):.2e})" for i in torch.nonzero(ill).flatten()]
    if tensor == "dh_in" and ref["want"]["dh_in_alt"] is not None:
        named += [f"{label} dh_in rows of node {int(i)}: an element of hidden sits on the head's relu edge" for i in ref["want"]["edge_nodes"]]
    ratio = row_ratio(err, scale)
    worst = float(ratio[~ill].max()) if bool((~ill).any()) else 0.0
    bad = [(f"{label} {tensor}", int(i), float(err[i]), float(limit[i])) for i in torch.nonzero(~(err <= limit)).flatten()]
    return worst, named, bad


def blend_elements(got_dh: torch.Tensor, ref: Dict) -> float:
    """blend probe: max over every ELEMENT of |dh_in - dhn32 z32| / (sum of |terms| of dhn) z -- held to BAR["dh_in_blend"]."""
    r32 = ref["r32"]
    return B._ratio((got_dh.double() - (r32["dhn"] * r32["z"]).double()).abs(), ref["den_blend"])


def bar_table(cases=None) -> Dict[str, Tuple[float, str]]:
    """class -> (worst ratio of cell32 over the well-conditioned rows, the case and probe that set it)."""
    out = {k: (0.0, "") for k in CLASSES}
    for name in (cases or CASES):
        for probe in PROBES:
            ref = reference(name, probe)
            for tensor in ("hidden", "pred", "dh_in"):
                worst = held(ref["r32"][tensor], ref, tensor, probe)[0]
                k = klass(tensor, probe)
                if worst > out[k][0]:
                    out[k] = (worst, f"{name} {probe}")
    return out


# ---- the dispatch, restated -------------------------------------------------------------------------------------------------------------

def _flat_kernel(mode: int, m: int, ncols: int, ks, nsplit: Optional[int], o: Dict) -> str:
    """gemm_dispatch.hip fast_class + gemm_flat.h launch_fast / launch_flat for [N][K] weight segments of widths ``ks`` (fp32 storage)."""
    fast = ncols % 4 == 0 and all(k % 4 == 0 for k in ks) and sum(B._cdiv(k, B.GBK) for k in ks) <= B.G_MAX_ITERS
    if nsplit is not None and nsplit < ncols and nsplit % B.GBN != 0:       # a column tile must not straddle B0 | B1
        fast = False
    if not fast:
        return "gemm_flat_kernel<vec=1>"
    if mode == 0 and B._cdiv(m, B.GBM) * B._cdiv(ncols, B.GBN) < B.SMALL_TILE_LIMIT:
        return "gemm_flat_small_kernel"
    if mode == 0 and o["fp32_core_wide"]:
        return "gemm_flat_fast_kernel<FastCore>"
    uniform = not o["desc_table"] and all(k % B.GBK == 0 for k in ks)
    return f"gemm_flat_split_kernel<{(0, 3)[mode]}>/{'scalar' if uniform else 'table'}"


def expected_forms(shape, mode: int, options: Optional[Dict] = None) -> Dict[str, str]:
    """shape (N, E, F, T, C, O, ...) -> {"gates", "candidate", "dgrad", "dgrad_candidate", "dgrad_gates", "cell_bwd"}: the kernel of the gate
    GEMM, of the candidate stage, the data-gradient form with the kernels of its GEMMs, and the cell_bwd variant ("-": none runs).
    options: dgrad1_gen (1), fp32_core_wide (0), desc_table (0).  Arithmetics 0 and 1 (fp32 storage; api_step.hip step_form with a
    caller's hidden input: ibf = abf = 0, tcol = false, split = mode != 0 || !fp32_core_wide)."""
    assert mode in MODES, "the cell probe covers the two fp32-storage arithmetics"
    o = dict(dgrad1_gen=1, fp32_core_wide=0, desc_table=0)
    o.update(options or {})
    n, f, t, c = shape[0], shape[2], shape[3], shape[4]
    f += (-f) % 4                                                           # zero feature rows: the kernels read 16-byte rows
    m = n * t
    tiles = B._cdiv(m, B.GBM) * B._cdiv(c, B.GBN)
    out = {"gates": _flat_kernel(mode, m, 2 * c, (c, f), c, o)}
    # gemm_cell.hip launch_gemm_candidate / launch_cand_vec: C % 4 == 0 and F % 4 == 0 always give the vector kernels here
    assert c % 4 == 0 and B._cdiv(c, B.GBK) + B._cdiv(f, B.GBK) <= B.G_MAX_ITERS and t <= 255
    uniform = not o["desc_table"] and c % B.GBK == 0 and f % B.GBK == 0
    three = not o["fp32_core_wide"] and (mode == 1 or tiles >= B.SMALL_TILE_LIMIT)
    if three:
        out["candidate"] = f"gemm_cand_split_kernel<{(0, 3)[mode]}>/{'scalar' if uniform else 'table'}"
    elif mode == 1:
        out["candidate"] = "gemm_cand_flat_kernel<SplitCore<3>>"
    elif tiles < B.SMALL_TILE_LIMIT:
        out["candidate"] = "gemm_cand_flat_kernel<SmallCore>"
    else:
        out["candidate"] = "gemm_cand_flat_kernel<FastCore>"
    split = mode != 0 or not o["fp32_core_wide"]
    # gemm_dispatch.hip gemm_dgrad1_gen_ok
    gen = split and bool(o["dgrad1_gen"]) and not o["fp32_core_wide"] and not o["desc_table"] and c % B.GBN == 0 and c % B.GBK == 0 and \
        tiles >= B.SMALL_TILE_LIMIT and n * c * 4 < (1 << 31)
    if gen:
        out["dgrad"], out["cell_bwd"] = "dgrad1_gen", "-"
        out["dgrad_candidate"] = f"gemm_dgrad1_gen_kernel<{(0, 3)[mode]}>"
    else:
        out["dgrad"], out["cell_bwd"] = "two-launch", "cell_bwd_kernel"
        out["dgrad_candidate"] = _flat_kernel(mode, m, c, (c,), None, o) if split else "gemm_flat_fast_kernel<FastCore>"
    out["dgrad_gates"] = _flat_kernel(mode, m, c, (c, c), None, o) if split else "gemm_flat_fast_kernel<FastCore>"
    return out


def form_label(forms: Dict[str, str]) -> str:
    return " | ".join(f"{k} {forms[k]}" for k in ("gates", "candidate", "dgrad", "dgrad_candidate", "dgrad_gates", "cell_bwd"))


# every name the table must reach, per arithmetic (default environment; the environment-only switches stay out)
FORM_NAMES = {
    0: {"gates": {"gemm_flat_kernel<vec=1>", "gemm_flat_small_kernel", "gemm_flat_split_kernel<0>/scalar", "gemm_flat_split_kernel<0>/table"},
        "candidate": {"gemm_cand_flat_kernel<SmallCore>", "gemm_cand_split_kernel<0>/scalar"},
        "dgrad": {"two-launch", "dgrad1_gen"},
        "dgrad_candidate": {"gemm_flat_small_kernel", "gemm_flat_split_kernel<0>/scalar", "gemm_dgrad1_gen_kernel<0>"},
        "dgrad_gates": {"gemm_flat_small_kernel", "gemm_flat_split_kernel<0>/scalar"},
        "cell_bwd": {"cell_bwd_kernel", "-"}},
    1: {"gates": {"gemm_flat_kernel<vec=1>", "gemm_flat_split_kernel<3>/scalar", "gemm_flat_split_kernel<3>/table"},
        "candidate": {"gemm_cand_split_kernel<3>/scalar", "gemm_cand_split_kernel<3>/table"},
        "dgrad": {"two-launch", "dgrad1_gen"},
        "dgrad_candidate": {"gemm_flat_split_kernel<3>/scalar", "gemm_flat_split_kernel<3>/table", "gemm_dgrad1_gen_kernel<3>"},
        "dgrad_gates": {"gemm_flat_split_kernel<3>/scalar", "gemm_flat_split_kernel<3>/table"},
        "cell_bwd": {"cell_bwd_kernel", "-"}},
}


def runs(name: str) -> List[Tuple[int, int]]:
    """(mode, dgrad1_gen) settings of one case: both settings of the switch where it changes the form, the default otherwise."""
    out = []
    for mode in MODES:
        both = expected_forms(CASES[name], mode, {"dgrad1_gen": 1}) != expected_forms(CASES[name], mode, {"dgrad1_gen": 0})
        out += [(mode, g) for g in (GEN_OPTIONS if both else GEN_OPTIONS[:1])]
    return out


def table_forms() -> Dict[int, Dict[str, set]]:
    out = {mode: {k: set() for k in FORM_NAMES[mode]} for mode in MODES}
    for name in CASES:
        for mode, g in runs(name):
            for k, v in expected_forms(CASES[name], mode, {"dgrad1_gen": g}).items():
                out[mode][k].add(v)
    return out


def cell_launches(gen: bool) -> List[str]:
    """The launcher calls of one regt_cell_forward + regt_cell_backward in fp32 storage (api_step.hip forward_impl / backward_impl with
    a caller's hidden input, a skinny last head layer and an attention gradient), as tests/golden/step_plan.txt names them."""
    fwd = ["forward", "side_fork", "launch_softmax_small", "launch_small_gemm_multi", "launch_pack_x", "launch_spmm_csr", "side_join",
           "launch_gemm_gates", "launch_gemm_candidate", "launch_gemm_bias_act", "launch_head2_fwd"]
    head = ["backward", "launch_head2_bwd", "side_fork", "launch_head2_wgrad", "launch_wgrad", "launch_gemm_mask_add", "launch_transpose3"]
    if gen:
        data = ["launch_gemm_dgrad1_gen", "side_fork", "launch_rowdot_reduce", "launch_att_bwd"]
    else:
        data = ["launch_cell_bwd", "side_fork", "launch_att_bwd", "launch_gemm_dgrad1"]
    tail = ["launch_gemm_dgrad2"] + ["launch_wgrad"] * 4 + ["side_join", "launch_wgrad_reduce_multi", "launch_small_gemm_multi"]
    return fwd + head + data + tail


# ---- the cell on the device (tests/test_gpu_cell_bars.py, tools/cell_bars.py) ------------------------------------------------------------

_DEVICE: Dict = {}


def device_case(R, name: str):
    """The prepared operator of one case on the device and its CSR on the host (shared by every probe and mode)."""
    if name not in _DEVICE:
        ei, ew = graph(name)
        op = R.graph.prepare_gcn_operator(ei.cuda(), ew.cuda(), CASES[name][0])
        _DEVICE[name] = (op, (op.rowptr.cpu(), op.col.cpu(), op.val.cpu()))
    return _DEVICE[name]


def run_hip(R, name: str, probe: str):
    """One CellFunction.apply + backward: (pred, hidden, dh_in) on the host.  A feature width that is no multiple of 4 gets zero feature
    rows and zero weight columns, as the modules of the package pad it."""
    op, _csr = device_case(R, name)
    p = params(name, probe)
    x, h_in, gh, gp = inputs(name, probe)
    pad = (-x.shape[1]) % 4
    if pad:
        x = torch.nn.functional.pad(x, (0, 0, 0, pad)).contiguous()
        for k in "zrh":
            key = f"tgnn._base_tgcn.conv_{k}.lin.weight"
            p[key] = torch.nn.functional.pad(p[key], (0, pad)).contiguous()
    h = h_in.cuda().requires_grad_(True)
    tens = [p[k].cuda() for k in R.functional.PARAM_NAMES_CELL]
    pred, hidden = R.functional.CellFunction.apply(x.cuda(), h, op, *tens)
    ((hidden * gh.cuda()).sum() + (pred * gp.cuda()).sum()).backward()
    torch.cuda.synchronize()
    return pred.detach().cpu(), hidden.detach().cpu(), h.grad.cpu()


def measure(R, name: str, probe: str, mode: int, gen: int) -> Dict:
    """One case, probe, arithmetic and switch setting on the device: runs it (twice where the sums are ordered: T <= 64), holds every
    row.  Returns {"forms", "ratios": {tensor: worst}, "named", "bad", "blend": per-element ratio | None, "identical": bool | None}."""
    lib = R.load_library()
    _op, csr = device_case(R, name)
    ref = reference(name, probe, csr)
    prev_mode = lib.regt_set_gemm_mode(mode)
    prev_gen = lib.regt_set_option(b"dgrad1_gen", gen)
    try:
        got = run_hip(R, name, probe)
        # (T > 64: a node spans three or more 64-row blocks and the order of the float atomics into hidden shows in the last bits)
        again = run_hip(R, name, probe) if CASES[name][3] <= 64 else None
    finally:
        lib.regt_set_option(b"dgrad1_gen", prev_gen)
        lib.regt_set_gemm_mode(prev_mode)
    out = {"forms": expected_forms(CASES[name], mode, {"dgrad1_gen": gen}), "ratios": {}, "named": [], "bad": [], "blend": None,
           "identical": None if again is None else all(torch.equal(a, b) for a, b in zip(got, again))}
    label = f"{name} {probe} mode {mode} dgrad1_gen {gen}"
    for tensor, g in zip(("pred", "hidden", "dh_in"), got):
        if not bool(torch.isfinite(g).all()):
            out["bad"].append((f"{label} {tensor}", -1, float("nan"), 0.0))
        worst, named, bad = held(g, ref, tensor, probe, label)
        out["ratios"][tensor] = worst
        out["named"] += named
        out["bad"] += bad
    if probe == "blend":
        out["blend"] = blend_elements(got[2], ref)
    return out


def restatement_ratios(name: str, probe: str) -> Dict[str, float]:
    """cell32's own worst ratio per tensor (well-conditioned rows), for the profile."""
    ref = reference(name, probe)
    return {tensor: held(ref["r32"][tensor], ref, tensor, probe)[0] for tensor in ("pred", "hidden", "dh_in")}
