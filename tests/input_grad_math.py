"""The whole-model input gradient dL/dx of RegionalTemporalGCN / TemporalGCN (regt_input_gradient), restated.

Test helper only (like tgcn_math.py).  With rows m = node T + t, the pre-activation gradients the backward leaves behind -- dzr = [dp_z | dp_r]
(M, 2C), dhp (M, C), ds (M, C) = the embedding's; in the collapsed TemporalGCN form dh, the gradient of the hidden input without the
gates' linear term -- and the composed weights of fused_math.compose:

    dAX = dzr [Gz; Gr] + dhp Gh
    dXd = ds A0                       collapsed: dh W0 + dzr P0zr          P0zr = [Uz2; Ur2] W0
    dLX = ds A_region(node)           collapsed: dh W1 + dzr P1zr          P1zr = [Uz2; Ur2] W1
    dXp = dXd + A_hat^T dAX + L~^T dLX                                     (N, T F) packed rows; L~ = the merged regional Laplacians
    dx (N, F, T) = unpack(dXp)

``restate`` takes the four gradients from autograd through fused_math.forward_fused (taps on the pre-activations) in the dtype of the
parameters and evaluates the five formulas with explicit (dense) transposed operators; ``transposed=False`` plants the error a missing
transpose would make.  The truth is ``reference(name)["dx"]``: float64 torch.autograd through oracle/model.py with x.requires_grad.

Cases: the smallest shapes that reach every edge of csrc/model_dx.hip and csrc/spmm_dual_t.hip -- (N, T) = (130, 1) a tile tail, (43, 3) a
node straddling the 128-row tile, (9, 150) T > 64 and rows wider than one column pass (T F = 4800 floats at F = 32); C = 16 (K below one
chunk), 48 (a tail chunk), 256; F = 7 (padded), 8, 32, 36, 64 (one and two accumulators per output, a partial second one); R = 1, R = 3 with
sorted and with shuffled region ids (region-pure tiles, the per-region passes); TemporalGCN collapsed and not; fp32 and bf16x3; a 2-copy
block-diagonal graph.  The graph follows _graph() of tests/test_gpu_tgcn_cell.py -- two isolated nodes, a node with in-edges only, a
duplicate edge, a self loop -- plus a node with out-edges only, with asymmetric random weights.

Bar for a row of dx viewed as (N, T F): err_n <= bar x max |want64[n, :]|, a row that is 0 in float64 must be 0.  ``bar()`` follows the
project's rule: the worst row ratio of the fp32 restatement over every case, x 4 (the summation-order allowance of cell_probe / op_bars);
if that is within cell_probe.BAR["dh_in"] the bar is that one, else 4 x the measured value.  Nothing is derived from the kernels' output.
The head's two relus: a case whose float64 ``hidden`` or inner pre-activation has an element within EDGE of 0 (relative to its row) could
take a mask either way in fp32; tests/test_input_grad_cpu.py asserts that no case has one, so the reference needs no second branch."""
from __future__ import annotations

from typing import Dict

import torch

import cell_probe as CP
import fused_math as FM
from oracle import model as M

ORDER_FACTOR = 4.0
EDGE = CP.BAR["hidden"]

# name -> model, N (per copy), T, F, C, R, region order, tgcn_collapse, arithmetic (0 fp32, 1 bf16x3), copies, and `salt`: which of the
# seeded input draws the case uses -- the first whose float64 forward keeps both head relus 4 x EDGE off their edge (find_salt below
# re-derives it; decided by the float64 oracle alone, asserted in tests/test_input_grad_cpu.py)
CASES: Dict[str, Dict] = {
    "regt-N130-T1-F8-C16-sorted": dict(model="regional", n=130, t=1, f=8, c=16, r=3, order="sorted", collapse=1, mode=0, copies=1, salt=1),
    "regt-N43-T3-F7-C48-shuffled": dict(model="regional", n=43, t=3, f=7, c=48, r=3, order="shuffled", collapse=1, mode=0, copies=1, salt=5),
    "regt-N43-T3-F36-C256-shuffled-bf16x3": dict(model="regional", n=43, t=3, f=36, c=256, r=3, order="shuffled", collapse=1, mode=1, copies=1, salt=5),
    "regt-N9-T150-F8-C16-R1": dict(model="regional", n=9, t=150, f=8, c=16, r=1, order="sorted", collapse=1, mode=0, copies=1, salt=0),
    "regt-N130-T1-F64-C48-sorted": dict(model="regional", n=130, t=1, f=64, c=48, r=3, order="sorted", collapse=1, mode=0, copies=1, salt=65),
    "regt-N43-T3-F32-C256-sorted": dict(model="regional", n=43, t=3, f=32, c=256, r=3, order="sorted", collapse=1, mode=0, copies=1, salt=43),
    "regt-N43-T3-F8-C48-sorted-2copies": dict(model="regional", n=43, t=3, f=8, c=48, r=3, order="sorted", collapse=1, mode=0, copies=2, salt=5),
    "tgcn-N130-T1-F8-C48-collapsed": dict(model="tgcn", n=130, t=1, f=8, c=48, r=1, order="sorted", collapse=1, mode=0, copies=1, salt=1),
    "tgcn-N43-T3-F36-C16-uncollapsed": dict(model="tgcn", n=43, t=3, f=36, c=16, r=1, order="sorted", collapse=0, mode=0, copies=1, salt=4),
    "tgcn-N9-T150-F32-C16-collapsed": dict(model="tgcn", n=9, t=150, f=32, c=16, r=1, order="sorted", collapse=1, mode=0, copies=1, salt=1),
    "tgcn-N43-T3-F64-C256-collapsed-bf16x3": dict(model="tgcn", n=43, t=3, f=64, c=256, r=1, order="sorted", collapse=1, mode=1, copies=1, salt=9),
    "tgcn-N130-T1-F7-C256-uncollapsed-bf16x3": dict(model="tgcn", n=130, t=1, f=7, c=256, r=1, order="sorted", collapse=0, mode=1, copies=1, salt=78),
}
OUT = 2           # output_dim of every case


def _seed(name: str) -> int:
    return 100 + list(CASES).index(name)


def base_graph(n: int, seed: int = 0):
    """_graph() of tests/test_gpu_tgcn_cell.py: nodes n - 1 and n - 2 are isolated, node n - 3 receives edges and sends none, one duplicate
    edge, one self loop -- and node 0 sends edges and receives none.  Weights 0.5 + U[0, 1) per edge: asymmetric."""
    g = torch.Generator().manual_seed(100 + seed)
    e = 4 * n
    src = torch.randint(0, n - 3, (e,), generator=g)
    dst = torch.randint(1, n - 2, (e,), generator=g)
    dst[0] = n - 3
    src[1], dst[1] = 1, 1
    src[2], dst[2] = src[3], dst[3]
    src[4] = 0
    return torch.stack([src, dst]), 0.5 + torch.rand(e, generator=g)


def graph(name: str):
    """(edge_index, edge_weight, [region edge_index], [region weights]) of ONE copy.  Regional: region k holds the edges whose two ends
    lie in part k (node-disjoint), with weights of their own; parts ascend with the node number or are drawn at random ("shuffled": the
    region ids the package derives are then not sorted by node)."""
    c = CASES[name]
    n, r = c["n"], c["r"]
    ei, ew = base_graph(n, _seed(name))
    if c["model"] == "tgcn":
        return ei, ew, [ei], [ew]
    g = torch.Generator().manual_seed(7000 + _seed(name))
    part = torch.arange(n) * r // n if c["order"] == "sorted" else torch.randint(0, r, (n,), generator=g)
    wr = 0.5 + torch.rand(ei.shape[1], generator=g)
    ri, rw = [], []
    for k in range(r):
        keep = (part[ei[0]] == k) & (part[ei[1]] == k)
        assert int(keep.sum()) > 0, f"{name}: region {k} has no edge"
        ri.append(ei[:, keep].contiguous())
        rw.append(wr[keep].contiguous())
    return ei, None, ri, rw


def replicate(ei, w, copies: int, n: int):
    """``copies`` disjoint copies of a graph on the host (graph.replicate_edges, restated)."""
    if copies == 1:
        return ei, w
    off = (torch.arange(copies) * n).view(copies, 1, 1)
    e2 = (ei.unsqueeze(0) + off).permute(1, 0, 2).reshape(2, -1).contiguous()
    return e2, (None if w is None else w.repeat(copies).contiguous())


def full_graph(name: str):
    """The graph of all copies: (edge_index, edge_weight, region index list, region weight list, nodes)."""
    c = CASES[name]
    ei, ew, ri, rw = graph(name)
    n, b = c["n"], c["copies"]
    ei2, ew2 = replicate(ei, ew, b, n)
    rep = [replicate(i, w, b, n) for i, w in zip(ri, rw)]
    return ei2, ew2, [q[0] for q in rep], [q[1] for q in rep], n * b


def params(name: str) -> Dict[str, torch.Tensor]:
    c = CASES[name]
    model = "RegionalTemporalGCN" if c["model"] == "regional" else "TemporalGCN"
    return M.init_params(model, c["f"], c["t"], OUT, num_nodes=c["n"] * c["copies"], num_regions=c["r"], seed=_seed(name), hidden=c["c"])


def inputs(name: str):
    """(x (N, F, T), g1 (N, O), g2 (N, C)): loss = (pred g1).sum() + (hidden g2).sum()."""
    c = CASES[name]
    n = c["n"] * c["copies"]
    g = torch.Generator().manual_seed(9000 + _seed(name) + 1000 * c["salt"])
    return torch.rand(n, c["f"], c["t"], generator=g), torch.randn(n, OUT, generator=g), torch.randn(n, c["c"], generator=g)


def oracle(name: str, p, x, regional: bool):
    ei, ew, ri, rw, _n = full_graph(name)
    dt = x.dtype
    if regional:
        return M.regional_temporal_gcn(p, x, ei, ri, [w.to(dt) for w in rw])
    return M.temporal_gcn(p, x, ei, ew.to(dt))


def node_region_of(ls) -> torch.Tensor:
    """The region whose Laplacian has entries in a node's row (0 where none has: such a row multiplies nothing)."""
    has = torch.stack([(l.abs().sum(dim=1) > 0) for l in ls], dim=1)
    assert int(has.sum(dim=1).max()) <= 1, "regions are not node-disjoint"
    return has.float().argmax(dim=1)


def restate(p, x, a, ls, regional: bool, g1, g2, collapsed: bool = False, transposed: bool = True):
    """dx (N, F, T) by the five formulas in the dtype of ``p``; ``a`` (N, N) = A_hat and ``ls`` the dense L~_r."""
    taps = {}

    def tap(key, v):
        if key == "h":                      # what the reset product and the blend read: its gradient is dh without the gates' linear term
            v = v * 1.0
        if key in ("pre", "pz", "pr", "ph", "h"):
            v.retain_grad()
            taps[key] = v
        return v

    xl = x.clone().requires_grad_(True)
    pred, hidden = FM.forward_fused(p, xl, a, ls, regional=regional, tap=tap)
    ((pred * g1).sum() + (hidden * g2).sum()).backward()
    w = FM.compose(p, len(ls), regional)
    dzr = torch.cat([taps["pz"].grad, taps["pr"].grad], dim=-1)              # (N, T, 2C)
    dhp, ds, dh = taps["ph"].grad, taps["pre"].grad, taps["h"].grad
    d_ax = dzr @ torch.cat([w["Gz"], w["Gr"]], dim=0) + dhp @ w["Gh"]
    if collapsed:
        assert not regional
        u2 = torch.cat([w["Uz"], w["Ur"]], dim=0)                            # (2C, C)
        d_xd = dh @ w["A0"] + dzr @ (u2 @ w["A0"])
        d_lx = dh @ w["Ar"][0] + dzr @ (u2 @ w["Ar"][0])
    else:
        d_xd = ds @ w["A0"]
        d_lx = torch.einsum("ntc,ncf->ntf", ds, torch.stack(w["Ar"])[node_region_of(ls)])
    lm = sum(ls)
    pull = "ji,jtf->itf" if transposed else "ij,jtf->itf"
    d_xp = d_xd + torch.einsum(pull, a, d_ax) + torch.einsum(pull, lm, d_lx)
    return d_xp.permute(0, 2, 1).contiguous(), xl.grad


_REFS: Dict = {}


def reference(name: str) -> Dict:
    """{"x", "g1", "g2", "p", "dx" (float64, oracle autograd), "pred", "hidden", "grads" (float64), "edge": closest relative distance of
    an element of hidden / of the head's inner pre-activation to 0, "r32": the fp32 restatement's dx, "plain64": the float64 restatement
    with the untransposed operators}.  Computed once and shared; nothing in it is changed by a test."""
    if name in _REFS:
        return _REFS[name]
    c = CASES[name]
    regional = c["model"] == "regional"
    p = params(name)
    x, g1, g2 = inputs(name)
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    x64 = x.double().requires_grad_(True)
    pred, hidden = oracle(name, p64, x64, regional)
    ((pred * g1.double()).sum() + (hidden * g2.double()).sum()).backward()
    pre1 = torch.relu(hidden.detach()) @ p64["linear1.weight"].detach().t() + p64["linear1.bias"].detach()
    rel0 = lambda v: float((v.abs() / v.abs().amax(dim=1, keepdim=True)).min())      # noqa: E731
    ei, ew, ri, rw, n = full_graph(name)
    out = {"x": x, "g1": g1, "g2": g2, "p": p, "dx": x64.grad.detach(), "pred": pred.detach(), "hidden": hidden.detach(),
           "grads": {k: (None if v.grad is None else v.grad.detach()) for k, v in p64.items()}, "edge": min(rel0(hidden.detach()), rel0(pre1))}
    collapsed = (not regional) and bool(c["collapse"])
    for key, dt, tr in (("r64", torch.float64, True), ("plain64", torch.float64, False), ("r32", torch.float32, True)):
        a, ls = FM.dense_ops(ei, None if ew is None else ew.to(dt), ri, [w.to(dt) for w in rw], n, dt)
        pd = {k: v.to(dt) for k, v in p.items()}
        out[key], auto = restate(pd, x.to(dt), a, ls, regional, g1.to(dt), g2.to(dt), collapsed=collapsed, transposed=tr)
        if key == "r64":
            out["fused_autograd64"] = auto
    _REFS[name] = out
    return out


def rows(t: torch.Tensor) -> torch.Tensor:
    """(N, F, T) -> the node's row (N, T F)."""
    return t.reshape(t.shape[0], -1)


def worst_row_ratio(got: torch.Tensor, want64: torch.Tensor) -> float:
    err, scale = CP.row_stats(rows(got), rows(want64))
    return float(CP.row_ratio(err, scale).max())


_BAR: Dict = {}


def measured_fp32() -> Dict[str, float]:
    """case -> worst row ratio of the fp32 restatement against float64."""
    return {name: worst_row_ratio(reference(name)["r32"], reference(name)["dx"]) for name in CASES}


def bar() -> float:
    if "bar" not in _BAR:
        worst = max(measured_fp32().values())
        _BAR["bar"] = CP.BAR["dh_in"] if ORDER_FACTOR * worst <= CP.BAR["dh_in"] else ORDER_FACTOR * worst
    return _BAR["bar"]


def held(got: torch.Tensor, want64: torch.Tensor, what: str) -> float:
    """Every row of ``got`` (N, F, T) within bar() of its float64 row's scale, exactly 0 where that is 0.  Returns the worst ratio."""
    assert tuple(got.shape) == tuple(want64.shape), (what, tuple(got.shape), tuple(want64.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err, scale = CP.row_stats(rows(got), rows(want64))
    ratio = CP.row_ratio(err, scale)
    worst = float(ratio.max())
    print(f"{what}: worst row ratio {worst:.3e} (bar {bar():.3e})")
    bad = torch.nonzero(~(err <= bar() * scale)).flatten()
    assert bad.numel() == 0, f"{what}: rows {bad.tolist()[:8]} over the bar, worst ratio {worst:.3e} > {bar():.3e}"
    return worst


def relu_edge(name: str, salt: int) -> float:
    """Closest relative distance to 0 of an element of the float64 hidden state / of the head's inner pre-activation for input draw ``salt``."""
    c = CASES[name]
    p64 = {k: v.double() for k, v in params(name).items()}
    g = torch.Generator().manual_seed(9000 + _seed(name) + 1000 * salt)
    x = torch.rand(c["n"] * c["copies"], c["f"], c["t"], generator=g).double()
    with torch.no_grad():
        _pred, hidden = oracle(name, p64, x, c["model"] == "regional")
        pre1 = torch.relu(hidden) @ p64["linear1.weight"].t() + p64["linear1.bias"]
    rel0 = lambda v: float((v.abs() / v.abs().amax(dim=1, keepdim=True)).min())      # noqa: E731
    return min(rel0(hidden), rel0(pre1))


def find_salt(name: str, limit: int = 200) -> int:
    """The first input draw whose float64 forward keeps both head relus 4 x EDGE off their edge: what CASES[name]["salt"] records."""
    for salt in range(limit):
        if relu_edge(name, salt) > 4 * EDGE:
            return salt
    raise AssertionError(f"{name}: no draw below {limit} keeps the relus off their edge")


# ---- the cases on the device (tests/test_gpu_input_grad.py, tools/input_grad_bench.py) ------------------------------------------------------

ARITH = {0: "fp32", 1: "bf16x3"}
_GRAPHS: Dict = {}


def device_module(R, name: str):
    c = CASES[name]
    n = c["n"] * c["copies"]
    if c["model"] == "regional":
        mod = R.RegionalTemporalGCN(node_features=c["f"], num_nodes=n, periods=c["t"], output_dim=OUT, num_regions=c["r"], hidden_channels=c["c"])
    else:
        mod = R.TemporalGCN(node_features=c["f"], periods=c["t"], output_dim=OUT, hidden_channels=c["c"])
    mod.load_state_dict(params(name), strict=True)
    mod.arithmetic = ARITH[c["mode"]]
    return mod.cuda()


def device_graph(R, name: str):
    """The prepared graph of a case (all copies), shared."""
    if name not in _GRAPHS:
        c = CASES[name]
        ei, ew, ri, rw = graph(name)
        if c["model"] == "regional":
            _GRAPHS[name] = R.prepare_graph(ei.cuda(), None, [t.cuda() for t in ri], [t.cuda() for t in rw], c["n"], c["copies"])
        else:
            _GRAPHS[name] = R.prepare_graph(ei.cuda(), ew.cuda(), [ei.cuda()], [ew.cuda()], c["n"], c["copies"])
    return _GRAPHS[name]


class collapse_option:
    """regt_set_option("tgcn_collapse", .) as the case names it, for the body."""

    def __init__(self, R, name: str):
        self.lib, self.v = R.load_library(), CASES[name]["collapse"]

    def __enter__(self):
        self.prev = self.lib.regt_set_option(b"tgcn_collapse", self.v)

    def __exit__(self, *exc):
        self.lib.regt_set_option(b"tgcn_collapse", self.prev)


def run_hip(R, name: str, x_grad: bool = True) -> Dict:
    """One module call and backward on the device: {pred, hidden, dx | None, grads} on the host."""
    ref = reference(name)
    mod = device_module(R, name)
    x = ref["x"].cuda().requires_grad_(x_grad)
    with collapse_option(R, name):
        pred, hidden = mod.forward_prepared(x, device_graph(R, name))
        ((pred * ref["g1"].cuda()).sum() + (hidden * ref["g2"].cuda()).sum()).backward()
    torch.cuda.synchronize()
    return {"pred": pred.detach().cpu(), "hidden": hidden.detach().cpu(), "dx": None if x.grad is None else x.grad.cpu(),
            "grads": {k: (None if v.grad is None else v.grad.cpu()) for k, v in mod.named_parameters()}}
