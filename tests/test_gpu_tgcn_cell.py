"""The callable TGCN cell on the device (nn.TGCN.forward, functional.TGCNStepFunction, regt_tgcn_*): the reference's golden, bit identity
with the regt_cell_* path at T = 1, per-row bars on h', dx and dh_in against the float64 restatement (tests/tgcn_math.py), poisoned and
strided buffers, a three-step recurrence, and the inner modules of the two whole models.

Bars.  No constant of its own: h' rows are held to cell_probe.BAR["hidden"], rows of dx and dh_in to cell_probe.BAR["dh_in"] (err_m <=
bar x max_c |want64[m, c]|, a row that is 0 in float64 must be 0), parameter gradients to grad_bars.REL per block.  dh_in is the quantity
that bar was set for (contractions of length C and 2C); a row of dx is a contraction of length 3C <= 768 followed by the row's in-degree of
A_hat^T (<= 30 here), both inside what the bar's x 4 order allowance over the fp32 restatement's own 7.7e-6 covers; the measured ratios
are in profiles/tgcn_cell.txt."""
import numpy as np
import pytest
import torch

import cell_probe as CP
import grad_bars as GB
import regtgcn_amd as R
import tgcn_math as TM
from conftest import load_npz, region_lists
from oracle import model as M
from regtgcn_amd import _lib
from regtgcn_amd import functional as Fn

pytestmark = pytest.mark.gpu
Q = "tgnn._base_tgcn."


def _graph(n: int, seed: int = 0):
    """Nodes n - 1 and n - 2 are isolated, node n - 3 receives edges and sends none; one duplicate edge, one pre-existing self loop."""
    if n < 8:
        return torch.zeros(2, 1, dtype=torch.long), torch.full((1,), 1.5)
    g = torch.Generator().manual_seed(100 + seed)
    e = 4 * n
    src = torch.randint(0, n - 3, (e,), generator=g)
    dst = torch.randint(0, n - 2, (e,), generator=g)
    dst[0] = n - 3
    src[1], dst[1] = 1, 1
    src[2], dst[2] = src[3], dst[3]
    return torch.stack([src, dst]), 0.5 + torch.rand(e, generator=g)


def _params(c: int, f: int, seed: int = 3):
    p = M.init_params("TemporalGCN", f, 1, 1, seed=seed, hidden=c)
    return {k[len(Q):]: v for k, v in p.items() if k.startswith(Q)}


def _cell(p, f: int, c: int):
    cell = R.nn.TGCN(f, c)
    cell.load_state_dict(p, strict=True)
    return cell.cuda()


def _grads(cell):
    return {k: v.grad.detach().cpu() for k, v in cell.named_parameters()}


def _rows_held(got, want64, bar, what):
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err, scale = CP.row_stats(got.cpu(), want64)
    ratio = CP.row_ratio(err, scale)
    print(f"{what}: worst row ratio {float(ratio.max()):.3e} (bar {bar:.3e})")
    bad = torch.nonzero(~(err <= bar * scale)).flatten()
    assert bad.numel() == 0, f"{what}: rows {bad.tolist()[:8]} over the bar, worst ratio {float(ratio.max()):.3e} > {bar:.3e}"


# ---- the reference's golden -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["unit", "weighted"])
def test_golden_cell(tag):
    g = load_npz("golden_cell.npz")
    p = {k[3:].replace("__", "."): torch.from_numpy(v) for k, v in g.items() if k.startswith("p__")}
    cell = _cell(p, 8, 16)
    ei = torch.from_numpy(g["edge_index"]).cuda()
    ew = None if tag == "unit" else torch.from_numpy(g["edge_weight"]).cuda()
    out = cell(torch.from_numpy(g["x"]).cuda(), ei, ew, torch.from_numpy(g["h"]).cuda())
    np.testing.assert_allclose(out.detach().cpu().numpy(), g[f"out_{tag}"], atol=1e-5)
    (out ** 2).sum().backward()
    want = {k: torch.from_numpy(g[f"g_{tag}__" + k.replace(".", "__")]).double() for k in p}
    GB.assert_grads_to_scale(_grads(cell), want, what=f"golden_cell {tag}")


# ---- bit identity with regt_cell_forward / regt_cell_backward at T = 1 -----------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("f", [8, 32])
def test_bit_identical_to_the_cell_path_at_one_period(f, mode):
    n, c = 130, 256
    lib = R.load_library()
    ei, ew = _graph(n)
    p = _params(c, f)
    gen = torch.Generator().manual_seed(7)
    x, h, gh = torch.rand(n, f, generator=gen).cuda(), (0.5 * torch.randn(n, c, generator=gen)).cuda(), torch.randn(n, c, generator=gen).cuda()
    op = R.graph.prepare_gcn_operator(ei.cuda(), ew.cuda(), n)
    prev = lib.regt_set_gemm_mode(mode)
    try:
        cell = _cell(p, f, c)
        hl = h.clone().requires_grad_(True)
        out = cell.forward_prepared(x, op, hl)
        (out * gh).sum().backward()
        # the existing path: one-logit attention, any finite head with O = 1, H1 = 4, dpred = 0 (pred is not used by the loss)
        full = {Q + k: v.cuda().requires_grad_(True) for k, v in p.items()}
        full["tgnn._attention"] = torch.full((1,), 0.3).cuda()
        for k, shp in (("linear1.weight", (4, c)), ("linear1.bias", (4,)), ("linear2.weight", (1, 4)), ("linear2.bias", (1,))):
            full[k] = (0.1 * torch.randn(shp, generator=gen)).cuda()
        h2 = h.clone().requires_grad_(True)
        _pred, hidden = Fn.CellFunction.apply(x.view(n, f, 1), h2, op, *[full[k] for k in Fn.PARAM_NAMES_CELL])
        (hidden * gh).sum().backward()
        assert torch.equal(out, hidden)
        assert torch.equal(hl.grad, h2.grad)
        for k, v in cell.named_parameters():
            assert torch.equal(v.grad, full[Q + k].grad), k
        with torch.no_grad():
            assert torch.equal(cell.forward_prepared(x, op, h), out)          # the forward-only call
            none, zeros = cell.forward_prepared(x, op, None), cell.forward_prepared(x, op, torch.zeros_like(h))
        assert torch.equal(none, zeros)
        assert torch.equal(cell.forward_prepared(x, op, None), zeros)        # ... and the training call without H
    finally:
        lib.regt_set_gemm_mode(prev)


# ---- per-row bars against float64 ------------------------------------------------------------------------------------------------------------

CASES = [(1, 256, 8), (63, 256, 8), (130, 256, 7), (130, 256, 10), (130, 256, 32), (130, 256, 64), (130, 16, 8)]


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("n,c,f", CASES, ids=[f"N{n}-C{c}-F{f}" for n, c, f in CASES])
def test_rows_of_output_dx_and_dh_against_float64(n, c, f, weighted):
    ei, ew = _graph(n)
    ew = ew if weighted else None
    p = _params(c, f)
    gen = torch.Generator().manual_seed(11)
    x, h, gh = torch.rand(n, f, generator=gen), 0.5 * torch.randn(n, c, generator=gen), torch.randn(n, c, generator=gen)
    op = R.graph.prepare_gcn_operator(ei.cuda(), None if ew is None else ew.cuda(), n)
    if n >= 8:          # node n - 3 sends no edge: its row of A_hat^T is its self loop alone, so its dx row is exactly that term
        t_rp = op.t_rowptr.cpu()
        assert int(t_rp[n - 2] - t_rp[n - 3]) == 1 and int(op.t_col[int(t_rp[n - 3])]) == n - 3
    cell = _cell(p, f, c)
    xl, hl = x.cuda().requires_grad_(True), h.cuda().requires_grad_(True)
    out = cell.forward_prepared(xl, op, hl)
    (out * gh.cuda()).sum().backward()
    a = TM.dense_from_csr(op.rowptr, op.col, op.val, n)
    p64 = {k: v.double() for k, v in p.items()}
    s = TM.step(p64, a, x.double(), h.double())
    dx, dh, grads = TM.backward(p64, a, s, gh.double())
    what = f"N{n} C{c} F{f} {'weighted' if weighted else 'unit'}"
    assert tuple(xl.grad.shape) == (n, f)
    _rows_held(out.detach(), s["out"], CP.BAR["hidden"], what + " h_out")
    _rows_held(hl.grad, dh, CP.BAR["dh_in"], what + " dh_in")
    _rows_held(xl.grad, dx, CP.BAR["dh_in"], what + " dx")
    GB.assert_grads_to_scale(_grads(cell), grads, what=what)


# ---- poisoned and strided buffers ------------------------------------------------------------------------------------------------------------

def test_poisoned_gradient_buffers_and_unwanted_gradients():
    from regtgcn_amd import ops
    n, c, f = 130, 256, 8
    ei, ew = _graph(n)
    p = _params(c, f)
    gen = torch.Generator().manual_seed(13)
    x, h, gh = torch.rand(n, f, generator=gen).cuda(), (0.5 * torch.randn(n, c, generator=gen)).cuda(), torch.randn(n, c, generator=gen).cuda()
    op = R.graph.prepare_gcn_operator(ei.cuda(), ew.cuda(), n)
    cell = _cell(p, f, c)
    xl, hl = x.clone().requires_grad_(True), h.clone().requires_grad_(True)
    out = cell.forward_prepared(xl, op, hl)
    (out * gh).sum().backward()
    # the same call through the wrappers, into buffers full of NaN
    tens = [t.detach() for t in cell._cell_params()]
    out2, st = Fn._tgcn_forward_call(x, h, op, tens, False)
    grads = {k: torch.full_like(t, float("nan")) for k, t in zip(Fn.PARAM_NAMES_TGCN, tens)}
    dx, dh = torch.full((n, f), float("nan")).cuda(), torch.full((n, c), float("nan")).cuda()
    ops.tgcn_backward(st.dims, st.gs, st.ps, Fn._fill(_lib.Grads(), grads, False), gh, h, out2, op, dx, dh, st.handle.ws)
    assert torch.equal(out2, out) and torch.equal(dx, xl.grad) and torch.equal(dh, hl.grad)
    for k, v in zip(Fn.PARAM_NAMES_TGCN, cell._cell_params()):
        assert torch.equal(grads[k], v.grad), k
    # no gradient is asked of x or H: none is produced, the parameter gradients are the same bits
    cell2 = _cell(p, f, c)
    x2, h2 = x.clone(), h.clone()
    (cell2.forward_prepared(x2, op, h2) * gh).sum().backward()
    assert x2.grad is None and h2.grad is None
    for (k, v), (_, w) in zip(cell.named_parameters(), cell2.named_parameters()):
        assert torch.equal(v.grad, w.grad), k


def test_strided_period_view_equals_its_contiguous_copy():
    n, c, f, t = 130, 256, 8, 3
    ei, ew = _graph(n)
    p = _params(c, f)
    gen = torch.Generator().manual_seed(17)
    xs, gh = torch.rand(n, f, t, generator=gen).cuda(), torch.randn(n, c, generator=gen).cuda()
    cell_a, cell_b = _cell(p, f, c), _cell(p, f, c)
    xa = xs.clone().requires_grad_(True)
    xb = xs[:, :, 1].contiguous().requires_grad_(True)
    view = xa[:, :, 1]
    assert not view.is_contiguous()
    out_a = cell_a(view, ei.cuda(), ew.cuda())
    out_b = cell_b(xb, ei.cuda(), ew.cuda())
    (out_a * gh).sum().backward()
    (out_b * gh).sum().backward()
    assert torch.equal(out_a, out_b) and torch.equal(xa.grad[:, :, 1], xb.grad)
    assert float(xa.grad[:, :, 0].abs().max()) == 0.0 and float(xa.grad[:, :, 2].abs().max()) == 0.0
    for (k, v), (_, w) in zip(cell_a.named_parameters(), cell_b.named_parameters()):
        assert torch.equal(v.grad, w.grad), k


# ---- recurrence ------------------------------------------------------------------------------------------------------------------------------

def test_three_step_recurrence_against_the_unrolled_restatement():
    n, c, f, t = 130, 256, 8, 3
    ei, ew = _graph(n)
    p = _params(c, f)
    gen = torch.Generator().manual_seed(19)
    xs, h0 = torch.rand(n, f, t, generator=gen), 0.5 * torch.randn(n, c, generator=gen)

    def run():
        cell = _cell(p, f, c)
        xl, hl = xs.cuda().requires_grad_(True), h0.cuda().requires_grad_(True)
        hh = hl
        for k in range(t):
            hh = cell(xl[:, :, k], ei.cuda(), ew.cuda(), hh)
        (hh ** 2).sum().backward()
        return hh.detach().cpu(), hl.grad.cpu(), xl.grad.cpu(), _grads(cell)

    got, again = run(), run()
    op = R.graph.prepare_gcn_operator(ei.cuda(), ew.cuda(), n)
    a = TM.dense_from_csr(op.rowptr, op.col, op.val, n)
    p64 = {k: v.double() for k, v in p.items()}
    last, dh0, dxs, grads = TM.unroll(p64, a, [xs[:, :, k].double() for k in range(t)], h0.double())
    _rows_held(got[0], last, CP.BAR["hidden"], "recurrence H")
    _rows_held(got[1], dh0, CP.BAR["dh_in"], "recurrence dH0")
    for k in range(t):
        _rows_held(got[2][:, :, k], dxs[k], CP.BAR["dh_in"], f"recurrence dX[:, :, {k}]")
    GB.assert_grads_to_scale(got[3], grads, what="recurrence")
    assert all(torch.equal(u, v) for u, v in zip(got[:3], again[:3]))
    assert all(torch.equal(got[3][k], again[3][k]) for k in got[3])


# ---- the inner modules of the whole models ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regional", [False, True], ids=["TemporalGCN", "RegionalTemporalGCN"])
def test_inner_module_is_the_models_hidden(tpims, regional):
    n = tpims["node_data"].shape[0]
    x = tpims["node_data"][:, :, :6].contiguous().cuda()
    ei = tpims["edge_index"].cuda()
    torch.manual_seed(5)
    if regional:
        ri, rw = region_lists(tpims)
        args = (ei, *[t.cuda() for t in ri], *[t.cuda() for t in rw])
        make = lambda: R.RegionalTemporalGCN(8, n, 6, 1)                      # noqa: E731
    else:
        args = (ei, tpims["edge_attr"].cuda())
        make = lambda: R.TemporalGCN(node_features=8, periods=6, output_dim=1)  # noqa: E731
    whole = make().cuda()
    inner = make().cuda()
    inner.load_state_dict(whole.state_dict())
    _pred, hidden = whole(x, *args)
    got = inner.tgnn(x, *args)
    assert torch.equal(got, hidden)
    with torch.no_grad():
        assert torch.equal(inner.tgnn(x, *args), hidden)
    gh = torch.randn(hidden.shape, generator=torch.Generator().manual_seed(23)).cuda()
    (hidden * gh).sum().backward()                                           # dpred = 0, dhidden = gh
    (got * gh).sum().backward()
    seen = 0
    for (k, v), (_, w) in zip(whole.tgnn.named_parameters(), inner.tgnn.named_parameters()):
        assert (v.grad is None) == (w.grad is None), k
        if v.grad is not None:
            assert torch.equal(v.grad, w.grad), k
            seen += 1
    assert seen >= 16
    assert all(v.grad is None for k, v in inner.named_parameters() if not k.startswith("tgnn."))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------

def test_documented_refusals():
    lib = R.load_library()
    n, c, f = 10, 16, 8
    ei, _ = _graph(n)
    cell = _cell(_params(c, f), f, c)
    x, h = torch.rand(n, f).cuda(), torch.rand(n, c).cuda()
    prev = lib.regt_set_gemm_mode(2)
    try:
        with pytest.raises(R.RegtError, match="bf16"):
            cell(x, ei.cuda(), None, h)
    finally:
        lib.regt_set_gemm_mode(prev)
    with pytest.raises(NotImplementedError, match="GATTemporal"):
        R.nn.TGCN(f, c, baseblock="gat").cuda()(x, ei.cuda(), None, h)
    with pytest.raises(R.RegtError):
        cell(x.cpu(), ei, None, h.cpu())
    assert tuple(cell(x, ei.cuda(), None, h).shape) == (n, c)
