"""The whole-model input gradient on the device (functional.RegTGCNFunction.backward -> regt_input_gradient; csrc/model_dx.hip,
csrc/spmm_dual_t.hip): ``x.grad`` of the module call against float64 autograd through the oracle, per row of (N, T F),
for the cases of tests/input_grad_math.py; the inner modules (the NO_HEAD route); bit identity of everything else with and without
``x.requires_grad``; run-to-run bit identity; a poisoned, offset dx buffer; a learnable encoder in front of the model; the refusals.

Bar: input_grad_math.bar() -- the worst row ratio of the fp32 restatement of the same formulas over these cases is 1.08e-6, x 4 = 4.3e-6 is
inside cell_probe.BAR["dh_in"] = 2 ** -14, so that bar holds and nothing is added (tests/test_input_grad_cpu.py derives it).  A row that
is 0 in float64 must be 0.  The measured ratios are in profiles/input_grad.txt."""
import ctypes

import pytest
import torch

import grad_bars as GB
import input_grad_math as IG
import regtgcn_amd as R
from regtgcn_amd import _lib, ops
from regtgcn_amd import functional as Fn

pytestmark = pytest.mark.gpu
ARITH = {0: "fp32", 1: "bf16x3"}


def _cuda(ts):
    return [None if t is None else t.cuda() for t in ts]


def _module(name):
    return IG.device_module(R, name)


def _prepared(name):
    return IG.device_graph(R, name)


def _Collapse(name):
    return IG.collapse_option(R, name)


def _run(name, x_grad=True):
    return IG.run_hip(R, name, x_grad)


_RUNS = {}


def _first_run(name):
    if name not in _RUNS:
        _RUNS[name] = _run(name)
    return _RUNS[name]


# ---- rows of dx against float64 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(IG.CASES))
def test_rows_of_dx_against_float64_autograd_of_the_oracle(name):
    ref = IG.reference(name)
    got = _first_run(name)
    assert got["dx"] is not None, "x.grad is None: the model's backward returned no input gradient"
    c = IG.CASES[name]
    assert tuple(got["dx"].shape) == (c["n"] * c["copies"], c["f"], c["t"])
    IG.held(got["dx"], ref["dx"], name + " dx")
    GB.assert_grads_to_scale({k: v for k, v in got["grads"].items()}, ref["grads"], what=name, num_regions=c["r"] if c["model"] == "regional" else None)


BIT_CASES = ["regt-N43-T3-F7-C48-shuffled", "regt-N43-T3-F32-C256-sorted", "regt-N43-T3-F8-C48-sorted-2copies", "tgcn-N130-T1-F8-C48-collapsed",
             "tgcn-N43-T3-F36-C16-uncollapsed", "tgcn-N43-T3-F64-C256-collapsed-bf16x3"]


@pytest.mark.parametrize("name", BIT_CASES)
def test_everything_else_keeps_its_bits_and_dx_repeats(name):
    assert IG.CASES[name]["t"] <= 64
    with_dx, again, without = _first_run(name), _run(name), _run(name, x_grad=False)
    assert without["dx"] is None
    assert torch.equal(with_dx["dx"], again["dx"])
    for other in (again, without):
        assert torch.equal(with_dx["pred"], other["pred"]) and torch.equal(with_dx["hidden"], other["hidden"])
        for k, v in with_dx["grads"].items():
            assert (v is None) == (other["grads"][k] is None), k
            if v is not None:
                assert torch.equal(v, other["grads"][k]), k


def test_nothing_is_launched_or_built_when_x_asks_for_no_gradient(monkeypatch):
    """ops.input_gradient is the bridge's one way to regt_input_gradient (both launches and the scratch allocation) and
    PreparedGraph.transposed_merged the one builder of the transposed operator: without x.requires_grad neither is touched, and the
    caching allocator's peak stays below the run that does ask by at least the scratch."""
    name = "regt-N43-T3-F32-C256-sorted"
    c = IG.CASES[name]
    ref = IG.reference(name)
    ei, _ew, ri, rw = IG.graph(name)
    graph = R.prepare_graph(ei.cuda(), None, _cuda(ri), _cuda(rw), c["n"], c["copies"])       # a graph of its own: no cache entry yet
    calls = []
    real = ops.input_gradient
    monkeypatch.setattr(ops, "input_gradient", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    mod = _module(name)
    g1, g2 = ref["g1"].cuda(), ref["g2"].cuda()

    def run(x_grad):
        x = ref["x"].cuda().requires_grad_(x_grad)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        pred, hidden = mod.forward_prepared(x, graph)
        ((pred * g1).sum() + (hidden * g2).sum()).backward()
        torch.cuda.synchronize()
        return x.grad, torch.cuda.max_memory_allocated() - base

    run(False)                                                    # (warm-up: the workspace pool and the call plan exist afterwards)
    assert not calls and "_transposed_merged" not in graph.__dict__
    grad, peak_without = run(False)
    assert grad is None and not calls and "_transposed_merged" not in graph.__dict__
    grad, _ = run(True)                                           # (builds the transposed operator)
    assert grad is not None and len(calls) == 1 and graph.__dict__["_transposed_merged"] is not None
    grad, peak_with = run(True)
    assert len(calls) == 2
    n, f, t = ref["x"].shape
    assert peak_with - peak_without >= 3 * n * f * t * 4, (peak_with, peak_without)      # at least the three (M, F) scratch arrays


# ---- hidden alone through the inner modules (REGT_DIMS_NO_HEAD) ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["regt-N43-T3-F7-C48-shuffled", "tgcn-N43-T3-F36-C16-uncollapsed", "tgcn-N130-T1-F8-C48-collapsed"])
def test_inner_module_hidden_alone(name):
    c = IG.CASES[name]
    regional = c["model"] == "regional"
    ref = IG.reference(name)
    ei, ew, ri, rw = IG.graph(name)
    mod = _module(name)
    mod.tgnn.arithmetic = ARITH[c["mode"]]
    x = ref["x"].cuda().requires_grad_(True)
    with _Collapse(name):
        hidden = mod.tgnn(x, ei.cuda(), *_cuda(ri), *_cuda(rw)) if regional else mod.tgnn(x, ei.cuda(), ew.cuda())
        (hidden * ref["g2"].cuda()).sum().backward()
    assert x.grad is not None
    p64 = {k: v.double() for k, v in ref["p"].items()}
    x64 = ref["x"].double().requires_grad_(True)
    _pred, hid64 = IG.oracle(name, p64, x64, regional)
    (hid64 * ref["g2"].double()).sum().backward()
    IG.held(x.grad.cpu(), x64.grad, name + " inner dx")
    # the whole model's call gives the same through both outputs when pred carries no gradient
    x2 = ref["x"].cuda().requires_grad_(True)
    with _Collapse(name):
        _p, hid2 = mod.forward_prepared(x2, _prepared(name))
        (hid2 * ref["g2"].cuda()).sum().backward()
    assert torch.equal(hid2, hidden) and torch.equal(x2.grad, x.grad)


# ---- a poisoned, offset buffer ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["regt-N43-T3-F32-C256-sorted", "tgcn-N9-T150-F32-C16-collapsed", "regt-N130-T1-F64-C48-sorted"])
def test_dx_into_a_poisoned_offset_buffer(name):
    c = IG.CASES[name]
    regional = c["model"] == "regional"
    ref = IG.reference(name)
    lib = R.load_library()
    mod = _module(name)
    graph = _prepared(name)
    params = [p.detach() for p in mod._params_in_order()]
    x = ref["x"].cuda()
    with _Collapse(name):
        pred, hidden, st = Fn._regt_forward_call(x, graph, regional, 0.01, (False, _lib.arith_code(ARITH[c["mode"]]), 0), params, False)
        grads = {k: torch.empty_like(p) for k, p in zip(st.names, params)}
        gr = Fn._fill(_lib.Grads(), grads, regional)
        g1, g2 = ref["g1"].cuda().contiguous(), ref["g2"].cuda().contiguous()
        _lib.check(lib.regt_backward(ctypes.byref(st.dims), ctypes.byref(st.gs), ctypes.byref(st.ps), ctypes.byref(gr), _lib.ptr(g1), _lib.ptr(g2),
                                     _lib.ptr(hidden), None, _lib.ptr(st.handle.ws), st.wsb, Fn._stream()), "regt_backward")
        n, f, t = x.shape
        buf = torch.full((n * f * t + 96,), float("nan"), device="cuda")
        dx = buf[32:32 + n * f * t].view(n, f, t)
        assert dx.data_ptr() % 16 == 0 and dx.data_ptr() != buf.data_ptr()
        ws_before = st.handle.ws.clone()
        ops.input_gradient(st.dims, st.gs, st.ps, graph.transposed_merged, dx, st.handle.ws)
        ops.input_gradient(st.dims, st.gs, st.ps, graph.transposed_merged, dx, st.handle.ws)      # reads the workspace only: repeatable
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:32]).all()) and bool(torch.isnan(buf[32 + n * f * t:]).all())
    assert torch.equal(st.handle.ws, ws_before), "regt_input_gradient wrote into the step's workspace"
    if t > 64:      # the forward's sum over periods is not ordered beyond 64 periods (check_dims): another run's bits differ, the bar holds
        IG.held(dx.cpu(), ref["dx"], name + " dx in the offset buffer")
        return
    assert torch.equal(dx.cpu(), _first_run(name)["dx"])
    for k, v in zip(st.names, mod._params_in_order()):
        want = _first_run(name)["grads"][k]
        assert want is None or torch.equal(grads[k].cpu(), want), k


# ---- end to end: a learnable encoder in front of the model ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["regt-N43-T3-F8-C48-sorted-2copies", "tgcn-N43-T3-F36-C16-uncollapsed"])
def test_learnable_encoder_receives_the_oracles_gradient(name):
    c = IG.CASES[name]
    regional = c["model"] == "regional"
    ref = IG.reference(name)
    n, f, t = ref["x"].shape
    f_in = 5
    gen = torch.Generator().manual_seed(31)
    raw = torch.rand(n, f_in, t, generator=gen)
    enc = torch.nn.Linear(f_in, f)
    with torch.no_grad():
        enc.weight.copy_(torch.rand(f, f_in, generator=gen) - 0.3)
        enc.bias.copy_(torch.rand(f, generator=gen))
    w64, b64 = enc.weight.detach().double().requires_grad_(True), enc.bias.detach().double().requires_grad_(True)
    x64 = (raw.double().permute(0, 2, 1) @ w64.t() + b64).permute(0, 2, 1)
    p64 = {k: v.double() for k, v in ref["p"].items()}
    pred64, hid64 = IG.oracle(name, p64, x64, regional)
    ((pred64 * ref["g1"].double()).sum() + (hid64 * ref["g2"].double()).sum()).backward()
    enc = enc.cuda()
    mod = _module(name)
    x = enc(raw.cuda().permute(0, 2, 1)).permute(0, 2, 1)
    with _Collapse(name):
        pred, hidden = mod.forward_prepared(x, _prepared(name))
        ((pred * ref["g1"].cuda()).sum() + (hidden * ref["g2"].cuda()).sum()).backward()
    assert enc.weight.grad is not None and enc.bias.grad is not None
    GB.assert_grads_to_scale({"encoder.weight": enc.weight.grad.cpu(), "encoder.bias": enc.bias.grad.cpu()},
                             {"encoder.weight": w64.grad, "encoder.bias": b64.grad}, what=name + " encoder")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------

def _loss_backward(mod, x, graph, ref, packed=False):
    pred, hidden = mod.forward_packed(x, graph) if packed else mod.forward_prepared(x, graph)
    ((pred * ref["g1"].cuda()).sum() + (hidden * ref["g2"].cuda()).sum()).backward()


def test_refused_forms_raise_instead_of_returning_none():
    name = "regt-N43-T3-F8-C48-sorted-2copies"
    ref = IG.reference(name)
    c = IG.CASES[name]
    graph = _prepared(name)
    # the bf16 arithmetic
    mod = _module(name)
    mod.arithmetic = "bf16"
    with pytest.raises(R.RegtError, match="bf16"):
        _loss_backward(mod, ref["x"].cuda().requires_grad_(True), graph, ref)
    _loss_backward(mod, ref["x"].cuda(), graph, ref)                       # ... which still trains when x asks for nothing
    # the packed (sharded) input
    mod = _module(name)
    xp = ref["x"].permute(0, 2, 1).contiguous().cuda().requires_grad_(True)
    with pytest.raises(R.RegtError, match="packed"):
        _loss_backward(mod, xp, graph, ref, packed=True)
    # overlapping regions: every node receives edges in both regional graphs
    ei, _ew, ri, rw = IG.graph(name)
    n = c["n"]
    p2 = IG.M.init_params("RegionalTemporalGCN", c["f"], c["t"], IG.OUT, num_nodes=n, num_regions=2, seed=5, hidden=c["c"])
    mod2 = R.RegionalTemporalGCN(node_features=c["f"], num_nodes=n, periods=c["t"], output_dim=IG.OUT, num_regions=2, hidden_channels=c["c"])
    mod2.load_state_dict(p2, strict=True)
    mod2 = mod2.cuda()
    over = R.prepare_graph(ei.cuda(), None, [ei.cuda(), ei.cuda()], [None, None], n)
    assert over.overlap and over.transposed_merged is None
    x1 = ref["x"][:n].cuda().requires_grad_(True)
    sub = {"g1": ref["g1"][:n], "g2": ref["g2"][:n]}
    with pytest.raises(R.RegtError, match="overlap"):
        _loss_backward(mod2, x1, over, sub)
    _loss_backward(mod2, ref["x"][:n].cuda(), over, sub)
    # a workspace whose last forward was forward-only
    lib = R.load_library()
    mod = _module(name)
    params = [p.detach() for p in mod._params_in_order()]
    x = ref["x"].cuda()
    pred, hidden, st = Fn._regt_forward_call(x, graph, True, 0.01, (False, _lib.ARITH_FP32, 0), params, False)
    d = st.dims
    fo = _lib.Dims(d.N, d.T, d.F, d.C, d.R, d.O, d.H1, d.regional, d.lrelu_slope, d.arith, int(d.flags) | _lib.DIMS_FORWARD_ONLY)
    _lib.check(lib.regt_forward(ctypes.byref(fo), ctypes.byref(st.gs), ctypes.byref(st.ps), _lib.ptr(x), _lib.ptr(pred), _lib.ptr(hidden),
                                _lib.ptr(st.handle.ws), st.wsb, Fn._stream()), "regt_forward")
    dx = torch.empty_like(x)
    with pytest.raises(R.RegtError, match="FORWARD_ONLY"):
        ops.input_gradient(st.dims, st.gs, st.ps, graph.transposed_merged, dx, st.handle.ws)
    torch.cuda.synchronize()
