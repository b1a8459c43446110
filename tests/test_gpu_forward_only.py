"""Forward-only calls on the GPU (REGT_DIMS_FORWARD_ONLY; functional.set_forward_only_in_no_grad): the same pred / hidden bit for
bit as the training forward in every form, nothing written outside the forward-only workspace, the refusals, the dispatch in the
modules and the evaluation loops."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import region_lists
from oracle import model as M
from test_gpu_model import _synthetic
from window_math import POISON

pytestmark = pytest.mark.gpu

ARITHS = ("fp32", "bf16x3", "bf16")
# (nodes, edges, regions, F, T, O) from tests/test_gpu_bf16.py::SHAPES: the two shapes of the fused forward (F = 32 / 64), nodes of 48
# rows across the 64-row halves, one period
SHAPES = [(1500, 15000, 8, 32, 12, 1), (2048, 20000, 64, 64, 12, 1), (400, 3000, 2, 32, 48, 1), (9000, 45000, 3, 32, 1, 1)]


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd as R_
    R_.load_library()
    return R_


@pytest.fixture()
def switch(R):
    """functional.set_forward_only_in_no_grad, restored afterwards."""
    F = R.functional
    prev = F.set_forward_only_in_no_grad(True)
    yield F.set_forward_only_in_no_grad
    F.set_forward_only_in_no_grad(prev)


def _cuda(ts):
    return [t.cuda() for t in ts]


_SYN = {}


def _regional(R, shape, arith):
    """Module + prepared graph + input of a synthetic regional problem (generated once per shape)."""
    n, e, regions, f, t, o = shape
    if shape not in _SYN:
        ei, ri, rw, x = _synthetic(n, e, regions, f, t, seed=n)
        _SYN[shape] = (ei, ri, rw, x, M.init_params("RegionalTemporalGCN", f, t, o, num_nodes=n, num_regions=regions, seed=3))
    ei, ri, rw, x, p = _SYN[shape]
    mod = R.RegionalTemporalGCN(node_features=f, num_nodes=n, periods=t, output_dim=o, num_regions=regions)
    mod.load_state_dict(p, strict=True)
    mod = mod.cuda()
    mod.arithmetic = arith
    return mod, mod.prepare_graph(ei.cuda(), _cuda(ri), _cuda(rw)), x.cuda()


def _both(switch, run):
    """``run()`` under no_grad with the training forward, then forward-only twice; the outputs must be the same bits."""
    with torch.no_grad():
        switch(False)
        a = run()
        switch(True)
        b = run()
        again = run()
    for u, v, w in zip(a, b, again):
        assert torch.isfinite(u).all()
        assert torch.equal(u, v)
        assert torch.equal(v, w)           # the forward-only call is deterministic (every T here is <= 64)
    return b


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_r%d_f%d_t%d" % (s[0], s[2], s[3], s[4]))
def test_bit_equal_on_synthetic_regional_graphs(R, switch, shape, arith):
    mod, graph, x = _regional(R, shape, arith)
    _both(switch, lambda: mod.forward_prepared(x, graph))


@pytest.mark.parametrize("form", ["rows", "tile64", "no_bf16_rows"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=["f32", "f64"])
def test_bit_equal_in_every_bf16_form(R, switch, shape, form):
    """The two fused shapes through the row-owning kernel, the 64-row kernel and the three-launch path on fp32 rows."""
    lib = R.load_library()
    mod, graph, x = _regional(R, shape, "bf16")
    prev = lib.regt_set_option(b"fused_rows", 0 if form == "tile64" else 1)
    try:
        if form == "no_bf16_rows":
            mod.call_flags = R._lib.DIMS_NO_BF16_ROWS
        _both(switch, lambda: mod.forward_prepared(x, graph))
    finally:
        lib.regt_set_option(b"fused_rows", prev)


@pytest.mark.parametrize("arith", ARITHS)
def test_bit_equal_on_the_tpims_fixture(R, switch, tpims, arith):
    """N = 104, F = 8, T = 6, five regions: the small-tile kernels."""
    ri, rw = region_lists(tpims)
    n = tpims["node_data"].shape[0]
    mod = R.RegionalTemporalGCN(8, n, 6, 1)
    mod.load_state_dict(M.init_params("RegionalTemporalGCN", 8, 6, 1, num_nodes=n, seed=0))
    mod = mod.cuda()
    mod.arithmetic = arith
    x = tpims["node_data"][:, :, :6].contiguous().cuda()
    _both(switch, lambda: mod(x, tpims["edge_index"].cuda(), *_cuda(ri), *_cuda(rw)))


@pytest.mark.parametrize("arith", ARITHS)
def test_bit_equal_temporal_gcn(R, switch, tpims, arith):
    """TemporalGCN: the collapsed gate form (FMT_TCOLLAPSE) in fp32 / bf16x3, the uncollapsed one in bf16."""
    n, f, t = 3000, 32, 12
    ei, _ri, _rw, x = _synthetic(n, 20000, 2, f, t, seed=5)
    w = torch.rand(ei.shape[1], generator=torch.Generator().manual_seed(2)) * 100 + 1
    mod = R.TemporalGCN(node_features=f, periods=t, output_dim=2)
    mod.load_state_dict(M.init_params("TemporalGCN", f, t, 2, seed=1), strict=True)
    mod = mod.cuda()
    mod.arithmetic = arith
    _both(switch, lambda: mod(x=x.cuda(), edge_index=ei.cuda(), edge_attr=w.cuda()))


@pytest.mark.parametrize("arith", ARITHS)
def test_bit_equal_overlapping_random_decomposition(R, switch, arith):
    n, e, regions, f, t, o = 3000, 30000, 3, 32, 12, 2
    g = torch.Generator().manual_seed(n)
    src, dst = torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)
    ei = torch.stack([src[src != dst], dst[src != dst]])
    w = torch.rand(ei.shape[1], generator=g) * 2925 + 75
    part = torch.randint(0, regions, (ei.shape[1],), generator=g)
    ri = [ei[:, part == r].contiguous() for r in range(regions)]
    rw = [w[part == r].contiguous() for r in range(regions)]
    x = torch.rand(n, f, t, generator=g).cuda()
    mod = R.RegionalTemporalGCN(f, n, t, o, num_regions=regions)
    mod.load_state_dict(M.init_params("RegionalTemporalGCN", f, t, o, num_nodes=n, num_regions=regions, seed=4))
    mod = mod.cuda()
    mod.arithmetic = arith
    graph = mod.prepare_graph(ei.cuda(), _cuda(ri), _cuda(rw))
    assert graph.overlap
    _both(switch, lambda: mod.forward_prepared(x, graph))


def test_bit_equal_conv_stacked_cell_path(R, switch, tpims):
    """ConvStackedTemporalGCN: regt_cell_forward on a caller-computed hidden input."""
    mod = R.ConvStackedTemporalGCN(8, 6, 1).cuda()
    x = tpims["node_data"][:, :, :6].contiguous().cuda()
    ei, ea = tpims["edge_index"].cuda(), tpims["edge_attr"].cuda()
    _both(switch, lambda: mod(x, ei, ea))
    # with grad enabled the parameters ask for a gradient: the training path, whose backward runs
    pred, _ = mod(x, ei, ea)
    pred.sum().backward()
    assert sum(q.grad is not None for q in mod.parameters()) > 10


@pytest.mark.parametrize("bf16_rows", [False, True], ids=["packed_fp32", "packed_bf16"])
def test_bit_equal_packed_entry_points(R, switch, bf16_rows):
    """regt_forward_packed / regt_forward_packed_bf16 as a one-shard problem (x_rows = N: no halo rows)."""
    shape = SHAPES[1]
    mod, graph, x = _regional(R, shape, "bf16" if bf16_rows else "fp32")
    n, f, t = shape[0], shape[3], shape[4]
    if bf16_rows:
        xp = R.ops.pack_x_bf16_into(x, torch.empty(n, t, f, dtype=torch.bfloat16, device="cuda"))
    else:
        xp = R.ops.pack_x(x)
    out = _both(switch, lambda: mod.forward_packed(xp, graph))
    with torch.no_grad():
        want = mod.forward_prepared(x, graph)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


_SHARDS = {}


def _shard(R, world):
    """Rank 0 of ``world`` region shards of one 2048-node graph (two regions per rank, F = 64, T = 12): own rows + halo rows."""
    if world not in _SHARDS:
        n, reg_per = 2048, 2
        g = R.data.synthetic_regional_graph(n, 30000, reg_per * world, seed=world, p_intra=0.3)
        bounds = np.asarray(g.region_bounds[::reg_per], dtype=np.int64)
        owner = [r // reg_per for r in range(reg_per * world)]
        sh = R.dist.build_shard(g.edge_index, g.region_index, g.region_attr, n, bounds, owner, 0, world, "cuda", method="global")
        x = torch.rand(sh.topo.x_rows, 12, 64, generator=torch.Generator().manual_seed(world))
        _SHARDS[world] = (sh, x.cuda(), M.init_params("RegionalTemporalGCN", 64, 12, 1, num_nodes=n, num_regions=reg_per * world, seed=5))
    return _SHARDS[world]


@pytest.mark.parametrize("world,rows", [(2, "fp32"), (4, "fp32"), (2, "bf16"), (4, "bf16")],
                         ids=["halo_le_2n_fp32_rows", "halo_gt_2n_fp32_rows", "halo_le_2n_bf16_rows", "halo_gt_2n_bf16_rows"])
def test_bit_equal_packed_with_halo_rows(R, switch, monkeypatch, world, rows):
    """A region shard in bf16 arithmetic whose packed input carries halo rows.  fp32 rows take the fused form up to x_rows = 2 N
    (the forward keeps a bf16 copy of all x_rows rows) and the three-launch form beyond, with or without the flag; bf16 rows are
    read in place.  The block taken is exactly what the packed sizing function returns, and the library accepts it."""
    sh, x, p = _shard(R, world)
    n, x_rows = sh.topo.n_local, sh.topo.x_rows
    assert (n < x_rows <= 2 * n) if world == 2 else (x_rows > 2 * n)
    regions = 2 * world
    mod = R.RegionalTemporalGCN(64, 2048, 12, 1, num_regions=regions)
    mod.load_state_dict(p, strict=True)
    mod = mod.cuda()
    mod.arithmetic = "bf16"
    xp = x.to(torch.bfloat16) if rows == "bf16" else x
    spy = _PoolSpy(R.functional, monkeypatch)
    _both(switch, lambda: mod.forward_packed(xp, sh.graph))
    lib = R.load_library()
    dims = R._lib.Dims(n, 12, 64, 256, regions, 1, 128, 1, 0.01, R._lib.ARITH_BF16, R._lib.DIMS_FORWARD_ONLY)
    gs = R.functional._graph_struct(sh.graph, 12)
    train = lib.regt_workspace_bytes(C.byref(dims), gs.n_chunks, gs.overlap)
    base = lib.regt_forward_only_workspace_bytes(C.byref(dims), C.byref(gs))
    want = lib.regt_forward_only_packed_workspace_bytes(C.byref(dims), C.byref(gs), x_rows, 1 if rows == "bf16" else 0)
    assert spy.sizes == [train, want, want] and 0 < want < train
    assert lib.regt_forward_only_packed_workspace_bytes(C.byref(dims), C.byref(gs), n, 0) == base
    m = n * 12
    if rows == "bf16":
        assert want == base                                   # the caller's rows are read in place
    elif world == 2:
        assert 0 <= want - base - (x_rows - n) * 12 * 64 * 2 < 512     # fused: the bf16 copy of the halo rows (+ rounding to 256 B)
    else:
        assert want >= base + m * 256 * 2                     # beyond 2 N the three-launch form: h, [Z | R], q


# ---- the C ABI directly -------------------------------------------------------------------------------------------------------------
def _abi_problem(R, shape, arith):
    """dims / graph / params structs of a synthetic problem, the training and the forward-only workspace size."""
    from regtgcn_amd import _lib
    from regtgcn_amd.functional import _fill, _graph_struct, param_names
    lib = R.load_library()
    mod, graph, x = _regional(R, shape, arith)
    n, _e, regions, f, t, o = shape
    named = dict(mod.named_parameters())
    tens = {k: named[k].detach() for k in param_names(True)}
    dims = _lib.Dims(n, t, f, 256, regions, o, 128, 1, 0.01, _lib.arith_code(arith), _lib.DIMS_FORWARD_ONLY)
    gs = _graph_struct(graph, t)
    ps = _fill(_lib.Params(), tens, True)
    train = lib.regt_workspace_bytes(C.byref(dims), gs.n_chunks, gs.overlap)
    fwd = lib.regt_forward_only_workspace_bytes(C.byref(dims), C.byref(gs))
    assert 0 < fwd < train
    return lib, _lib, (mod, graph, x, tens), dims, gs, ps, train, fwd


def _poisoned(nwords):
    return torch.full((nwords,), POISON, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("shape,arith", [(SHAPES[0], "fp32"), (SHAPES[1], "bf16"), (SHAPES[0], "bf16")], ids=["fp32", "bf16_fused_f64", "bf16_fused_f32"])
def test_nothing_outside_the_declared_workspace_is_touched(R, shape, arith):
    lib, _lib, keep, dims, gs, ps, train, fwd = _abi_problem(R, shape, arith)
    x = keep[2]
    n, o = shape[0], shape[5]
    ws = _poisoned(train // 4)                     # training size: a store through an old offset lands inside the allocation
    pred, hidden = _poisoned(n * o), _poisoned(n * 256)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.regt_forward(C.byref(dims), C.byref(gs), C.byref(ps), _lib.ptr(x), _lib.ptr(pred), _lib.ptr(hidden), _lib.ptr(ws),
                                fwd, st), "regt_forward")
    torch.cuda.synchronize()
    assert fwd % 4 == 0
    assert bool((ws[fwd // 4:] == POISON).all()), "a word behind the forward-only workspace changed"
    assert not bool((pred == POISON).any()) and not bool((hidden == POISON).any())
    # ... and these are the values of the training forward
    dims.flags = 0
    pred2, hidden2 = torch.empty_like(pred), torch.empty_like(hidden)
    _lib.check(lib.regt_forward(C.byref(dims), C.byref(gs), C.byref(ps), _lib.ptr(x), _lib.ptr(pred2), _lib.ptr(hidden2), _lib.ptr(ws),
                                train, st), "regt_forward")
    assert torch.equal(pred, pred2) and torch.equal(hidden, hidden2)


def test_refusals_are_host_side(R):
    from regtgcn_amd.functional import _fill
    lib, _lib, keep, dims, gs, ps, train, fwd = _abi_problem(R, SHAPES[0], "fp32")
    x, tens = keep[2], keep[3]
    n = SHAPES[0][0]
    ws = torch.empty(train, dtype=torch.uint8, device="cuda")
    pred, hidden = torch.empty(n, 1, device="cuda"), torch.empty(n, 256, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    fwd_call = lambda nbytes: lib.regt_forward(C.byref(dims), C.byref(gs), C.byref(ps), _lib.ptr(x), _lib.ptr(pred), _lib.ptr(hidden),
                                               _lib.ptr(ws), nbytes, st)
    # one byte short: refused, nothing launched (pred keeps its poison)
    pred.view(torch.int32).fill_(POISON)
    assert fwd_call(fwd - 1) != 0
    msg = lib.regt_last_error().decode()
    assert "FORWARD_ONLY" in msg and str(fwd) in msg
    torch.cuda.synchronize()
    assert bool((pred.view(torch.int32) == POISON).all())
    # a backward on a forward-only workspace: refused with the cause, whatever the size passed
    assert fwd_call(fwd) == 0
    grads = {k: torch.full_like(v, float("nan")) for k, v in tens.items()}
    gr = _fill(_lib.Grads(), grads, True)
    dpred = torch.ones(n, 1, device="cuda")
    dims.flags = 0
    rc = lib.regt_backward(C.byref(dims), C.byref(gs), C.byref(ps), C.byref(gr), _lib.ptr(dpred), None, _lib.ptr(hidden), None,
                           _lib.ptr(ws), train, st)
    assert rc != 0 and "FORWARD_ONLY" in lib.regt_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(g).all()) for g in grads.values())          # nothing was written
    # a training forward on the same workspace makes it usable again
    assert lib.regt_forward(C.byref(dims), C.byref(gs), C.byref(ps), _lib.ptr(x), _lib.ptr(pred), _lib.ptr(hidden), _lib.ptr(ws), train, st) == 0
    assert lib.regt_backward(C.byref(dims), C.byref(gs), C.byref(ps), C.byref(gr), _lib.ptr(dpred), None, _lib.ptr(hidden), None,
                             _lib.ptr(ws), train, st) == 0


def test_cell_backward_refuses_a_forward_only_workspace(R, tpims):
    from regtgcn_amd import _lib
    from regtgcn_amd.functional import PARAM_NAMES_CELL, _fill, _gcn_graph_struct
    from regtgcn_amd.graph import prepare_gcn_operator
    lib = R.load_library()
    mod = R.ConvStackedTemporalGCN(8, 6, 1).cuda()
    n, t, c = tpims["node_data"].shape[0], 6, 512
    x = tpims["node_data"][:, :, :t].contiguous().cuda()
    op = prepare_gcn_operator(tpims["edge_index"].cuda(), tpims["edge_attr"].cuda(), n)
    named = dict(mod.named_parameters())
    tens = {k: named[k].detach() for k in PARAM_NAMES_CELL}
    h_in = torch.rand(n * t, c, device="cuda")
    dims = _lib.Dims(n, t, 8, c, 1, 1, 128, 0, 0.0, 0, _lib.DIMS_FORWARD_ONLY)
    gs, ps = _gcn_graph_struct(op), _fill(_lib.Params(), tens, False)
    train = lib.regt_workspace_bytes(C.byref(dims), 0, 0)
    fwd = lib.regt_forward_only_workspace_bytes(C.byref(dims), C.byref(gs))
    assert 0 < fwd < train
    ws = torch.empty(train, dtype=torch.uint8, device="cuda")
    pred, hidden = torch.empty(n, 1, device="cuda"), torch.empty(n, c, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    call = lambda nbytes: lib.regt_cell_forward(C.byref(dims), C.byref(gs), C.byref(ps), _lib.ptr(x), _lib.ptr(h_in), _lib.ptr(pred),
                                                _lib.ptr(hidden), _lib.ptr(ws), nbytes, st)
    assert call(fwd - 1) != 0 and "FORWARD_ONLY" in lib.regt_last_error().decode()
    assert call(fwd) == 0
    grads = {k: torch.empty_like(v) for k, v in tens.items()}
    gr = _fill(_lib.Grads(), grads, False)
    dh_in, dpred = torch.empty_like(h_in), torch.ones(n, 1, device="cuda")
    dims.flags = 0
    rc = lib.regt_cell_backward(C.byref(dims), C.byref(gs), C.byref(ps), C.byref(gr), _lib.ptr(dpred), None, _lib.ptr(hidden),
                                _lib.ptr(h_in), _lib.ptr(dh_in), _lib.ptr(ws), train, st)
    assert rc != 0 and "FORWARD_ONLY" in lib.regt_last_error().decode()


# ---- dispatch in the modules -------------------------------------------------------------------------------------------------------
class _PoolSpy:
    """Records what RegTGCNFunction / regt_run take from the workspace pool."""

    def __init__(self, F, monkeypatch):
        self.sizes, self.pool = [], F._POOL
        orig = F._POOL.acquire

        def acquire(nbytes, device):
            self.sizes.append(nbytes)
            return orig(nbytes, device)
        monkeypatch.setattr(F._POOL, "acquire", acquire)

    def free_blocks(self, nbytes):
        return sum(len(v) for k, v in self.pool._free.items() if k[2] == nbytes)


@pytest.mark.parametrize("arith", ["fp32", "bf16"])
def test_dispatch_by_grad_mode_and_requires_grad(R, switch, monkeypatch, arith):
    F = R.functional
    shape = SHAPES[0]
    mod, graph, x = _regional(R, shape, arith)
    lib = R.load_library()
    dims = R._lib.Dims(shape[0], shape[4], shape[3], 256, shape[2], shape[5], 128, 1, 0.01, R._lib.arith_code(arith), 0)
    gs = F._graph_struct(graph, shape[4])
    train = lib.regt_workspace_bytes(C.byref(dims), gs.n_chunks, gs.overlap)
    fwd = lib.regt_forward_only_workspace_bytes(C.byref(dims), C.byref(gs))
    spy = _PoolSpy(F, monkeypatch)
    # no_grad: the forward-only block, back in the pool when the call returns
    with torch.no_grad():
        pred_e, hid_e = mod.forward_prepared(x, graph)
    assert spy.sizes == [fwd] and spy.free_blocks(fwd) >= 1
    assert pred_e.grad_fn is None and not pred_e.requires_grad
    # grad enabled: the training block, and the same gradients as with the switch off
    grads = []
    for flag in (True, False):
        switch(flag)
        spy.sizes.clear()
        mod.zero_grad(set_to_none=True)
        pred, hidden = mod.forward_prepared(x, graph)
        assert spy.sizes == [train]
        assert torch.equal(pred.detach(), pred_e) and torch.equal(hidden.detach(), hid_e)
        (pred.square().mean() + hidden.mean()).backward()
        grads.append({k: q.grad.clone() for k, q in mod.named_parameters() if q.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 10
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])
    # frozen parameters: forward-only with grad mode on
    switch(True)
    mod.requires_grad_(False)
    spy.sizes.clear()
    pred_f, _ = mod.forward_prepared(x, graph)
    assert spy.sizes == [fwd] and torch.equal(pred_f, pred_e)
    # ... and the switch turns it off
    switch(False)
    spy.sizes.clear()
    with torch.no_grad():
        mod.forward_prepared(x, graph)
    assert spy.sizes == [train]


def test_evaluation_loops_return_the_same_floats(R, switch, tpims):
    """train.evaluate / evaluate_batched (B = 64) and evaluate.predict_metrics / _batched on the TPIMS fixture, switch on and off."""
    ri, rw = region_lists(tpims)
    n, t_in, t_out = tpims["node_data"].shape[0], 6, 1
    mod = R.RegionalTemporalGCN(8, n, t_in, t_out)
    mod.load_state_dict(M.init_params("RegionalTemporalGCN", 8, t_in, t_out, num_nodes=n, seed=0))
    mod = mod.cuda().eval()
    ei, ric, rwc = tpims["edge_index"].cuda(), _cuda(ri), _cuda(rw)
    graphs = R.train.BatchedGraphs(lambda b: mod.prepare_graph(ei, ric, rwc, copies=b))
    nd = tpims["node_data"].cuda()
    steps = min(nd.shape[2] - t_in - t_out, 130)
    xs = [nd[:, :, s:s + t_in].contiguous() for s in range(steps)]
    ys = [nd[:, -1, s + t_in:s + t_in + t_out].contiguous() for s in range(steps)]
    store = R.train.WindowStore(xs, ys)

    def run():
        return (R.train.evaluate(mod, xs, ys, graphs.get(1)), R.train.evaluate_batched(mod, store, graphs, 64),
                R.evaluate.predict_metrics(mod, xs, ys, graphs.get(1)), R.evaluate.predict_metrics_batched(mod, store, graphs, 64))

    switch(False)
    want = run()
    switch(True)
    got = run()
    assert got == want
    assert all(np.isfinite(v) for tup in got for v in tup)
