"""Every parameter gradient of the whole backward pass against the FLOAT64 oracle, block by block, at a bar relative to the
block's own scale (grad_bars.py) -- the parity tests' atol = 1e-5 is 15 .. 70 % of the scale of the reset gate's, the
attention's and (at many regions) the Chebyshev lins.1 gradients, so a wrong term there passes them.

Both outputs feed the loss, mse(pred, y) + (hidden ** 2).mean(), so the dhidden path is held too.  The float64 oracle is the
slow half; it runs once per shape (module cache) and is shared by the arithmetics and switch settings.
tools/grad_scale_bars.py runs the same cases and writes the table REL was taken from."""
import os

import pytest
import torch

from conftest import GOLDEN, REGIONS, load_npz
from grad_bars import REL, assert_grads_to_scale
from oracle import model as M

pytestmark = pytest.mark.gpu


def _cast(obj, dtype):
    if isinstance(obj, torch.Tensor):
        return obj.to(dtype) if obj.is_floating_point() else obj
    if isinstance(obj, (list, tuple)):
        return [_cast(o, dtype) for o in obj]
    return obj


def _cuda(obj):
    if isinstance(obj, torch.Tensor):
        return obj.cuda()
    if isinstance(obj, (list, tuple)):
        return [_cuda(o) for o in obj]
    return obj


def _loss(pred, hidden, y):
    return torch.mean((pred - y) ** 2) + (hidden ** 2).mean()


class Case:
    """One model instance: fp32 parameters `p`, target `y`, the oracle's and the module's inputs `args` (tensors / lists of
    tensors; float ones are cast for the float64 run), `oracle(p, *args)` and `module(R)` + `call(mod, *args)` -> (pred, hidden)."""

    def __init__(self, p, y, args, oracle, module, call=None, num_regions=None):
        self.p, self.y, self.args, self.oracle, self.module, self.num_regions = p, y, args, oracle, module, num_regions
        self.call = call or (lambda mod, *a: mod(*a))

    def oracle_grads(self, dtype, loss=_loss):
        po = {k: v.detach().to(dtype).requires_grad_(True) for k, v in self.p.items()}
        pred, hidden = self.oracle(po, *_cast(self.args, dtype))
        loss(pred, hidden, self.y.to(dtype)).backward()
        return {k: v.grad for k, v in po.items()}

    def hip_grads(self, R):
        mod = self.module(R)
        mod.load_state_dict(self.p, strict=True)
        mod = mod.cuda()
        pred, hidden = self.call(mod, *_cuda(self.args))
        _loss(pred, hidden, self.y.cuda()).backward()
        torch.cuda.synchronize()
        return {k: (None if q.grad is None else q.grad.cpu()) for k, q in mod.named_parameters()}


def _regt(n, e, regions, f, t, o):
    """The synthetic regional graph, parameters and targets of test_regt_matches_oracle_on_synthetic_regional_graph."""
    from test_gpu_model import _synthetic
    ei, ri, rw, x = _synthetic(n, e, regions, f, t, seed=n)
    y = torch.rand(n, o, generator=torch.Generator().manual_seed(1))
    p = M.init_params("RegionalTemporalGCN", f, t, o, num_nodes=n, num_regions=regions, seed=3)
    return Case(p, y, (x, ei, ri, rw), M.regional_temporal_gcn,
                lambda R: R.RegionalTemporalGCN(node_features=f, num_nodes=n, periods=t, output_dim=o, num_regions=regions), num_regions=regions)


def _overlap(n, e, regions, f, t, o):
    """test_overlapping_random_decomposition_matches_oracle's graph: edges dealt to the regions at random (general layout)."""
    g = torch.Generator().manual_seed(n)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n, (e,), generator=g)
    keep = src != dst
    ei = torch.stack([src[keep], dst[keep]])
    w = torch.rand(ei.shape[1], generator=g) * 2925 + 75
    part = torch.randint(0, regions, (ei.shape[1],), generator=g)
    ri = [ei[:, part == r].contiguous() for r in range(regions)]
    rw = [w[part == r].contiguous() for r in range(regions)]
    x = torch.rand(n, f, t, generator=g)
    y = torch.rand(n, o, generator=g)
    p = M.init_params("RegionalTemporalGCN", f, t, o, num_nodes=n, num_regions=regions, seed=4)
    return Case(p, y, (x, ei, ri, rw), M.regional_temporal_gcn, lambda R: R.RegionalTemporalGCN(f, n, t, o, num_regions=regions), num_regions=regions)


def _ragged(n, f, t, o):
    """Regions of 1, 2, 3, 5, 8, 11, 40, 300 nodes in turn (embed_probe.ragged_blocks) with random directed edges inside each region
    and ordinary random parameters: a node without regional in-edges joins the region in front of it (graph.node_regions), so
    graph.region_chunks holds chunks of a single node, 64-row tiles hold three and more regions and some region ids own no row
    (tests/test_embed_probe_cpu.py checks that on the host, and that the fp32 oracle is within REL / 4 of float64 on every block)."""
    from embed_probe import ragged_blocks
    g = torch.Generator().manual_seed(n)
    blocks = ragged_blocks(n)
    ri, rw, start = [], [], 0
    for size in blocks:
        if size == 1:                                # no edge inside one node: a self loop (dropped by ChebConv) keeps the list non-empty
            ei = torch.tensor([[start], [start]])
        elif size <= 3:                              # every edge into the block's last node: it alone owns rows of this region
            ei = torch.stack([start + torch.arange(size - 1), torch.full((size - 1,), start + size - 1)])
        else:
            e = size
            src = start + torch.randint(0, size, (e,), generator=g)
            dst = start + (src - start + 1 + torch.randint(0, size - 1, (e,), generator=g)) % size
            ei = torch.stack([src, dst])
        ri.append(ei.contiguous())
        rw.append(torch.rand(ei.shape[1], generator=g) * 2925 + 75)
        start += size
    cross = torch.randint(0, n, (2, n // 2), generator=g)
    ei = torch.cat(ri + [cross[:, cross[0] != cross[1]]], dim=1).contiguous()
    x = torch.rand(n, f, t, generator=g)
    y = torch.rand(n, o, generator=g)
    regions = len(blocks)
    p = M.init_params("RegionalTemporalGCN", f, t, o, num_nodes=n, num_regions=regions, seed=6)
    return Case(p, y, (x, ei, ri, rw), M.regional_temporal_gcn,
                lambda R: R.RegionalTemporalGCN(node_features=f, num_nodes=n, periods=t, output_dim=o, num_regions=regions), num_regions=regions)


def _tgcn(n, e, f, t, o):
    from test_gpu_model import _synthetic
    ei, _ri, rw, x = _synthetic(n, e, 1, f, t, seed=n)               # one region: rw[0] weighs every edge of ei
    y = torch.rand(n, o, generator=torch.Generator().manual_seed(1))
    p = M.init_params("TemporalGCN", f, t, o, seed=3)
    return Case(p, y, (x, ei, rw[0]), M.temporal_gcn, lambda R: R.TemporalGCN(node_features=f, periods=t, output_dim=o))


def _zero_hidden(name, n, e, f, t, o):
    from test_gpu_zero_hidden import _graph
    ei = _graph(n, e, n + f)
    gen = torch.Generator().manual_seed(n)
    x, y = torch.rand(n, f, t, generator=gen), torch.rand(n, o, generator=gen)
    p = M.init_params(name, f, t, o, num_nodes=n, seed=5)
    fwd = M.graphsage_temporal_gcn if name == "GraphSAGETemporalGCN" else M.gat_temporal
    return Case(p, y, (x, ei), fwd, lambda R: getattr(R, name)(node_features=f, num_nodes=n, periods=t, output_dim=o),
                call=lambda mod, x_, ei_: mod(x_, ei_, None))


def _convstack(collapse):
    """The directed synthetic graph of test_convstack_matches_oracle_on_directed_synthetic_graph."""
    import regtgcn_amd as R
    n, e, f, t, o = 700, 5000, 8, 6, 2
    g = R.data.synthetic_regional_graph(n, e, 3, seed=21)
    (x, y), = R.data.synthetic_snapshots(n, f, t, o, 1, seed=21)
    p = M.init_params("ConvStackedTemporalGCN", f, t, o, seed=22)
    for layer in range(2, 6):
        p[f"tgnn.conv{layer}.lin.weight"] *= 0.5

    def module(R_):
        mod = R_.ConvStackedTemporalGCN(f, t, o)
        mod.collapse = collapse
        return mod

    return Case(p, y, (x, g.edge_index, g.edge_attr), M.conv_stacked_temporal_gcn, module)


def _fixture(golden):
    """The 104-node TPIMS fixture with the shipped checkpoint (6 periods in, 1 out) on the window of one of its golden files."""
    fx = {k: torch.from_numpy(v) for k, v in load_npz("tpims_fixture.npz").items() if v.ndim > 0}
    g = load_npz(golden)
    t_in, t_out, w0 = int(g["t_in"]), int(g["t_out"]), int(g["window"])
    assert (t_in, t_out) == (6, 1)
    n = fx["node_data"].shape[0]
    p = torch.load(os.path.join(GOLDEN, "ref_ckpt_in6_out1_epoch50.pt"), map_location="cpu", weights_only=True)
    x = fx["node_data"][:, :, w0:w0 + t_in].contiguous()
    y = fx["node_data"][:, -1, w0 + t_in:w0 + t_in + t_out].contiguous()
    ri, rw = [fx[f"edge_{r}_index"] for r in REGIONS], [fx[f"edge_{r}_attr"] for r in REGIONS]
    return Case(p, y, (x, fx["edge_index"], ri, rw), M.regional_temporal_gcn, lambda R: R.RegionalTemporalGCN(8, n, t_in, t_out),
                call=lambda mod, x_, ei_, ri_, rw_: mod(x_, ei_, *ri_, *rw_), num_regions=len(REGIONS))


# name -> (builder of the Case, [runtime switch settings to run it under: ((option, value), ...)])
CASES = {
    # RegionalTemporalGCN, small-tile regime; F = 7 is no multiple of 4: generic weight-gradient kernels
    "regt-777-4000-3-8-6-3": (lambda: _regt(777, 4000, 3, 8, 6, 3), [()]),
    "regt-600-4000-3-7-5-2": (lambda: _regt(600, 4000, 3, 7, 5, 2), [()]),
    # big-tile regime (18 000 rows): the smallest shape of the suite that reaches gemm_dgrad1_gen_kernel, the 64-column weight-gradient
    # tile and the region chunk table with grouped reduction.  (Not embed_fp32_kernel: embed_fp32_ok needs 65 536 rows --
    # tests/test_gpu_embed_bars.py holds that kernel.)
    "regt-1500-15000-8-32-12-1": (lambda: _regt(1500, 15000, 8, 32, 12, 1), [((b"dgrad1_gen", 1),), ((b"dgrad1_gen", 0),)]),
    # ragged regions of 1 .. 300 nodes: region chunks of a single node, tiles with three and more regions, region ids without rows
    "ragged-700-8-6-1": (lambda: _ragged(700, 8, 6, 1), [()]),
    # many regions: lins.1's gradient is tiny
    "regt-2000-16000-64-8-6-1": (lambda: _regt(2000, 16000, 64, 8, 6, 1), [()]),
    "tgcn-1409-9000-1-8-6-2": (lambda: _tgcn(1409, 9000, 8, 6, 2), [((b"tgcn_collapse", 1),), ((b"tgcn_collapse", 0),)]),
    "overlap-900-6000-5-8-6-1": (lambda: _overlap(900, 6000, 5, 8, 6, 1), [()]),
    # zero-hidden models: the reset gate is dead, its gradients are exact zeros
    "sage-400-3000-8-6-3": (lambda: _zero_hidden("GraphSAGETemporalGCN", 400, 3000, 8, 6, 3), [()]),
    "gat-400-3000-8-6-3": (lambda: _zero_hidden("GATTemporal", 400, 3000, 8, 6, 3), [()]),
    "convstack-collapsed": (lambda: _convstack(True), [()]),
    "convstack-layerwise": (lambda: _convstack(False), [()]),
    # the fixture's own inputs (the windows of golden_regt_in6_out1 and of golden_regt_ckpt) with the trained checkpoint
    "fixture-ckpt-in6_out1": (lambda: _fixture("golden_regt_in6_out1.npz"), [()]),
    "fixture-ckpt-own-window": (lambda: _fixture("golden_regt_ckpt.npz"), [()]),
}

_CACHE = {}


def case_and_want64(name):
    """(Case, float64 oracle gradients), computed once per case."""
    if name not in _CACHE:
        case = CASES[name][0]()
        _CACHE[name] = (case, case.oracle_grads(torch.float64))
    return _CACHE[name]


def hip_grads_under(R, case, arith, switches):
    """The HIP gradients of `case` under GEMM arithmetic `arith` (0 fp32 MFMA, 1 bf16x3 split) and the given option settings."""
    lib = R.load_library()
    prev_mode = lib.regt_set_gemm_mode(arith)
    prev = [(opt, lib.regt_set_option(opt, val)) for opt, val in switches]
    try:
        return case.hip_grads(R)
    finally:
        for opt, val in reversed(prev):
            lib.regt_set_option(opt, val)
        lib.regt_set_gemm_mode(prev_mode)


def _ids():
    out = []
    for name, (_b, settings) in CASES.items():
        for sw in settings:
            out.append(pytest.param(name, sw, id=name + "".join(f"-{o.decode()}{v}" for o, v in sw)))
    return out


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd
    regtgcn_amd.load_library()
    return regtgcn_amd


@pytest.mark.parametrize("arith", [0, 1], ids=["fp32mfma", "bf16x3split"])
@pytest.mark.parametrize("name,switches", _ids())
def test_every_gradient_block_is_within_its_own_scale_of_float64(R, name, switches, arith):
    case, want64 = case_and_want64(name)
    got = hip_grads_under(R, case, arith, switches)
    for k, w in want64.items():
        assert (got[k] is None) == (w is None), k                      # gradients exist exactly where the oracle's do
    if name.startswith(("sage", "gat")):                               # the exact-zero rule is in play: the dead reset gate
        dead = [k for k, w in want64.items() if w is not None and (".conv_r." in k or ".linear_r." in k)]
        assert len(dead) >= 3 and all(float(want64[k].abs().max()) == 0.0 for k in dead), dead
    assert_grads_to_scale(got, want64, REL, f"{name} arith {arith} {switches}", num_regions=case.num_regions)
