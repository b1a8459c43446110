"""SpatialGCN on the HIP path: the reference module's goldens (eval, and train with the recorded dropout masks), the fused first-layer
kernel pair against a float64 restatement on awkward graphs, reproducibility, the drawn dropout mask, snapshot batching, the cfg-3
shape, and the train / evaluate command lines.

Next to every gradient comparison stands grad_bars.assert_grads_conditioned: every block (gcn.lins.0 and gcn.lins.1 by 16-feature
accumulator) against the float64 restatement -- for the goldens, which store only summaries of the large gradients, the one
full reference -- at a bar relative to the block's OWN scale; no block of these cases is ill-conditioned."""
import os
import time

import numpy as np
import pytest
import torch

from conftest import GOLDEN, check_grads_against_golden, load_npz
from grad_bars import REL, assert_grads_conditioned
from oracle import graph_ops as G
from spatial_math import spatial_gcn, unpack_keep

pytestmark = pytest.mark.gpu
TOL = 1e-5
K_GAP = 4                     # what an ill-conditioned block's fp32 gap is multiplied by: the summation-order allowance of the
                              # STNorm and STID tests (torch sums pairwise; the kernels add tiles, waves and chunks in sequence)


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd as R
    R.load_library()
    return R


def _golden(tag):
    g = load_npz(f"golden_spatial_{tag}.npz")
    return g, {str(k): torch.from_numpy(g[f"p__{k}"]) for k in g["state_dict_keys"]}


def golden_case(tpims, tag, mode):
    """The float64 and fp32 restatement gradients of the golden's step (its parameters, window, recorded keep mask and loss).  The
    goldens keep only summaries of the large gradients: the float64 restatement is the one full reference."""
    g, params = _golden(tag)
    t_in, t_out, w0 = int(g["t_in"]), int(g["t_out"]), int(g["window"])
    x = tpims["node_data"][:, :, w0:w0 + t_in].contiguous()
    y = tpims["node_data"][:, -1, w0 + t_in:w0 + t_in + t_out].contiguous()
    keep = g["train__keep"] if mode == "train" else None
    out = []
    for dtype in (torch.float64, torch.float32):
        p = {k: v.to(dtype).requires_grad_(True) for k, v in params.items()}
        pred, _hidden = spatial_gcn(p, x, tpims["edge_index"], tpims["edge_attr"], keep, dtype=dtype)
        torch.mean((pred - y.to(dtype)) ** 2).backward()
        out.append({k: v.grad for k, v in p.items()})
    return out


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("tag", ["in6_out1", "in12_out3"])
def test_spatial_matches_reference_goldens(R, tpims, tag, mode):
    g, params = _golden(tag)
    rec = {k[len(mode) + 2:]: v for k, v in g.items() if k.startswith(mode + "__")}
    t_in, t_out, w0 = int(g["t_in"]), int(g["t_out"]), int(g["window"])
    x = tpims["node_data"][:, :, w0:w0 + t_in].contiguous().cuda()
    y = tpims["node_data"][:, -1, w0 + t_in:w0 + t_in + t_out].contiguous().cuda()
    mod = R.SpatialGCN(8, t_in, t_out)
    mod.load_state_dict(params, strict=True)
    mod = mod.cuda()
    n = x.shape[0]
    op = mod.prepare_graph(tpims["edge_index"].cuda(), tpims["edge_attr"].cuda(), n)
    if mode == "train":
        mod.train()
        pred, hidden = mod.forward_prepared(x, op, keep=torch.from_numpy(rec["keep"]).cuda())
    else:
        mod.eval()
        pred, hidden = mod(x, tpims["edge_index"].cuda(), tpims["edge_attr"].cuda())      # positional call, run.py:224
    loss = torch.mean((pred - y) ** 2)
    loss.backward()
    np.testing.assert_allclose(pred.detach().cpu().numpy(), rec["pred"], atol=TOL)
    np.testing.assert_allclose(hidden.detach().cpu().numpy(), rec["hidden"], atol=TOL)
    assert abs(float(loss.detach()) - float(rec["loss"][0])) < TOL
    grads = {k: (None if q.grad is None else q.grad.cpu()) for k, q in mod.named_parameters()}
    check_grads_against_golden(rec, grads, atol=TOL, rtol=1e-4)
    g64, g32 = golden_case(tpims, tag, mode)
    ill, _ = assert_grads_conditioned(grads, g64, g32, K_GAP, REL, f"golden {tag} {mode}")
    assert ill == []


def _awkward_graph(R, n, e, seed):
    """Directed synthetic graph on the first n - 3 nodes (3 isolated nodes), plus a self loop and a duplicated edge."""
    g = R.data.synthetic_regional_graph(n - 3, e, 3, seed=seed)
    ei, ea = g.edge_index, g.edge_attr
    ei = torch.cat([ei, torch.tensor([[1], [1]]), ei[:, :1]], dim=1).contiguous()
    ea = torch.cat([ea, torch.tensor([500.0]), ea[:1]]).contiguous()
    return ei, ea


def _embed_reference(x, ei, ea, w0, w1, b, keep, ds, dtype=torch.float64):
    """float64 S, (dW0, dW1, db), the absolute-value sums that bound their fp32 rounding, and the allowance for ReLU decisions that
    fp32 may take either way (|pre| within fp32 rounding of 0: the whole row term may or may not count), in the reference's order."""
    n, f, t = x.shape
    x, w0, w1, b, ds = x.to(dtype), w0.to(dtype), w1.to(dtype), b.to(dtype), ds.to(dtype)
    src, dst, w = G.cheb_norm_edges(ei, ea.to(dtype), n, dtype)
    km = None if keep is None else unpack_keep(keep.cpu().numpy(), n, t).to(dtype) * 2
    zeros = lambda: [torch.zeros(64, f, dtype=dtype), torch.zeros(64, f, dtype=dtype), torch.zeros(64, dtype=dtype)]
    s = torch.zeros(n, 64, dtype=dtype)
    grads, bounds, allow = zeros(), zeros(), zeros()
    for p in range(t):
        xt = x[:, :, p]
        lxt = G.propagate(src, dst, w, xt, n)
        pre = xt @ w0.t() + lxt @ w1.t() + b
        m = (pre > 0).to(dtype) if km is None else (pre > 0).to(dtype) * km[:, p, :]
        s += torch.relu(pre) * (1.0 if km is None else km[:, p, :])
        dg = ds * m
        grads[0] += dg.t() @ xt
        grads[1] += dg.t() @ lxt
        grads[2] += dg.sum(0)
        bounds[0] += dg.abs().t() @ xt.abs()
        bounds[1] += dg.abs().t() @ lxt.abs()
        bounds[2] += dg.abs().sum(0)
        size = xt.abs() @ w0.abs().t() + lxt.abs() @ w1.abs().t() + b.abs()
        amb = (pre.abs() <= 4e-6 * size).to(dtype) * (ds.abs() if km is None else ds.abs() * km[:, p, :])
        allow[0] += amb.t() @ xt.abs()
        allow[1] += amb.t() @ lxt.abs()
        allow[2] += amb.sum(0)
    return s, grads, bounds, allow


def _embed_gpu(R, x, ei, ea, w0, w1, b, keep, ds):
    n, f, t = x.shape
    op = R.graph.prepare_cheb_operator(ei.cuda(), ea.cuda(), n)
    xp = R.ops.pack_x(x.cuda())
    lxp = R.ops.spmm_csr(op.rowptr, op.col, op.val, xp.view(n, t * f)).view(n, t, f)
    w0, w1, b, ds = w0.cuda(), w1.cuda(), b.cuda(), ds.cuda()
    s = R.ops.spatial_embed_forward(xp, lxp, w0, w1, b, keep)
    return s, R.ops.spatial_embed_backward(xp, lxp, w0, w1, b, keep, ds)


def _inputs(n, t, f, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, f, t, generator=g)
    w0 = torch.randn(64, f, generator=g) / f ** 0.5
    w1 = torch.randn(64, f, generator=g) / f ** 0.5
    b = torch.randn(64, generator=g) * 0.2
    ds = torch.randn(n, 64, generator=g)
    return x, w0, w1, b, ds


EMBED_NAMES = ("gcn.lins.0.weight", "gcn.lins.1.weight", "gcn.bias")            # what the kernel pair's dW0, dW1, db are gradients of


def embed_case(x, ei, ea, w0, w1, b, keep, ds):
    """(float64 reference of _check, {name: float64 gradient}, {name: fp32 restatement gradient}, {name: ReLU allowance}): the
    restatement runs once per arithmetic and serves both assertions."""
    ref = _embed_reference(x, ei, ea, w0, w1, b, keep, ds)
    g32 = _embed_reference(x, ei, ea, w0, w1, b, keep, ds, dtype=torch.float32)[1]
    return ref, dict(zip(EMBED_NAMES, ref[1])), dict(zip(EMBED_NAMES, g32)), dict(zip(EMBED_NAMES, ref[3]))


def _check(s, grads, s_ref, g_ref, bounds, allow):
    scale = max(1.0, float(s_ref.abs().max()))
    assert float((s.cpu().double() - s_ref).abs().max()) < TOL * scale
    for got, ref, bnd, alw, name in zip(grads, g_ref, bounds, allow, ("dW0", "dW1", "db")):
        err = (got.cpu().double() - ref).abs()
        assert bool((err <= TOL * bnd + alw + 1e-6).all()), (name, float(err.max()), float(bnd.max()))


def _check_to_scale(grads, g64, g32, allow, what):
    """Every block of dW0, dW1, db within its own scale of float64; an element whose ReLU decision fp32 may take either way
    (`allow`, from the float64 pre-activations alone) keeps the allowance _check gives it."""
    got = dict(zip(EMBED_NAMES, (g.cpu() for g in grads)))
    return assert_grads_conditioned(got, g64, g32, K_GAP, REL, what, allow=allow)


KERNEL_PAIR_SHAPES = [(40, 1, 4), (300, 12, 32), (1000, 6, 8), (257, 13, 64)]


def kernel_pair_inputs(R, n, t, f):
    ei, ea = _awkward_graph(R, n, 6 * n, seed=n + t)
    return (ei, ea) + _inputs(n, t, f, seed=7 * n + f)


@pytest.mark.parametrize("masked", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("n,t,f", KERNEL_PAIR_SHAPES)
def test_kernel_pair_matches_restatement(R, n, t, f, masked):
    ei, ea, x, w0, w1, b, ds = kernel_pair_inputs(R, n, t, f)
    keep = R.nn.draw_keep_mask(n * t, "cuda") if masked else None
    s, grads = _embed_gpu(R, x, ei, ea, w0, w1, b, keep, ds)
    ref, g64, g32, allow = embed_case(x, ei, ea, w0, w1, b, keep, ds)
    _check(s, grads, *ref)
    ill, _ = _check_to_scale(grads, g64, g32, allow, f"n {n} t {t} f {f} masked {masked}")
    assert ill == []


def test_forward_backward_bit_identical(R):
    n, t, f = 5000, 12, 32
    ei, ea = _awkward_graph(R, n, 8 * n, seed=3)
    x, w0, w1, b, ds = _inputs(n, t, f, seed=4)
    keep = R.nn.draw_keep_mask(n * t, "cuda")
    s1, g1 = _embed_gpu(R, x, ei, ea, w0, w1, b, keep, ds)
    s2, g2 = _embed_gpu(R, x, ei, ea, w0, w1, b, keep, ds)
    assert torch.equal(s1, s2)
    assert all(torch.equal(a, c) for a, c in zip(g1, g2))


def test_drawn_mask_keeps_half_and_uses_every_bit(R):
    keep = R.nn.draw_keep_mask(200_000, "cuda")
    assert keep.dtype == torch.int32 and tuple(keep.shape) == (200_000, 2)
    bits = unpack_keep(keep.cpu().numpy(), 200_000, 1).reshape(200_000, 64).double()
    assert 0.49 <= float(bits.mean()) <= 0.51
    per_bit = bits.mean(0)
    assert bool((per_bit > 0.45).all()) and bool((per_bit < 0.55).all())        # bit 31 of each word included


def test_training_mode_draws_fresh_masks_and_eval_is_deterministic(R, tpims):
    mod = R.SpatialGCN(8, 6, 1).cuda()
    x = tpims["node_data"][:, :, :6].contiguous().cuda()
    ei, ea = tpims["edge_index"].cuda(), tpims["edge_attr"].cuda()
    mod.train()
    a, _ = mod(x, ei, ea)
    c, _ = mod(x, ei, ea)
    assert not torch.equal(a, c)
    mod.eval()
    d, _ = mod(x, ei, ea)
    e, _ = mod(x, ei, ea)
    assert torch.equal(d, e)


def test_snapshot_batching_equals_separate_calls(R, tpims):
    mod = R.SpatialGCN(8, 6, 1).cuda().eval()
    n = tpims["node_data"].shape[0]
    ei, ea = tpims["edge_index"].cuda(), tpims["edge_attr"].cuda()
    xs = [tpims["node_data"][:, :, i:i + 6].contiguous().cuda() for i in range(0, 16, 4)]
    op1 = mod.prepare_graph(ei, ea, n)
    op4 = mod.prepare_graph(ei, ea, n, copies=4)
    with torch.no_grad():
        sep = [mod.forward_prepared(x, op1) for x in xs]
        pred, hid = mod.forward_prepared(torch.cat(xs, dim=0), op4)
    ref_p, ref_h = torch.cat([p for p, _ in sep]), torch.cat([h for _, h in sep])
    assert float((pred - ref_p).abs().max()) <= 1e-6 * max(1.0, float(ref_p.abs().max()))
    assert float((hid - ref_h).abs().max()) <= 1e-6 * max(1.0, float(ref_h.abs().max()))


def test_cfg3_shape_matches_restatement(R):
    """The full cfg-3 shape (N = 100k, E = 1M, F = 32, T = 12), forward + backward, masked."""
    t0 = time.time()
    n, e, t, f = 100_000, 1_000_000, 12, 32
    g = R.data.synthetic_regional_graph(n, e, 5, seed=31)
    x, w0, w1, b, ds = _inputs(n, t, f, seed=32)
    keep = R.nn.draw_keep_mask(n * t, "cuda")
    s, grads = _embed_gpu(R, x, g.edge_index, g.edge_attr, w0, w1, b, keep, ds)
    ref, g64, g32, allow = embed_case(x, g.edge_index, g.edge_attr, w0, w1, b, keep, ds)
    _check(s, grads, *ref)
    ill, _ = _check_to_scale(grads, g64, g32, allow, "cfg-3 shape")
    assert ill == []
    assert time.time() - t0 < 120


@pytest.mark.parametrize("snap_batch", [1, 16])
def test_train_and_evaluate_command_lines(R, tmp_path, capsys, snap_batch):
    from regtgcn_amd import evaluate, train
    fx = os.path.join(GOLDEN, "tpims_fixture.npz")
    argv = ["--model", "SpatialGCN", "--num_timesteps_in", "6", "--num_timesteps_out", "1", "--tr", "0.2", "--tf", "occrate",
            "--epochs", "1", "--snap_batch", str(snap_batch), "--fixture", fx, "--out_dir", str(tmp_path)]
    train.main(argv)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Train Loss:")]
    assert len(lines) == 2
    losses = [float(ln.split("Train Loss:")[1].split(",")[0]) for ln in lines]
    assert all(np.isfinite(losses))
    ck = tmp_path / "occrate" / "SpatialGCN" / "model_in6_out1_epoch0.pt"
    assert ck.exists()
    sd = torch.load(str(ck), map_location="cpu", weights_only=True)
    R.SpatialGCN(8, 6, 1).load_state_dict(sd, strict=True)
    evaluate.main(["--model", "SpatialGCN", "--fixture", fx, "--checkpoint", str(ck), "--snap_batch", str(snap_batch)])
    out = capsys.readouterr().out
    assert "RMSE:" in out
