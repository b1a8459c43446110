"""Streaming inference on the TPIMS fixture: serve.StreamingPredictor against the reference's goldens, evaluate.predict_metrics_streamed
against the CPU oracle window by window, the stale-weight guard, and the limits of period_outputs.

Tolerances: 1e-5 against the goldens (TOL of tests/test_gpu_model.py, the project's stated tolerance against the reference) and
rtol 2e-5 / atol 1e-6 on the metrics (test_predict_metrics_with_shipped_checkpoint's)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_npz, region_lists
from oracle import loop as oloop
from oracle import model as M

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd
    regtgcn_amd.load_library()
    return regtgcn_amd


@pytest.fixture(params=[0, 1], ids=["fp32mfma", "bf16x3split"])
def arith(request, R):
    """Both fp32-storage GEMM arithmetics, as tests/test_gpu_model.py runs its goldens."""
    lib = R.load_library()
    prev = lib.regt_set_gemm_mode(request.param)
    yield request.param
    lib.regt_set_gemm_mode(prev)


def _cuda_list(ts):
    return [t.cuda() for t in ts]


def _regt(R, tpims, params, t_in, t_out):
    n = tpims["node_data"].shape[0]
    mod = R.RegionalTemporalGCN(8, n, t_in, t_out)
    mod.load_state_dict(params, strict=True)
    mod = mod.cuda().eval()
    ri, rw = region_lists(tpims)
    ei, ric, rwc = tpims["edge_index"].cuda(), _cuda_list(ri), _cuda_list(rw)
    return mod, (lambda b: mod.prepare_graph(ei, ric, rwc, copies=b))


def _push_until(sp, node_data, last_step):
    """Pushes steps 0 .. last_step; every push before T steps are in returns None.  Returns the last push's result."""
    out = None
    for s in range(last_step + 1):
        out = sp.push(node_data[:, :, s].contiguous().cuda())
        assert (out is None) == (s + 1 < sp.periods), s
        assert sp.steps_seen == s + 1
    return out


@pytest.mark.parametrize("tag", ["in6_out1", "in12_out1", "in12_out3", "ckpt"])
def test_streaming_regt_matches_reference_goldens(R, arith, tpims, tag):
    g = load_npz(f"golden_regt_{tag}.npz")
    t_in, t_out, w0 = int(g["t_in"]), int(g["t_out"]), int(g["window"])
    n = tpims["node_data"].shape[0]
    if tag == "ckpt":
        p = torch.load(os.path.join(GOLDEN, "ref_ckpt_in6_out1_epoch50.pt"), map_location="cpu", weights_only=True)
    else:
        p = M.init_params("RegionalTemporalGCN", 8, t_in, t_out, num_nodes=n, seed=int(g["seed"]))
    mod, build = _regt(R, tpims, p, t_in, t_out)
    sp = R.StreamingPredictor(mod, build(1))
    pred, hidden = _push_until(sp, tpims["node_data"], w0 + t_in - 1)          # w0 > 0: the ring has wrapped by then
    assert pred.shape == (n, t_out) and hidden.shape == (n, 256)
    np.testing.assert_allclose(pred.cpu().numpy(), g["pred"], atol=TOL)
    np.testing.assert_allclose(hidden.cpu().numpy(), g["hidden"], atol=TOL)


@pytest.mark.parametrize("tag", ["in6_out1", "in12_out3"])
def test_streaming_temporal_gcn_matches_reference_goldens(R, arith, tpims, tag):
    g = load_npz(f"golden_tgcn_{tag}.npz")
    t_in, t_out, w0 = int(g["t_in"]), int(g["t_out"]), int(g["window"])
    n = tpims["node_data"].shape[0]
    mod = R.TemporalGCN(node_features=8, periods=t_in, output_dim=t_out)
    mod.load_state_dict(M.init_params("TemporalGCN", 8, t_in, t_out, seed=int(g["seed"])), strict=True)
    mod = mod.cuda().eval()
    sp = R.StreamingPredictor(mod, mod.prepare_graph(tpims["edge_index"].cuda(), tpims["edge_attr"].cuda(), n))
    pred, hidden = _push_until(sp, tpims["node_data"], w0 + t_in - 1)
    np.testing.assert_allclose(pred.cpu().numpy(), g["pred"], atol=TOL)
    np.testing.assert_allclose(hidden.cpu().numpy(), g["hidden"], atol=TOL)


_ORACLE = {}


def _oracle_windows(tpims, p, t_in, t_out, count):
    """The CPU oracle on the first ``count`` windows, one by one; computed once."""
    if "w" not in _ORACLE:
        ri, rw = region_lists(tpims)
        xs, ys = oloop.make_windows(tpims["node_data"][:, :, :count + t_in + t_out - 1], t_in, t_out)
        with torch.no_grad():
            outs = [M.regional_temporal_gcn(p, x.contiguous(), tpims["edge_index"], ri, rw) for x in xs]
        replay = iter(outs)                                    # the metrics read the same oracle outputs, in window order
        _ORACLE["w"] = (outs, oloop.predict_metrics(p, lambda prm, x: next(replay), xs, ys), xs, ys)
    return _ORACLE["w"]


@pytest.mark.parametrize("step_batch", [1, 5, 64])
def test_streamed_evaluation_matches_oracle_window_by_window(R, tpims, step_batch):
    """The first 2 T + 3 consecutive windows: metrics and every window's pred / hidden against the oracle; per-window hidden the same
    bits as StreamingPredictor pushes over the same steps."""
    t_in, t_out = 6, 1
    count = 2 * t_in + 3
    p = torch.load(os.path.join(GOLDEN, "ref_ckpt_in6_out1_epoch50.pt"), map_location="cpu", weights_only=True)
    outs, want, _, _ = _oracle_windows(tpims, p, t_in, t_out, count)
    mod, build = _regt(R, tpims, p, t_in, t_out)
    nd = tpims["node_data"]
    got = R.evaluate.predict_metrics_streamed(mod, nd, t_in, t_out, build, 0, count, step_batch=step_batch)
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-6)
    rm = R.train.evaluate_streamed(mod, nd, t_in, t_out, build, 0, count, step_batch=step_batch)
    ys = torch.stack([nd[:, -1, i + t_in:i + t_in + t_out] for i in range(count)])
    mse = float(((torch.stack([o[0] for o in outs]) - ys) ** 2).mean())
    np.testing.assert_allclose(rm, (mse ** 0.5, mse), rtol=2e-5, atol=1e-6)
    chunks = list(R.serve.window_outputs(mod, nd, t_in, build, 0, count, step_batch))
    assert [c[0] for c in chunks] == list(range(0, count, R.serve.WINDOW_BATCH))
    pred = torch.cat([c[1] for c in chunks])
    hidden = torch.cat([c[2] for c in chunks])
    for i, (op, oh) in enumerate(outs):
        np.testing.assert_allclose(pred[i].cpu().numpy(), op.numpy(), atol=TOL)
        np.testing.assert_allclose(hidden[i].cpu().numpy(), oh.numpy(), atol=TOL)
    sp = R.StreamingPredictor(mod, build(1))
    for s in range(count + t_in - 1):
        out = sp.push(nd[:, :, s].contiguous().cuda())
        if s >= t_in - 1:
            assert torch.equal(out[1], hidden[s - t_in + 1]), (step_batch, s)
            assert torch.equal(out[0], pred[s - t_in + 1]), (step_batch, s)


@pytest.mark.parametrize("window_batch", [4, 7])
def test_timeline_is_bounded_and_batches_hand_over_their_last_slabs(R, tpims, monkeypatch, window_batch):
    """window_outputs keeps WINDOW_BATCH + T - 1 slabs whatever the window count: with small batches (shorter and longer than the
    T - 1 slabs a batch inherits) every window is the same bits as in one batch."""
    t_in, count = 6, 15
    n = tpims["node_data"].shape[0]
    mod, build = _regt(R, tpims, M.init_params("RegionalTemporalGCN", 8, t_in, 1, num_nodes=n, seed=9), t_in, 1)
    graphs = R.train.BatchedGraphs(build)
    nd = tpims["node_data"]
    (i0, pred, hidden), = list(R.serve.window_outputs(mod, nd, t_in, graphs.get, 2, count, 5))
    assert i0 == 2
    monkeypatch.setattr(R.serve, "WINDOW_BATCH", window_batch)
    chunks = list(R.serve.window_outputs(mod, nd, t_in, graphs.get, 2, count, 5))
    assert [c[0] for c in chunks] == list(range(2, 2 + count, window_batch))
    assert torch.equal(torch.cat([c[2] for c in chunks]), hidden) and torch.equal(torch.cat([c[1] for c in chunks]), pred)


def _last_floats(text):
    import re
    return [float(v) for v in re.findall(r"-?\d+\.\d+", text.strip().splitlines()[-1])]


def test_evaluate_command_streamed_prints_the_same_metrics(R, capsys):
    args = ["--fixture", os.path.join(GOLDEN, "tpims_fixture.npz"), "--checkpoint", os.path.join(GOLDEN, "ref_ckpt_in6_out1_epoch50.pt"),
            "--model", "RegionalTemporalGCN", "--num_timesteps_in", "6", "--num_timesteps_out", "1", "--tr", "0.2"]
    R.evaluate.main(args)
    want = _last_floats(capsys.readouterr().out)
    R.evaluate.main(args + ["--streamed"])
    got = _last_floats(capsys.readouterr().out)
    assert len(want) == 3
    np.testing.assert_allclose(got, want, atol=2e-4)           # the command prints four decimals


def test_train_command_streamed_prints_the_same_test_metrics(R, capsys, tmp_path):
    args = ["--fixture", os.path.join(GOLDEN, "tpims_fixture.npz"), "--model", "TemporalGCN", "--num_timesteps_in", "6",
            "--num_timesteps_out", "1", "--tr", "0.5", "--epochs", "1", "--tf", "occrate", "--loss_digits", "6"]
    R.train.main(args + ["--out_dir", str(tmp_path / "a")])
    want = [_last_floats(ln) for ln in capsys.readouterr().out.strip().splitlines() if ln.startswith("Train Loss")]
    R.train.main(args + ["--out_dir", str(tmp_path / "b"), "--streamed"])
    got = [_last_floats(ln) for ln in capsys.readouterr().out.strip().splitlines() if ln.startswith("Train Loss")]
    assert len(want) == 2 and all(len(v) == 3 for v in want)
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)


def test_stale_weights_are_refused_until_reset(R, tpims):
    t_in = 6
    n = tpims["node_data"].shape[0]
    mod, build = _regt(R, tpims, M.init_params("RegionalTemporalGCN", 8, t_in, 1, num_nodes=n, seed=3), t_in, 1)
    sp = R.StreamingPredictor(mod, build(1))
    x = tpims["node_data"][:, :, 0].contiguous().cuda()
    for _ in range(t_in):
        out = sp.push(x)
    assert out is not None
    with torch.no_grad():
        mod.linear2.bias.add_(1.0)                             # an optimizer step does the same: in place, _version moves
    with pytest.raises(R.RegtError, match="reset"):
        sp.push(x)
    assert sp.steps_seen == t_in                               # the refused push cached nothing
    sp.reset()
    assert sp.steps_seen == 0
    for s in range(t_in):
        new = sp.push(x)
        assert (new is None) == (s + 1 < t_in)
    assert torch.allclose(new[0], out[0] + 1.0, atol=1e-6) and torch.equal(new[1], out[1])
    with pytest.raises(R.RegtError):
        sp.push(x.cpu())


def test_period_outputs_is_gradient_free_and_is_the_t1_hidden(R, tpims):
    t_in = 6
    n = tpims["node_data"].shape[0]
    mod, build = _regt(R, tpims, M.init_params("RegionalTemporalGCN", 8, t_in, 1, num_nodes=n, seed=5), t_in, 1)
    mod.train()
    assert torch.is_grad_enabled() and all(q.requires_grad for q in mod.parameters())
    x = tpims["node_data"][:, :, 3:5].permute(2, 0, 1).contiguous().cuda().requires_grad_(True)
    s = mod.period_outputs(x, build(2))
    assert s.shape == (2, n, 256) and not s.requires_grad and s.grad_fn is None
    # one period with probability 1: the T = 1 model's hidden on the same step
    one = R.RegionalTemporalGCN(8, n, 1, 1).cuda()
    sd = {k: v for k, v in mod.state_dict().items() if k != "tgnn._attention"}
    sd["tgnn._attention"] = torch.zeros(1, device="cuda")
    one.load_state_dict(sd)
    with torch.no_grad():
        _, h = one.forward_prepared(x[1].detach().unsqueeze(2).contiguous(), build(1))
    np.testing.assert_allclose(s[1].cpu().numpy(), h.cpu().numpy(), atol=TOL)
    with pytest.raises(ValueError):
        mod.period_outputs(x, build(1))                        # two steps on a one-copy graph


def test_bf16_arithmetic_is_refused(R, tpims):
    n = tpims["node_data"].shape[0]
    mod, build = _regt(R, tpims, M.init_params("RegionalTemporalGCN", 8, 6, 1, num_nodes=n, seed=5), 6, 1)
    x = tpims["node_data"][:, :, :1].permute(2, 0, 1).contiguous().cuda()
    mod.arithmetic = "bf16"
    with pytest.raises(NotImplementedError, match="bf16"):
        mod.period_outputs(x, build(1))
    with pytest.raises(NotImplementedError, match="bf16"):
        R.StreamingPredictor(mod, build(1)).push(x[0])
    mod.arithmetic = None
    lib = R.load_library()
    prev = lib.regt_set_gemm_mode(2)
    try:
        with pytest.raises(NotImplementedError, match="bf16"):
            mod.period_outputs(x, build(1))
        mod.arithmetic = "bf16x3"                              # the model's own arithmetic is honoured over the process default
        assert mod.period_outputs(x, build(1)).shape == (1, n, 256)
    finally:
        lib.regt_set_gemm_mode(prev)
