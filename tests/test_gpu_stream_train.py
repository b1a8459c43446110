"""Streamed training on the TPIMS fixture (N = 104), T = 6, O = 1, 2 T + 3 windows: REGT_DIMS_NO_HEAD against a normal backward, the
epoch's gradients of train.train_epoch_streamed against the float64 oracle's summed per-window gradients and against
train.train_epoch_batched (grad_bars.REL, per block), per-window losses against the oracle (rtol 2e-5 / atol 1e-6, tests/test_gpu_stream.py's
tolerances), bit-identical cell gradients whatever the window batch, the command line, a weight update between epochs, the bf16 refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, region_lists
from grad_bars import REL, assert_grads_to_scale, block_ratios
from oracle import model as M

pytestmark = pytest.mark.gpu
T_IN, T_OUT = 6, 1
COUNT = 2 * T_IN + 3
DIRECT = ("tgnn._attention", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias")      # ops.window_backward's outputs


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd
    regtgcn_amd.load_library()
    return regtgcn_amd


@pytest.fixture(params=[0, 1], ids=["fp32mfma", "bf16x3split"])
def arith(request, R):
    lib = R.load_library()
    prev = lib.regt_set_gemm_mode(request.param)
    yield request.param
    lib.regt_set_gemm_mode(prev)


class Capture:
    """An optimizer that keeps the epoch's gradients instead of stepping."""

    def __init__(self, model):
        self.model, self.grads = model, None

    def step(self):
        torch.cuda.synchronize()
        self.grads = {k: (None if p.grad is None else p.grad.detach().cpu().clone()) for k, p in self.model.named_parameters()}

    def zero_grad(self):
        for p in self.model.parameters():
            p.grad = None


def _params(kind, n):
    if kind == "regt":
        return torch.load(os.path.join(GOLDEN, "ref_ckpt_in6_out1_epoch50.pt"), map_location="cpu", weights_only=True)
    return M.init_params("TemporalGCN", 8, T_IN, T_OUT, seed=21)


def _model(R, tpims, kind, p):
    n = tpims["node_data"].shape[0]
    if kind == "regt":
        mod = R.RegionalTemporalGCN(8, n, T_IN, T_OUT)
        mod.load_state_dict(p, strict=True)
        mod = mod.cuda()
        ri, rw = region_lists(tpims)
        ei, ric, rwc = tpims["edge_index"].cuda(), [t.cuda() for t in ri], [t.cuda() for t in rw]
        return mod, (lambda b: mod.prepare_graph(ei, ric, rwc, copies=b))
    mod = R.TemporalGCN(node_features=8, periods=T_IN, output_dim=T_OUT)
    mod.load_state_dict(p, strict=True)
    mod = mod.cuda()
    ei, ea = tpims["edge_index"].cuda(), tpims["edge_attr"].cuda()
    return mod, (lambda b: mod.prepare_graph(ei, ea, n, copies=b))


_ORACLE = {}


def _oracle(tpims, kind):
    """Float64 oracle over the first COUNT windows: (summed gradients, per-window losses); computed once per model kind."""
    if kind not in _ORACLE:
        nd = tpims["node_data"].double()
        p = {k: v.detach().double().requires_grad_(True) for k, v in _params(kind, nd.shape[0]).items()}
        ri, rw = region_lists(tpims)
        rw = [w.double() for w in rw]
        losses = []
        for w in range(COUNT):
            x = nd[:, :, w:w + T_IN].contiguous()
            if kind == "regt":
                pred, _ = M.regional_temporal_gcn(p, x, tpims["edge_index"], ri, rw)
            else:
                pred, _ = M.temporal_gcn(p, x, tpims["edge_index"], tpims["edge_attr"].double())
            loss = torch.mean((pred - nd[:, -1, w + T_IN:w + T_IN + T_OUT]) ** 2)
            loss.backward()
            losses.append(float(loss.detach()))
        _ORACLE[kind] = ({k: v.grad for k, v in p.items()}, losses)
    return _ORACLE[kind]


def _streamed(R, tpims, kind, step_batch=64, p=None):
    mod, build = _model(R, tpims, kind, _params(kind, 0) if p is None else p)
    cap = Capture(mod)
    graphs = R.train.BatchedGraphs(build)
    last, losses = R.train.train_epoch_streamed(mod, tpims["node_data"], T_IN, T_OUT, graphs.get, 0, COUNT, cap, step_batch=step_batch)
    return cap.grads, torch.stack(losses).cpu(), float(last)


def _batched(R, tpims, kind, snap_batch=COUNT):
    mod, build = _model(R, tpims, kind, _params(kind, 0))
    nd = tpims["node_data"]
    xs = [nd[:, :, w:w + T_IN].contiguous().cuda() for w in range(COUNT)]
    ys = [nd[:, -1, w + T_IN:w + T_IN + T_OUT].contiguous().cuda() for w in range(COUNT)]
    cap = Capture(mod)
    _, losses = R.train.train_epoch_batched(mod, R.train.WindowStore(xs, ys), R.train.BatchedGraphs(build), cap, snap_batch)
    return cap.grads, torch.stack(losses).cpu()


def _worst(got, want, regions):
    rows = block_ratios({k: got[k] for k in want}, want, regions)
    return max(((err / scale if scale > 0 else 0.0) / REL[cls], label) for _, label, cls, err, scale in rows)


@pytest.fixture
def gemm_mode(R):
    lib = R.load_library()
    prev = lib.regt_gemm_mode()
    yield lambda mode: lib.regt_set_gemm_mode(mode)
    lib.regt_set_gemm_mode(prev)


@pytest.mark.parametrize("kind,arith", [("regt", 0), ("regt", 1), ("tgcn", 0)], ids=["regt-fp32mfma", "regt-bf16x3split", "tgcn-fp32mfma"])
def test_epoch_gradients_and_losses_match_the_oracle_and_the_batched_path(R, tpims, gemm_mode, kind, arith):
    gemm_mode(arith)
    want, want_losses = _oracle(tpims, kind)
    regions = 5 if kind == "regt" else None
    got, losses, last = _streamed(R, tpims, kind)
    ref, ref_losses = _batched(R, tpims, kind)
    print(f"{kind} arith {arith}: worst block over its bar -- streamed {_worst(got, want, regions)}, batched {_worst(ref, want, regions)}")
    np.testing.assert_allclose(losses.numpy(), want_losses, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(losses.numpy(), ref_losses.numpy(), rtol=2e-5, atol=1e-6)
    assert last == float(losses[-1])
    assert_grads_to_scale(got, want, what=f"streamed epoch vs float64 oracle ({kind})", num_regions=regions)
    # against the batched path by the same bars: its float64-scaled blocks, the batched gradients in the oracle's place
    assert_grads_to_scale(got, {k: (None if v is None else ref[k].double()) for k, v in want.items()},
                          what=f"streamed vs batched ({kind})", num_regions=regions)
    for k, v in got.items():
        if want.get(k) is None:
            assert v is None or float(v.abs().max()) == 0.0, k              # the reference's dead parameters get no gradient


def test_no_head_backward_is_the_normal_backward_with_zero_dpred(R, tpims, arith):
    """regt_backward with REGT_DIMS_NO_HEAD and dhidden alone: the cell, embedding and attention gradients of a normal call with
    dpred = 0 and the same dhidden, bit for bit; the head's gradient buffers stay poisoned."""
    from regtgcn_amd import _lib
    from regtgcn_amd import functional as F_
    mod, build = _model(R, tpims, "regt", _params("regt", 0))
    lib = R.load_library()
    n = tpims["node_data"].shape[0]
    x = tpims["node_data"][:, :, 2:2 + T_IN].contiguous().cuda()
    graph = build(1)
    params = [p.detach() for p in mod._params_in_order()]
    dh = torch.randn(n, 256, generator=torch.Generator().manual_seed(5)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    res = []
    for flags in (0, _lib.DIMS_NO_HEAD):
        pred, hidden, st = F_._regt_forward_call(x, graph, True, 0.01, (False, 0, flags), params, False)
        assert (pred is None) == bool(flags)
        grads = {k: torch.full_like(p, float("nan")) for k, p in zip(st.names, params)}
        gr = F_._fill(_lib.Grads(), grads, True)
        dpred = None if flags else torch.zeros(n, T_OUT, device="cuda")
        _lib.check(lib.regt_backward(C.byref(st.dims), C.byref(st.gs), C.byref(st.ps), C.byref(gr), _lib.ptr(dpred), _lib.ptr(dh),
                                     _lib.ptr(hidden), None, _lib.ptr(st.handle.ws), st.wsb, stream), "regt_backward")
        torch.cuda.synchronize()
        res.append((hidden.cpu(), {k: v.cpu() for k, v in grads.items()}))
    (h0, g0), (h1, g1) = res
    assert torch.equal(h0, h1)
    for k in g0:
        if k in DIRECT[1:]:
            assert bool(torch.isnan(g1[k]).all()), k                        # neither read nor written
            assert not bool(torch.isnan(g0[k]).any()), k
        else:
            assert torch.equal(g0[k], g1[k]), k
    want = {k: v.double() for k, v in g0.items() if k not in DIRECT[1:]}
    assert_grads_to_scale({k: g1[k] for k in want}, want, what="NO_HEAD vs normal backward", num_regions=5)
    # refusals: without the flag a NULL dpred, with it a NULL dhidden
    pred, hidden, st = F_._regt_forward_call(x, graph, True, 0.01, (False, 0, 0), params, False)
    gr = F_._fill(_lib.Grads(), {k: torch.empty_like(p) for k, p in zip(st.names, params)}, True)
    assert lib.regt_backward(C.byref(st.dims), C.byref(st.gs), C.byref(st.ps), C.byref(gr), None, _lib.ptr(dh), _lib.ptr(hidden), None,
                             _lib.ptr(st.handle.ws), st.wsb, stream) != 0
    d2 = _lib.Dims.from_buffer_copy(st.dims)
    d2.flags |= _lib.DIMS_NO_HEAD
    assert lib.regt_backward(C.byref(d2), C.byref(st.gs), C.byref(st.ps), C.byref(gr), None, None, _lib.ptr(hidden), None,
                             _lib.ptr(st.handle.ws), st.wsb, stream) != 0
    assert b"dhidden" in lib.regt_last_error()


@pytest.mark.parametrize("step_batch", [1, 5])
@pytest.mark.parametrize("window_batch", [4, 7])
def test_cell_gradients_are_the_same_bits_whatever_the_window_batch(R, tpims, monkeypatch, window_batch, step_batch):
    """WINDOW_BATCH shorter and longer than the T - 1 slabs a batch inherits: dS is handed over bit-exactly and the steps reach the cell's
    backward in the same groups, so every cell and embedding gradient is the same bits as with one batch; the head and the attention
    logits, summed per batch, stay within the bars."""
    one, losses1, _ = _streamed(R, tpims, "regt", step_batch)
    monkeypatch.setattr(R.serve, "WINDOW_BATCH", window_batch)
    got, losses, _ = _streamed(R, tpims, "regt", step_batch)
    assert torch.equal(losses, losses1)
    for k, v in one.items():
        if v is None:
            assert got[k] is None, k
        elif k not in DIRECT:
            assert torch.equal(got[k], v), k
    want, _ = _oracle(tpims, "regt")
    assert_grads_to_scale(got, want, what=f"WINDOW_BATCH {window_batch}, step_batch {step_batch}", num_regions=5)


def _train_lines(text):
    return [[float(v) for v in re.findall(r"-?\d+\.\d+", ln)] for ln in text.strip().splitlines() if ln.startswith("Train Loss")]


def test_train_command_streamed_train_prints_the_same_lines(R, capsys, tmp_path):
    args = ["--fixture", os.path.join(GOLDEN, "tpims_fixture.npz"), "--model", "RegionalTemporalGCN", "--num_timesteps_in", "6",
            "--num_timesteps_out", "1", "--tr", "0.3", "--epochs", "1", "--tf", "occrate", "--loss_digits", "6"]
    R.train.main(args + ["--out_dir", str(tmp_path / "a")])
    want = _train_lines(capsys.readouterr().out)
    R.train.main(args + ["--out_dir", str(tmp_path / "b"), "--streamed_train"])
    got = _train_lines(capsys.readouterr().out)
    assert len(want) == 2 and all(len(v) == 3 for v in want)
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6)


def test_a_weight_update_between_epochs_is_picked_up(R, tpims):
    nd = tpims["node_data"]
    runs = []
    for streamed in (True, False):
        mod, build = _model(R, tpims, "regt", _params("regt", 0))
        opt = torch.optim.SGD(mod.parameters(), lr=0.05)
        graphs = R.train.BatchedGraphs(build)
        epochs = []
        for _ in range(2):
            if streamed:
                _, losses = R.train.train_epoch_streamed(mod, nd, T_IN, T_OUT, graphs.get, 0, COUNT, opt)
            else:
                xs = [nd[:, :, w:w + T_IN].contiguous().cuda() for w in range(COUNT)]
                ys = [nd[:, -1, w + T_IN:w + T_IN + T_OUT].contiguous().cuda() for w in range(COUNT)]
                _, losses = R.train.train_epoch_batched(mod, R.train.WindowStore(xs, ys), graphs, opt, COUNT)
            epochs.append(torch.stack(losses).cpu().numpy())
        runs.append(epochs)
    (s1, s2), (b1, b2) = runs
    assert not np.allclose(s1, s2, rtol=1e-4, atol=0)                       # the second epoch ran on the updated weights
    np.testing.assert_allclose(s1, b1, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(s2, b2, rtol=2e-5, atol=1e-6)


def test_bf16_arithmetic_is_refused(R, tpims):
    mod, build = _model(R, tpims, "regt", _params("regt", 0))
    mod.arithmetic = "bf16"
    n = tpims["node_data"].shape[0]
    x = tpims["node_data"][:, :, :1].permute(2, 0, 1).contiguous().cuda()
    with pytest.raises(NotImplementedError, match="bf16"):
        mod.period_gradients(x, build(1), torch.zeros(1, n, 256, device="cuda"))
    with pytest.raises(NotImplementedError, match="bf16"):
        R.train.train_epoch_streamed(mod, tpims["node_data"], T_IN, T_OUT, build, 0, COUNT, Capture(mod))
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in mod.parameters())
