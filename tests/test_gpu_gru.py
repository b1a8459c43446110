"""StackedGRU on the GPU: the reference module's goldens in training and eval mode with the run.py / predict.py metrics, the
three-window RMSprop trajectory, the layer entry points against the float64 restatement over input sizes, row counts, sequence
lengths, optional h0 / out / h_last and an upstream gradient on every row, output widths, bit-reproducibility of the backward,
stacked snapshots against sequential calls, and the train / evaluate command lines.

Every comparison is per tensor: max |difference| / max |reference| against gru_math.bar(gap), the gap being the fp32 reference's
own distance to float64 for that tensor and shape class (the constants of gru_math.py).

Measured on an MI355X: goldens, output 3.4e-7, gradients at most 2.5e-7; layer cases up to seq 104, at most 6.0e-7 (dW_ih); the
4096-step case out 9.8e-8, h_last 1.1e-7, dW_ih 4.4e-7, dW_hh 5.3e-7, db_ih 4.3e-7, db_hh 4.3e-7, dh0 1.1e-7 against bars of
1.9e-6 (out, h_last, db_ih, dh0), 3.4e-6 (dW_ih), 1.9e-5 (dW_hh) and 1.7e-5 (db_hh).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_npz
from gru_math import (GRAD_GAP, GRAD_GAP_ANY, KEYS, LAYER_GAP, OUT_GAP, OUT_GAP_ANY, bar, build_params, check_stored, gru_layer, rel_err,
                      rmsprop_first_step, stacked_gru, trajectory)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["in6_out1", "in12_out3"]
DEV = "cuda:0"


def _model(tag):
    import regtgcn_amd as R
    g = load_npz(f"golden_gru_{tag}.npz")
    t_in, t_out = int(g["t_in"]), int(g["t_out"])
    params = build_params(int(g["seed"]), t_in, t_out)
    mod = R.StackedGRU(t_in, 8, t_in, t_out)
    mod.load_state_dict(params)
    return g, params, mod.to(DEV)


@pytest.mark.parametrize("tag", TAGS)
def test_training_golden(tag):
    g, params, mod = _model(tag)
    mod.train()
    out = mod(torch.from_numpy(g["x"]).to(DEV), None)
    y = torch.from_numpy(g["y"]).to(DEV)
    loss = torch.mean((out[:, -1, :] - y) ** 2)
    loss.backward()
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    o64 = stacked_gru(p64, torch.from_numpy(g["x"]))
    torch.mean((o64[:, -1, :] - torch.from_numpy(g["y"]).double()) ** 2).backward()
    grads = dict(mod.named_parameters())
    print("out", rel_err(out, o64), {k: f"{rel_err(grads[k].grad, p64[k].grad):.2e}" for k in KEYS})
    assert rel_err(out, o64) <= bar(OUT_GAP[tag])
    assert rel_err(out, torch.from_numpy(g["train__out"])) <= bar(OUT_GAP[tag])
    assert abs(loss.item() - g["train__loss"][0]) <= bar(OUT_GAP[tag]) * g["train__loss"][0]
    for k in KEYS:
        assert rel_err(grads[k].grad, p64[k].grad) <= bar(GRAD_GAP[tag][k]), k
    check_stored(g, "train__g__", {k: grads[k].grad for k in KEYS}, lambda k: bar(GRAD_GAP[tag][k]), "grad")


@pytest.mark.parametrize("tag", TAGS)
def test_eval_golden_and_metrics(tag):
    from regtgcn_amd.evaluate import predict_metrics_gru
    from regtgcn_amd.train import WindowStore, evaluate_gru
    g, params, mod = _model(tag)
    mod.eval()
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    with torch.no_grad():
        out = mod(x)
    assert tuple(out.shape) == (104, 8, int(g["t_out"]))
    b = bar(OUT_GAP[tag])
    assert rel_err(out, torch.from_numpy(g["eval__out"])) <= b
    # the errors y - out are larger than the outputs here (max |out| 0.08, mean |y - out| 0.4), so an output error of b max |out|
    # moves the metrics that are linear in the error by less than b of their value and the squared ones by less than 2 b
    rmse, mse = evaluate_gru(mod, WindowStore([x], [y]), 1)
    assert abs(mse - g["eval__test_mse"][0]) <= 2 * b * g["eval__test_mse"][0] and abs(rmse - mse ** 0.5) < 1e-12
    mae, rmse2, mape = predict_metrics_gru(mod, [x], [y], 1)
    assert abs(mae - g["eval__mae"][0]) <= b * g["eval__mae"][0]
    assert abs(rmse2 ** 2 - g["eval__mse"][0]) <= 2 * b * g["eval__mse"][0]
    assert abs(mape - g["eval__mape"][0]) <= b * g["eval__mape"][0]


@pytest.mark.parametrize("tag", TAGS)
def test_trajectory_golden(tag, tpims):
    from regtgcn_amd.train import WindowStore, train_epoch_gru
    g, params, mod = _model(tag)
    t_in, t_out, w = int(g["t_in"]), int(g["t_out"]), int(g["window"])
    xs = [tpims["node_data"][:, :, w + k:w + k + t_in].contiguous().to(DEV) for k in range(3)]
    ys = [tpims["node_data"][:, -1, w + k + t_in:w + k + t_in + t_out].contiguous().to(DEV) for k in range(3)]
    opt = torch.optim.RMSprop(mod.parameters(), lr=1e-3, weight_decay=1e-4)
    last, losses = train_epoch_gru(mod, WindowStore(xs, ys), opt, 1)
    np.testing.assert_allclose([float(l) for l in losses], g["traj__loss"], rtol=bar(OUT_GAP[tag]))
    assert float(last) == float(losses[-1])
    # the accumulated float64 gradient gives the conditioning of the RMSprop step (test_gru_cpu.test_restatement_reproduces_trajectory)
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    trajectory(tpims, g, lambda x, y: torch.mean((stacked_gru(p64, x)[:, -1, :] - y.double()) ** 2))
    now = dict(mod.named_parameters())
    # golden and kernel are each within the gradient's bar of the float64 gradient (hence 2 x); both round the fp32 update
    steps, bounds = {}, {}
    for k in KEYS:
        _, sens = rmsprop_first_step(p64[k].grad, params[k])
        steps[k] = now[k].detach().cpu().double() - params[k].double()
        bounds[k] = 2 * sens * (bar(GRAD_GAP[tag][k]) * float(p64[k].grad.abs().max())) + 2.0 ** -22 * params[k].abs().double() + 32 * 2.0 ** -24 * 1e-2
    check_stored(g, "traj__dp__", steps, lambda k: bounds[k], "step")


# (seq, rows, input size, h0, out, h_last): every input size, row count and sequence length of the issue, each optional pointer
LAYER_CASES = [(104, 8, 12, False, True, True), (104, 8, 12, True, True, True), (104, 8, 6, True, False, True),
               (104, 8, 12, True, True, False), (9, 8, 1, True, True, True), (9, 9, 37, True, True, True), (5, 16, 255, True, True, True),
               (6, 1, 6, True, True, True), (6, 7, 12, False, True, True), (6, 100, 12, True, True, True), (4, 512, 12, True, True, True),
               (1, 8, 12, True, True, True), (2, 9, 6, False, True, True), (4096, 8, 12, True, True, True)]


@pytest.mark.parametrize("seq,rows,t,use_h0,want_out,want_last", LAYER_CASES)
def test_layer_against_restatement(seq, rows, t, use_h0, want_out, want_last):
    from regtgcn_amd import ops
    gen = torch.Generator().manual_seed(seq * 1000 + rows * 10 + t)
    ref = torch.nn.GRU(t, 256)
    w = [q.detach() for q in ref.parameters()]
    x = torch.randn(seq, rows, t, generator=gen)
    h0 = torch.randn(1, rows, 256, generator=gen) * 0.5 if use_h0 else None
    dout = torch.randn(seq, rows, 256, generator=gen) if want_out else None            # an upstream gradient on every row
    dlast = torch.randn(1, rows, 256, generator=gen) if want_last else None
    w64 = [q.double().requires_grad_(True) for q in w]
    h64 = None if h0 is None else h0.double().requires_grad_(True)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)               # thousands of tiny float64 products: a thread team only adds hand-over time to each
    try:
        o64, l64 = gru_layer(x.double(), *w64, h0=h64)
        loss = (o64 * dout.double()).sum() if want_out else 0.0
        if want_last:
            loss = loss + (l64 * dlast[0].double()).sum()
        loss.backward()
    finally:
        torch.set_num_threads(threads)
    wd = [q.to(DEV) for q in w]
    xd = x.to(DEV)
    out, last, dims, ws = ops.gru_forward(xd, wd, None if h0 is None else h0.to(DEV), want_out, want_last, save=True)
    grads, dh0 = ops.gru_backward(dims, xd, wd, None if dout is None else dout.to(DEV), None if dlast is None else dlast.to(DEV), ws,
                                  want_dh0=use_h0)
    gaps = LAYER_GAP["long" if seq > 1000 else "short"]
    errs = {}
    assert (out is None) == (not want_out) and (last is None) == (not want_last)
    if want_out:
        errs["out"] = rel_err(out, o64)
    if want_last:
        errs["h_last"] = rel_err(last[0], l64)
    for name, a, r in zip(("dW_ih", "dW_hh", "db_ih", "db_hh"), grads, w64):
        errs[name] = rel_err(a, r.grad)
    if use_h0:
        errs["dh0"] = rel_err(dh0[0], h64.grad[0])
    print({k: f"{v:.2e} / {bar(gaps[k]):.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= bar(gaps[k]), (k, v, bar(gaps[k]))
    # the eval-mode forward (nothing saved) gives the same bits
    out2, last2, _, _ = ops.gru_forward(xd, wd, None if h0 is None else h0.to(DEV), want_out, want_last, save=False)
    assert (not want_out or torch.equal(out, out2)) and (not want_last or torch.equal(last, last2))


def test_strided_input_is_read_in_place():
    from regtgcn_amd import ops
    gen = torch.Generator().manual_seed(5)
    ref = torch.nn.GRU(6, 256)
    wd = [q.detach().to(DEV) for q in ref.parameters()]
    base = torch.randn(8, 11, 20, generator=gen).to(DEV)
    x = base.permute(1, 0, 2)[:, :, 3:15:2]                                 # (11, 8, 6), no stride is the contiguous one
    assert not x.is_contiguous()
    dout = torch.randn(11, 8, 256, generator=gen).to(DEV)
    o1, l1, d1, ws1 = ops.gru_forward(x, wd)
    o2, l2, d2, ws2 = ops.gru_forward(x.contiguous(), wd)
    assert (d1.x_stride_seq, d1.x_stride_row, d1.x_stride_t) == (20, 220, 2)
    assert torch.equal(o1, o2) and torch.equal(l1, l2)
    g1, _ = ops.gru_backward(d1, x, wd, dout, None, ws1)
    g2, _ = ops.gru_backward(d2, x.contiguous(), wd, dout, None, ws2)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


@pytest.mark.parametrize("o", [1, 3, 64])
def test_model_output_widths(o):
    import regtgcn_amd as R
    torch.manual_seed(o)
    mod = R.StackedGRU(6, 8, 6, o).to(DEV)
    x = torch.randn(21, 9, 6)
    dy = torch.randn(21, 9, o)
    out = mod(x.to(DEV))
    (out * dy.to(DEV)).sum().backward()
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mod.state_dict().items()}
    o64 = stacked_gru(p64, x)
    (o64 * dy.double()).sum().backward()
    assert tuple(out.shape) == (21, 9, o) and rel_err(out, o64) <= bar(OUT_GAP_ANY)
    for k, p in mod.named_parameters():
        assert rel_err(p.grad, p64[k].grad) <= bar(GRAD_GAP_ANY[k]), k


def test_backward_is_bit_identical_across_runs():
    import regtgcn_amd as R
    torch.manual_seed(3)
    mod = R.StackedGRU(12, 8, 12, 3).to(DEV)
    x, dy = torch.randn(300, 24, 12, device=DEV), torch.randn(300, 24, 3, device=DEV)
    runs = []
    for _ in range(2):
        mod.zero_grad()
        (mod(x) * dy).sum().backward()
        runs.append([p.grad.clone() for p in mod.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_accumulation_in_backward_gives_the_same_bits():
    """GRUFunction and MLPHeadFunction under set_grad_accumulation_in_backward: two backwards in turn (the first hands its gradient
    tensors over as ``.grad``, the second adds to them) leave the ``.grad`` autograd's own accumulation leaves.  Nine rows cross the
    8-row tile a workgroup owns, nine steps make a real recurrence."""
    import regtgcn_amd as R
    torch.manual_seed(7)
    mod = R.StackedGRU(6, 8, 6, 1).to(DEV)
    gen = torch.Generator().manual_seed(17)
    xs = [torch.randn(9, 9, 6, generator=gen).to(DEV) for _ in range(2)]
    assert not torch.equal(xs[0], xs[1])
    runs = {}
    for flag in (False, True):
        prev = R.functional.set_grad_accumulation_in_backward(flag)
        try:
            mod.zero_grad(set_to_none=True)
            for x in xs:
                mod(x).square().sum().backward()
        finally:
            R.functional.set_grad_accumulation_in_backward(prev)
        runs[flag] = {k: p.grad.clone() for k, p in mod.named_parameters()}
    assert list(runs[True]) == KEYS and len(KEYS) == 12
    for k in KEYS:
        assert float(runs[False][k].abs().max()) > 0 and torch.equal(runs[True][k], runs[False][k]), k


@pytest.mark.parametrize("snap_batch", [4, 64])
def test_snap_batch_equals_sequential_calls(snap_batch):
    import regtgcn_amd as R
    from regtgcn_amd.evaluate import predict_metrics_gru
    from regtgcn_amd.train import WindowStore, evaluate_gru, train_epoch_gru
    gen = torch.Generator().manual_seed(11)
    s, n, t, o = 70, 13, 6, 3                                               # 70 snapshots: the last batch is short
    xs = [torch.rand(n, 8, t, generator=gen).to(DEV) for _ in range(s)]
    ys = [torch.rand(n, o, generator=gen).to(DEV) for _ in range(s)]
    store = WindowStore(xs, ys)
    torch.manual_seed(1)
    ref = R.StackedGRU(t, 8, t, o).to(DEV)
    init = {k: v.clone() for k, v in ref.state_dict().items()}
    res = {}
    for b in (1, snap_batch):
        mod = R.StackedGRU(t, 8, t, o).to(DEV)
        mod.load_state_dict(init)
        opt = torch.optim.SGD(mod.parameters(), lr=1.0)                     # the step is minus the accumulated gradient
        last, losses = train_epoch_gru(mod, store, opt, b)
        grads = {k: init[k] - v for k, v in mod.state_dict().items()}
        mod.load_state_dict(init)
        res[b] = (torch.stack(losses), grads, evaluate_gru(mod, store, b), predict_metrics_gru(mod, xs, ys, b))
    l1, g1, e1, m1 = res[1]
    lb, gb, eb, mb = res[snap_batch]
    assert len(l1) == len(lb) == s
    # rows are independent and every row runs the same instructions: the per-snapshot losses agree to fp32 rounding of the mean; the
    # accumulated gradients are sums of s terms in another grouping
    assert rel_err(lb, l1) <= bar(OUT_GAP_ANY)
    for k in KEYS:
        assert rel_err(gb[k], g1[k]) <= bar(GRAD_GAP_ANY[k]), k
    np.testing.assert_allclose(eb, e1, rtol=bar(OUT_GAP_ANY))
    np.testing.assert_allclose(mb, m1, rtol=bar(OUT_GAP_ANY))


def test_train_and_evaluate_command_lines(tmp_path):
    """The commands end to end on the fixture; --snap_batch 1 and 64 print the same epoch lines within the bars.  The lines are
    read at 12 decimals (--loss_digits).  Epoch 0's loss comes before any optimizer step; epoch 1's and the test metrics follow an
    RMSprop step whose ill-conditioned elements are those with a vanishing gradient, which move the loss by their gradient times
    their step: far below the bar.  The loss and the printed mean squared error are squares of the error (2 x the output's bar,
    see test_eval_golden_and_metrics), the RMSE is linear in it."""
    fx = os.path.join(ROOT, "tests", "golden", "tpims_fixture.npz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    epochs = {}
    for b in ("1", "64"):
        cmd = [sys.executable, "-m", "regtgcn_amd.train", "--model", "StackedGRU", "--num_timesteps_in", "6", "--num_timesteps_out", "1",
               "--tr", "0.2", "--tf", "occrate", "--fixture", fx, "--epochs", "1", "--snap_batch", b, "--out_dir", str(tmp_path / b),
               "--loss_digits", "12"]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("Train Loss:")]
        assert len(lines) == 2 and all("nan" not in l and "inf" not in l for l in lines)
        epochs[b] = [[float(f.split(":")[1]) for f in l.split(",")] for l in lines]          # [loss, rmse, mse] per epoch
    print(epochs)
    bo = bar(OUT_GAP["in6_out1"])
    for e1, e64 in zip(epochs["1"], epochs["64"]):
        assert abs(e1[0] - e64[0]) <= 2 * bo * e1[0] and abs(e1[1] - e64[1]) <= bo * e1[1] and abs(e1[2] - e64[2]) <= 2 * bo * e1[2], epochs
    ck = os.path.join(tmp_path, "64", "occrate", "StackedGRU", "model_in6_out1_epoch0.pt")
    assert os.path.exists(ck)
    r = subprocess.run([sys.executable, "-m", "regtgcn_amd.evaluate", "--model", "StackedGRU", "--fixture", fx, "--checkpoint", ck,
                        "--num_timesteps_in", "6", "--num_timesteps_out", "1", "--tr", "0.2", "--snap_batch", "8"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1].startswith("MAE:")
