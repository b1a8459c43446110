"""STID on the GPU: the reference module's goldens (training forward / backward with the keep mask the reference drew, eval with
the metrics, a three-window RMSprop trajectory), the kernels against the float64 restatement over lengths, feature counts, output
lengths, node counts, batch sizes, depths and the node-embedding switch, the module's own dropout draw, bit-reproducible
gradients, snapshot batching and the command lines.

Tolerances, all absolute.  Against the reference goldens: 1e-5 + GRAD_GAP on outputs, losses and gradients (GRAD_GAP is the
fp32-vs-float64 gap of the restatement on the goldens, tests/test_stid_cpu.py) and 1e-3 on MAPE, which predict.py scales by 100.
After the RMSprop step: the bound of test_three_window_trajectory_matches_reference_golden.  Against the float64 restatement:
1e-5 + K_GAP x the fp32-vs-float64 gap of the same restatement evaluated in fp32 on the same inputs, per tensor, with
K_GAP = 4 as for STNorm: torch sums in pairwise blocks, the kernels add a tile's 64 nodes in sequence on the matrix unit, then a
workgroup's tiles in sequence, then the workgroups in sequence."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_npz
from stid_math import stid, unpack_keep
from test_stid_cpu import GRAD_GAP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["in6_out1", "in12_out3"]
DEV = "cuda:0"
K_GAP = 4
TILE = 64                     # nodes per tile of csrc/stid.hip
OFF = dict(if_time_in_day=False, if_day_in_week=False)


def _golden(tag):
    g = load_npz(f"golden_stid_{tag}.npz")
    return g, [str(k) for k in g["state_dict_keys"]]


def _module(g, keys):
    import regtgcn_amd as R
    mod = R.STID(num_nodes=g["x"].shape[2], input_len=int(g["t_in"]), output_len=int(g["t_out"]), **OFF)
    mod.load_state_dict({k: torch.from_numpy(g[f"p__{k}"]) for k in keys})
    return mod.to(DEV)


def _close(a, b, atol=1e-5, rtol=0.0, what=""):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    print(f"{what or 'value'}: max |diff| {float(np.abs(a - b).max()):.3g} (bound {atol:.3g})")
    np.testing.assert_allclose(a, b, atol=atol, rtol=rtol, err_msg=what)


@pytest.mark.parametrize("tag", TAGS)
def test_train_mode_matches_reference_golden(tag):
    g, keys = _golden(tag)
    mod = _module(g, keys).train()
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    out = mod(x, keep=torch.from_numpy(g["train__keep"]).to(DEV))
    loss = torch.mean((out - y) ** 2)
    loss.backward()
    _close(out, g["train__out"], atol=1e-5 + GRAD_GAP, what="out")
    _close(loss, g["train__loss"][0], atol=1e-5 + GRAD_GAP, what="loss")
    for k, p in mod.named_parameters():
        assert p.grad is not None, k
        _close(p.grad, g[f"train__g__{k}"], atol=1e-5 + GRAD_GAP, what=k)


@pytest.mark.parametrize("tag", TAGS)
def test_eval_mode_and_metrics_match_reference_golden(tag):
    from regtgcn_amd.evaluate import predict_metrics_stid
    g, keys = _golden(tag)
    mod = _module(g, keys).eval()
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    with torch.no_grad():
        out = mod(x)
    _close(out, g["eval__out"], atol=1e-5 + GRAD_GAP, what="eval out")
    _close(((out[0][0] - y) ** 2).mean(), g["eval__test_mse"][0], atol=1e-5 + GRAD_GAP)
    xs = [torch.from_numpy(g["x"][0]).permute(1, 2, 0).to(DEV)]              # back to the (N, F, T) snapshot
    mae, rmse, mape = predict_metrics_stid(mod, xs, [y])
    _close(mae, g["eval__mae"][0], atol=1e-5 + GRAD_GAP)
    _close(rmse, np.sqrt(g["eval__mse"][0]), atol=1e-5 + GRAD_GAP)
    _close(mape, g["eval__mape"][0], atol=1e-3)


@pytest.mark.parametrize("tag", TAGS)
def test_three_window_trajectory_matches_reference_golden(tag, tpims):
    from regtgcn_amd import functional as F_
    g, keys = _golden(tag)
    mod = _module(g, keys).train()
    t_in, t_out, w = int(g["t_in"]), int(g["t_out"]), int(g["window"])
    opt = torch.optim.RMSprop(mod.parameters(), lr=1e-3, weight_decay=1e-4)
    losses = []
    prev = F_.set_grad_accumulation_in_backward(True)
    try:
        for k in range(3):
            x = tpims["node_data"][:, :, w + k:w + k + t_in].permute(2, 0, 1).unsqueeze(0).contiguous().to(DEV)
            y = tpims["node_data"][:, -1, w + k + t_in:w + k + t_in + t_out].contiguous().to(DEV)
            loss = torch.mean((mod(x, keep=torch.from_numpy(g["traj__keep"][k]).to(DEV)) - y) ** 2)
            loss.backward()
            losses.append(float(loss.detach()))
    finally:
        F_.set_grad_accumulation_in_backward(prev)
    opt.step()
    _close(losses, g["traj__loss"], atol=1e-5 + GRAD_GAP, what="losses")
    # RMSprop's first step is -lr g' / (sqrt(0.01 g'^2) + 1e-8), g' = g + wd p: where g' is tiny it amplifies a gradient error dg by
    # lr 1e-8 / (0.1 |g'| + 1e-8)^2.  The bound per element takes g' from the float64 restatement and dg = GRAD_GAP, the largest
    # fp32-vs-float64 gradient gap of the restatement on the goldens (tests/test_stid_cpu.py)
    ref = {k: torch.from_numpy(g[f"p__{k}"]).double().requires_grad_(True) for k in keys}
    for k in range(3):
        x = tpims["node_data"][:, :, w + k:w + k + t_in].permute(2, 0, 1).unsqueeze(0).contiguous()
        y = tpims["node_data"][:, -1, w + k + t_in:w + k + t_in + t_out].double()
        ro = stid(ref, x, 3, keep=unpack_keep(torch.from_numpy(g["traj__keep"][k])))
        torch.mean((ro - y) ** 2).backward()
    # the golden stores the step as an fp16 delta: half an fp16 ulp of each stored value joins the bound
    for k, p in mod.named_parameters():
        dp = g[f"traj__dp__{k}"]
        half_ulp = np.spacing(np.abs(dp)).astype(np.float64) / 2
        target = g[f"p__{k}"].astype(np.float64) + dp.astype(np.float64)
        err = np.abs(p.detach().cpu().double().numpy() - target)
        gp = (ref[k].grad + 1e-4 * ref[k].detach()).abs().numpy()
        bound = 1e-5 + half_ulp + 1e-3 * 1e-8 * GRAD_GAP / (0.1 * gp + 1e-8) ** 2
        print(f"{k}: max step error {float(err.max()):.3g}, max excess over bound {float((err - bound).max()):.3g}")
        assert (err <= bound).all(), (k, float(err.max()))


def _random_biases(mod, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith("bias"):
                p.copy_((torch.rand(p.shape, generator=gen) - 0.5) * 0.4)


def _against_restatement(n, b=1, l=6, c=8, d=3, o=1, nl=3, if_node=True, seed=0, training=True):
    import regtgcn_amd as R
    torch.manual_seed(seed)
    mod = R.STID(num_nodes=n, input_len=l, output_len=o, input_dim=d, num_layer=nl, if_node=if_node, **OFF)
    _random_biases(mod, seed)
    ref = {k: v.detach().clone().double().requires_grad_(True) for k, v in mod.state_dict().items()}
    x = torch.randn(b, l, n, c, generator=torch.Generator().manual_seed(seed + 1))
    keep = (torch.rand(nl, b, n, mod.hidden_dim, generator=torch.Generator().manual_seed(seed + 3)) < 0.85) if training else None
    mod = mod.to(DEV).train(training)
    from stid_math import pack_keep
    out = mod(x.to(DEV), keep=None if keep is None else pack_keep(keep).to(DEV))
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed + 2))
    (out * w.to(DEV)).sum().backward()
    ro = stid(ref, x, d, keep=keep)
    (ro * w.double()).sum().backward()
    # the same restatement in fp32 gives the per-tensor gap of the bound (module docstring)
    r32 = {k: v.detach().float().requires_grad_(True) for k, v in ref.items()}
    o32 = stid(r32, x, d, keep=keep, dtype=torch.float32)
    (o32 * w).sum().backward()
    assert tuple(out.shape) == (b, o, n, 1) == tuple(ro.shape)
    _close(out, ro.detach(), atol=1e-5 + K_GAP * float((o32.detach().double() - ro.detach()).abs().max()), what="out")
    for k, p in mod.named_parameters():
        gap = float((r32[k].grad.double() - ref[k].grad).abs().max())
        _close(p.grad, ref[k].grad, atol=1e-5 + K_GAP * gap, what=k)
    return mod


@pytest.mark.parametrize("l", [1, 3, 6, 12, 24])
def test_kernels_match_restatement_over_input_lengths(l):
    _against_restatement(104, b=2, l=l, seed=l)


@pytest.mark.parametrize("d", [1, 3, 8])
def test_kernels_match_restatement_over_input_dims(d):
    _against_restatement(104, b=1, l=24 if d == 8 else 6, c=8, d=d, o=3, seed=10 + d)


@pytest.mark.parametrize("o", [1, 3, 12, 64])
def test_kernels_match_restatement_over_output_lengths(o):
    _against_restatement(130, b=1, l=6, o=o, seed=20 + o)


@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE + 1, 1000])
@pytest.mark.parametrize("b", [1, 3])
def test_small_and_ragged_node_counts(n, b):
    _against_restatement(n, b=b, l=12, o=3, seed=30 + n + b)


@pytest.mark.parametrize("nl", [1, 3, 8])
def test_depths(nl):
    _against_restatement(200, b=2, l=6, o=2, nl=nl, seed=40 + nl)


@pytest.mark.parametrize("nl", [1, 3, 8])
def test_without_node_embedding(nl):
    mod = _against_restatement(150, b=2, l=6, o=33, nl=nl, if_node=False, seed=50 + nl)
    assert "node_emb" not in mod.state_dict()


def test_eval_mode_against_restatement():
    _against_restatement(300, b=3, l=12, o=3, seed=60, training=False)


def test_module_draws_dropout_in_training_mode():
    """Two training calls differ; the recorded bits replay the first call bit for bit, forward and backward; eval ignores keep."""
    import regtgcn_amd as R
    from regtgcn_amd.nn import draw_stid_keep
    torch.manual_seed(0)
    mod = R.STID(num_nodes=500, input_len=6, output_len=2, **OFF).to(DEV).train()
    x = torch.randn(2, 6, 500, 8, device=DEV)
    out1 = mod(x)
    keep1 = mod.last_keep
    assert keep1.dtype == torch.int32 and tuple(keep1.shape) == (3, 2, 500, 2)
    (out1 ** 2).mean().backward()
    g1 = [p.grad.clone() for p in mod.parameters()]
    out2 = mod(x)
    assert not torch.equal(out1, out2) and not torch.equal(keep1, mod.last_keep)
    mod.zero_grad()
    out3 = mod(x, keep=keep1)
    (out3 ** 2).mean().backward()
    assert torch.equal(out1, out3)
    for a, p in zip(g1, mod.parameters()):
        assert torch.equal(a, p.grad)
    mod.eval()
    with torch.no_grad():
        assert torch.equal(mod(x), mod(x, keep=keep1))
    # the kept fraction: n Bernoulli(0.85) bits, a condition of 5 standard deviations
    bits = unpack_keep(draw_stid_keep(3, 4, 4096, 64, DEV))
    assert tuple(bits.shape) == (3, 4, 4096, 64)
    n = bits.numel()
    assert abs(float(bits.double().mean()) - 0.85) < 5 * (0.85 * 0.15 / n) ** 0.5
    top = bits[..., 31].double().mean(), bits[..., 63].double().mean()       # a word's top bit is as live as the others
    for t in top:
        assert abs(float(t) - 0.85) < 5 * (0.85 * 0.15 / (n // 64)) ** 0.5
    each = bits.reshape(-1, 64).double().mean(0)
    assert float((each - 0.85).abs().max()) < 6 * (0.85 * 0.15 / (n // 64)) ** 0.5


def test_host_module_or_wrong_dtype_is_refused_before_launch():
    import regtgcn_amd as R
    mod = R.STID(num_nodes=50, input_len=6, output_len=1, **OFF)
    x = torch.randn(1, 6, 50, 8, device=DEV)
    with pytest.raises(R.RegtError):
        mod(x)                                                   # parameters still on the host
    mod = mod.to(DEV)
    with pytest.raises(R.RegtError):
        mod(x.double())
    with pytest.raises(R.RegtError):
        mod.double()(x)
    mod = mod.float()
    with pytest.raises(ValueError):
        mod(x[:, :5])
    assert tuple(mod(x).shape) == (1, 1, 50, 1)


def test_backward_is_bit_reproducible():
    import regtgcn_amd as R
    torch.manual_seed(0)
    mod = R.STID(num_nodes=1000, input_len=12, output_len=3, **OFF).to(DEV).train()
    x = torch.randn(2, 12, 1000, 8, device=DEV)
    keep = None
    grads = []
    for _ in range(2):
        mod.zero_grad()
        (mod(x, keep=keep) ** 2).mean().backward()
        keep = mod.last_keep
        grads.append([p.grad.clone() for p in mod.parameters()])
    assert len(grads[0]) == 17
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_snapshot_batching_equals_sequential_calls():
    """(B, T, N, F) == B sequential calls with B = 1 when both get the same keep bits: losses and accumulated gradients."""
    import regtgcn_amd as R
    from regtgcn_amd.nn import draw_stid_keep
    from regtgcn_amd.train import WindowStore, train_epoch_stid
    torch.manual_seed(1)
    base = R.STID(num_nodes=104, input_len=6, output_len=2, **OFF)
    _random_biases(base, 1)
    xs = [torch.randn(104, 8, 6, device=DEV) for _ in range(8)]
    ys = [torch.randn(104, 2, device=DEV) for _ in range(8)]
    keeps = draw_stid_keep(3, 8, 104, 64, DEV)
    res = []
    for sb in (1, 4):
        mod = R.STID(num_nodes=104, input_len=6, output_len=2, **OFF)
        mod.load_state_dict(base.state_dict())
        mod = mod.to(DEV)
        opt = torch.optim.SGD(mod.parameters(), lr=0.0)
        grads = {}
        orig = opt.step

        def step(orig=orig, mod=mod, grads=grads):
            grads.update({k: p.grad.clone() for k, p in mod.named_parameters() if p.grad is not None})
            return orig()
        opt.step = step
        _, losses = train_epoch_stid(mod, WindowStore(xs, ys), opt, sb, keeps=keeps)
        res.append((torch.stack(losses), grads))
    assert len(res[0][1]) == 17
    _close(res[0][0], res[1][0].cpu(), atol=1e-6, what="losses")
    for k in res[0][1]:
        _close(res[0][1][k], res[1][1][k].cpu(), atol=1e-5, what=k)


def test_cfg3_shape_against_restatement():
    """The cfg-3 shape: N = 100 000 nodes, C = 8, L = 12, O = 1 (forward and gradients; the weight gradients sum 100 000 nodes)."""
    _against_restatement(100_000, b=1, l=12, c=8, d=3, o=1, seed=9)


@pytest.mark.parametrize("t_out", [1, 3])
def test_train_and_evaluate_command_lines(tmp_path, t_out):
    fx = os.path.join(ROOT, "tests", "golden", "tpims_fixture.npz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "regtgcn_amd.train", "--model", "STID", "--num_timesteps_in", "6", "--num_timesteps_out", str(t_out),
           "--tr", "0.2", "--tf", "occrate", "--fixture", fx, "--epochs", "1", "--snap_batch", "16", "--out_dir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("Train Loss:")]
    assert len(lines) == 2 and all("nan" not in l and "inf" not in l for l in lines)
    ck = os.path.join(tmp_path, "occrate", "STID", f"model_in6_out{t_out}_epoch0.pt")
    assert os.path.exists(ck)
    r = subprocess.run([sys.executable, "-m", "regtgcn_amd.evaluate", "--model", "STID", "--fixture", fx, "--checkpoint", ck,
                        "--num_timesteps_in", "6", "--num_timesteps_out", str(t_out), "--tr", "0.2", "--snap_batch", "8"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1].startswith("MAE:")
