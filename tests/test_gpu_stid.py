"""STID on the GPU: the reference module's goldens (training forward / backward with the keep mask the reference drew, eval with
the metrics, a three-window RMSprop trajectory), the kernels against the float64 restatement over lengths, feature counts, output
lengths, node counts, batch sizes, depths and the node-embedding switch, the module's own dropout draw, bit-reproducible
gradients, snapshot batching and the command lines.

Tolerances, all absolute.  Against the reference goldens: 1e-5 + GRAD_GAP on outputs, losses and gradients (GRAD_GAP is the
fp32-vs-float64 gap of the restatement on the goldens, tests/test_stid_cpu.py) and 1e-3 on MAPE, which predict.py scales by 100.
After the RMSprop step: the bound of test_three_window_trajectory_matches_reference_golden.  Against the float64 restatement:
1e-5 + K_GAP x the fp32-vs-float64 gap of the same restatement evaluated in fp32 on the same inputs, per tensor, with
K_GAP = 4 as for STNorm: torch sums in pairwise blocks, the kernels add a tile's 64 nodes in sequence on the matrix unit, then a
workgroup's tiles in sequence, then the workgroups in sequence.

Next to every one of these gradient comparisons stands grad_bars.assert_grads_conditioned: every block (node_emb by 64-node
tile, the ragged last tile on its own; the embedding weight by input step; the 64 x 64 weights by wave quadrant) against the
float64 restatement at a bar relative to the block's OWN scale; no block of these cases is ill-conditioned.  The restatements
run once per case on the host and serve both assertions."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_npz
from grad_bars import REL, assert_grads_conditioned
from stid_math import pack_keep, stid, unpack_keep
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


def _restated_grads(params, x, input_dim, keep, loss, dtype):
    """({name: gradient}, output) of the restatement in `dtype`; `loss(out)` -> scalar."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    out = stid(p, x, input_dim, keep=keep, dtype=dtype)
    loss(out).backward()
    return {k: v.grad for k, v in p.items()}, out.detach()


def golden_case(tag):
    """The float64 and fp32 restatement gradients of the golden's training step (its parameters, input, keep mask and loss)."""
    g, keys = _golden(tag)
    params = {k: torch.from_numpy(g[f"p__{k}"]) for k in keys}
    x, y, keep = torch.from_numpy(g["x"]), torch.from_numpy(g["y"]), unpack_keep(torch.from_numpy(g["train__keep"]))
    g64, _ = _restated_grads(params, x, 3, keep, lambda o: torch.mean((o - y.double()) ** 2), torch.float64)
    g32, _ = _restated_grads(params, x, 3, keep, lambda o: torch.mean((o - y) ** 2), torch.float32)
    return g64, g32


def _hip_grads(mod):
    return {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in mod.named_parameters()}


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
    g64, g32 = golden_case(tag)
    ill, _ = assert_grads_conditioned(_hip_grads(mod), g64, g32, K_GAP, REL, f"golden {tag}", input_dim=3)
    assert ill == []


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


def restatement_case(n, b=1, l=6, c=8, d=3, o=1, nl=3, if_node=True, seed=0, training=True):
    """What the host alone computes of one comparison: the module with its parameters, the input, the keep mask, the loss weights,
    and the restatement's output and gradients in float64 and in fp32 (computed once, shared by every assertion)."""
    import regtgcn_amd as R
    torch.manual_seed(seed)
    mod = R.STID(num_nodes=n, input_len=l, output_len=o, input_dim=d, num_layer=nl, if_node=if_node, **OFF)
    _random_biases(mod, seed)
    sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    x = torch.randn(b, l, n, c, generator=torch.Generator().manual_seed(seed + 1))
    keep = (torch.rand(nl, b, n, mod.hidden_dim, generator=torch.Generator().manual_seed(seed + 3)) < 0.85) if training else None
    w = torch.randn(b, o, n, 1, generator=torch.Generator().manual_seed(seed + 2))
    g64, ro = _restated_grads(sd, x, d, keep, lambda out: (out * w.double()).sum(), torch.float64)
    # the same restatement in fp32 gives the per-tensor gap of the bound (module docstring)
    g32, o32 = _restated_grads(sd, x, d, keep, lambda out: (out * w).sum(), torch.float32)
    return dict(mod=mod, x=x, keep=keep, w=w, ro=ro, o32=o32, g64=g64, g32=g32, input_dim=d)


def _against_restatement(n, b=1, l=6, c=8, d=3, o=1, nl=3, if_node=True, seed=0, training=True, ill_share=0.0):
    case = restatement_case(n, b, l, c, d, o, nl, if_node, seed, training)
    x, keep, w, ro, o32, g64, g32 = (case[k] for k in ("x", "keep", "w", "ro", "o32", "g64", "g32"))
    mod = case["mod"].to(DEV).train(training)
    out = mod(x.to(DEV), keep=None if keep is None else pack_keep(keep).to(DEV))
    (out * w.to(DEV)).sum().backward()
    assert tuple(out.shape) == (b, o, n, 1) == tuple(ro.shape)
    _close(out, ro, atol=1e-5 + K_GAP * float((o32.double() - ro).abs().max()), what="out")
    for k, p in mod.named_parameters():
        gap = float((g32[k].double() - g64[k]).abs().max())
        _close(p.grad, g64[k], atol=1e-5 + K_GAP * gap, what=k)
    ill, nblocks = assert_grads_conditioned(_hip_grads(mod), g64, g32, K_GAP, REL, f"n {n} b {b} l {l} d {d} o {o} nl {nl} node {if_node}",
                                            input_dim=d)
    assert len(ill) <= ill_share * nblocks, ill
    return mod


def _node_count_seed(n, b):
    """30 + n + b, but for (1000, 3): under seed 1033 one fc1 pre-activation of the last layer lies within fp32 rounding of zero, the
    fp32 restatement takes its ReLU the other way than float64 and 37 of the 62 gradient blocks move by up to 7e-3 of their scale
    (tests/test_baseline_bars_cpu.py shows the ill-conditioned list): a comparison of two ReLU decisions, not of gradients."""
    return 2033 if (n, b) == (1000, 3) else 30 + n + b


# every comparison against the restatement that the tests below run (tests/test_baseline_bars_cpu.py proves the bars on them)
RESTATEMENT_CASES = ([dict(n=104, b=2, l=l, seed=l) for l in (1, 3, 6, 12, 24)] +
                     [dict(n=104, b=1, l=24 if d == 8 else 6, c=8, d=d, o=3, seed=10 + d) for d in (1, 3, 8)] +
                     [dict(n=130, b=1, l=6, o=o, seed=20 + o) for o in (1, 3, 12, 64)] +
                     [dict(n=n, b=b, l=12, o=3, seed=_node_count_seed(n, b)) for b in (1, 3) for n in (1, 2, TILE - 1, TILE + 1, 1000)] +
                     [dict(n=200, b=2, l=6, o=2, nl=nl, seed=40 + nl) for nl in (1, 3, 8)] +
                     [dict(n=150, b=2, l=6, o=33, nl=nl, if_node=False, seed=50 + nl) for nl in (1, 3, 8)] +
                     [dict(n=300, b=3, l=12, o=3, seed=60, training=False)])
CFG3_CASE = dict(n=100_000, b=1, l=12, c=8, d=3, o=1, seed=9)
# Among the cfg-3 shape's 19 million fc1 pre-activations one lies within fp32 rounding of zero: the fp32 restatement takes that ReLU
# the other way than float64, and the blocks it reaches (17 of 1609: one node_emb tile, the embedding and first-layer weights) are
# ill-conditioned (tests/grad_bars.py), held to K_GAP x their fp32 gap.  Other seeds move the coin to the kernels' side instead.
CFG3_ILL_SHARE = 0.05


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
    _against_restatement(n, b=b, l=12, o=3, seed=_node_count_seed(n, b))


def test_relu_within_rounding_of_zero_keeps_its_absolute_bar():
    """Seed 1033 of the (1000, 3) case (see _node_count_seed): the fp32 restatement and float64 disagree on one ReLU.  The absolute
    bars built on the fp32 gap hold as they did; the blocks that decision reaches are ill-conditioned and held to K_GAP x their gap."""
    _against_restatement(1000, b=3, l=12, o=3, seed=1033, ill_share=1.0)


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


def snapshot_batching_case():
    """The module, eight snapshots (N, F, T) with targets (N, O) and keep bits, and the restatement's accumulated gradients of
    train_epoch_stid on them: the sum over the snapshots of each one's mean-squared loss."""
    import regtgcn_amd as R
    torch.manual_seed(1)
    base = R.STID(num_nodes=104, input_len=6, output_len=2, **OFF)
    _random_biases(base, 1)
    gen = torch.Generator().manual_seed(11)
    xs = [torch.randn(104, 8, 6, generator=gen) for _ in range(8)]
    ys = [torch.randn(104, 2, generator=gen) for _ in range(8)]
    keep = torch.rand(3, 8, 104, 64, generator=gen) < 0.85
    x, y = torch.stack(xs).permute(0, 3, 1, 2), torch.stack(ys)               # (8, T, N, F), (8, N, O)
    loss = lambda out: ((out - y.to(out.dtype).unsqueeze(1)) ** 2).mean(dim=(1, 2, 3)).sum()
    sd = {k: v.detach().clone() for k, v in base.state_dict().items()}
    g64, _ = _restated_grads(sd, x, 3, keep, loss, torch.float64)
    g32, _ = _restated_grads(sd, x, 3, keep, loss, torch.float32)
    return base, xs, ys, pack_keep(keep), g64, g32


def test_snapshot_batching_equals_sequential_calls():
    """(B, T, N, F) == B sequential calls with B = 1 when both get the same keep bits: losses and accumulated gradients."""
    import regtgcn_amd as R
    from regtgcn_amd.train import WindowStore, train_epoch_stid
    base, xs, ys, keeps, g64, g32 = snapshot_batching_case()
    xs, ys, keeps = [x.to(DEV) for x in xs], [y.to(DEV) for y in ys], keeps.to(DEV)
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
    for sb, (_l, grads) in zip((1, 4), res):
        ill, _ = assert_grads_conditioned(grads, g64, g32, K_GAP, REL, f"snapshot batch {sb}", input_dim=3)
        assert ill == []


def test_cfg3_shape_against_restatement():
    """The cfg-3 shape: N = 100 000 nodes, C = 8, L = 12, O = 1 (forward and gradients; the weight gradients sum 100 000 nodes)."""
    _against_restatement(**CFG3_CASE, ill_share=CFG3_ILL_SHARE)


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
