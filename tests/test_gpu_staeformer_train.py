"""Whole-STAEformer training on the GPU: keep-bit dropout folded into add+LayerNorm, the embedding and output-projection gradients,
nn.STAEformerTrainable against the float64 restatement (tests/staeformer_train_math.py), train.train_epoch_staeformer and the
train_staeformer / evaluate command lines.  Bars: tests/staeformer_train_bars.py (those of grad_bars.py)."""
import os
import subprocess
import sys

import pytest
import torch

import regtgcn_amd as R
from regtgcn_amd import functional as F_, ops
import staeformer_train_bars as TB
import staeformer_train_math as TM
from staeformer_math import embed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV, SENT = TB.DEV, TB.SENTINEL


# ---- drop-add-LayerNorm ---------------------------------------------------------------------------------------------------------

def _ln_case(m, d, seed=0):
    gen = torch.Generator().manual_seed(13 * m + d + seed)
    res, y, dout = (torch.randn(m, d, generator=gen) for _ in range(3))
    gamma = 1.0 + 0.5 * (torch.rand(d, generator=gen) - 0.5)
    beta = 0.4 * (torch.rand(d, generator=gen) - 0.5)
    keep = TM.pack_keep(torch.rand(m, d, generator=gen) >= TB.LN_P)
    return res, y, gamma, beta, dout, keep


def _ln_oracle(res, y, gamma, beta, dout, keep, p, dtype):
    mask = TM.unpack_keep(keep, res.shape[1])
    r, yy, g, b = (z.detach().to(dtype).requires_grad_(True) for z in (res, y, gamma, beta))
    out = TM.drop_add_layernorm(r, yy, mask, p, g, b, dtype=dtype)
    dz, dy, dg, db = torch.autograd.grad(out, (r, yy, g, b), dout.to(dtype))
    return out.detach(), {"dz": dz, "dy": dy, "dgamma": dg, "dbeta": db}


@pytest.mark.parametrize("m", TB.LN_M)
@pytest.mark.parametrize("d", TB.LN_D)
def test_drop_add_layernorm_against_float64(m, d):
    res, y, gamma, beta, dout, keep = _ln_case(m, d)
    o64, g64 = _ln_oracle(res, y, gamma, beta, dout, keep, TB.LN_P, torch.float64)
    o32, g32 = _ln_oracle(res, y, gamma, beta, dout, keep, TB.LN_P, torch.float32)
    c = [z.to(DEV) for z in (res, y, gamma, beta, dout, keep)]
    out = ops.stae_drop_add_layernorm(c[0], c[1], c[5], TB.LN_P, c[2], c[3])
    runs = [ops.stae_drop_add_layernorm_backward(c[0], c[1], c[5], TB.LN_P, c[2], c[4]) for _ in range(2)]
    torch.cuda.synchronize()
    TB.forward_bar(out, o64, o32, f"drop_add_layernorm forward M {m} D {d}")
    got = dict(zip(("dz", "dy", "dgamma", "dbeta"), runs[0]))
    TB.assert_blocks(got, g64, g32, f"drop LN backward M {m} D {d}", d)
    mask = TM.unpack_keep(keep, d)
    assert bool((got["dy"].cpu()[~mask] == 0).all())                          # a dropped column gets exactly 0
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])), "two runs differ"


@pytest.mark.parametrize("m,d", [(17, 32), (65, 128), (16, 256)])
def test_drop_add_layernorm_special_keeps_and_windows(m, d):
    res, y, gamma, beta, dout, _ = (z.to(DEV) for z in _ln_case(m, d, seed=5))
    plain = ops.stae_add_layernorm(res, y, gamma, beta)
    pdz, pdg, pdb = ops.stae_add_layernorm_backward(res, y, gamma, dout)
    ones = torch.full((m, d // 32), -1, dtype=torch.int32, device=DEV)
    zeros = torch.zeros(m, d // 32, dtype=torch.int32, device=DEV)
    top = torch.full((m, d // 32), -2 ** 31, dtype=torch.int32, device=DEV)
    for keep, p in ((None, 0.3), (ones, 0.0)):                                 # the bits of the existing entries
        assert torch.equal(ops.stae_drop_add_layernorm(res, y, keep, p, gamma, beta), plain)
        dz, dy, dg, db = ops.stae_drop_add_layernorm_backward(res, y, keep, p, gamma, dout)
        assert torch.equal(dz, pdz) and torch.equal(dy, pdz) and torch.equal(dg, pdg) and torch.equal(db, pdb)
    out0 = ops.stae_drop_add_layernorm(res, y, zeros, 0.1, gamma, beta)
    assert torch.equal(out0, ops.stae_add_layernorm(res, torch.zeros_like(y), gamma, beta))
    dz0, dy0, _, _ = ops.stae_drop_add_layernorm_backward(res, y, zeros, 0.1, gamma, dout)
    assert bool((dy0 == 0).all()) and torch.equal(dz0, ops.stae_add_layernorm_backward(res, torch.zeros_like(y), gamma, dout)[0])
    # only bit 31 of each word: column 32 w + 31 alone is kept
    mask = torch.zeros(m, d, dtype=torch.bool)
    mask[:, 31::32] = True
    assert torch.equal(TM.pack_keep(mask), top.cpu())
    o64 = TM.drop_add_layernorm(res.cpu(), y.cpu(), mask, 0.1, gamma.cpu(), beta.cpu())
    o32 = TM.drop_add_layernorm(res.cpu(), y.cpu(), mask, 0.1, gamma.cpu(), beta.cpu(), dtype=torch.float32)
    TB.forward_bar(ops.stae_drop_add_layernorm(res, y, top, 0.1, gamma, beta), o64, o32, f"bit 31 keep M {m} D {d}")
    _, dyt, _, _ = ops.stae_drop_add_layernorm_backward(res, y, top, 0.1, gamma, dout)
    assert bool((dyt.cpu()[~mask] == 0).all()) and bool((dyt.cpu()[mask] != 0).any())
    # sentinel-filled buffers around the outputs: the raw entry writes its windows only
    lib = R.load_library()
    pad = 64
    bufs = {k: torch.full((n + 2 * pad,), SENT, device=DEV) for k, n in (("out", m * d), ("dz", m * d), ("dy", m * d), ("dg", d), ("db", d))}
    win = {k: v[pad:v.numel() - pad] for k, v in bufs.items()}
    keep = TM.pack_keep(torch.rand(m, d, generator=torch.Generator().manual_seed(1)) >= 0.1).to(DEV)
    scratch = torch.empty(lib.regt_stae_drop_add_layernorm_backward_scratch_floats(m, d), device=DEV)
    P = R._lib.ptr
    s = torch.cuda.current_stream().cuda_stream
    R._lib.check(lib.regt_stae_drop_add_layernorm(P(res), P(y), P(keep), 0.1, P(gamma), P(beta), 1e-5, m, d, P(win["out"]), s), "forward")
    R._lib.check(lib.regt_stae_drop_add_layernorm_backward(P(res), P(y), P(keep), 0.1, P(gamma), P(dout), 1e-5, m, d, P(win["dz"]), P(win["dy"]),
                                                           P(win["dg"]), P(win["db"]), P(scratch), s), "backward")
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v[:pad] == SENT).all()) and bool((v[-pad:] == SENT).all()), k
        assert bool(torch.isfinite(win[k]).all()) and not bool((win[k] == SENT).any()), k
    assert torch.equal(win["out"].view(m, d), ops.stae_drop_add_layernorm(res, y, keep, 0.1, gamma, beta))


# ---- embedding ------------------------------------------------------------------------------------------------------------------

def _embed_case(shape, widths, cin=TB.EMBED_CIN):
    (b, t, n), (e, tod, dow, s, a) = shape, widths
    kw = dict(num_nodes=n, in_steps=t, out_steps=1, input_embedding_dim=e, tod_embedding_dim=tod, dow_embedding_dim=dow, spatial_embedding_dim=s,
              adaptive_embedding_dim=a, steps_per_day=TB.EMBED_SPD, num_heads=(e + tod + dow + s + a) // 32, num_layers=1, feed_forward_dim=32,
              input_dim=cin)
    shapes, d = TB.state_shapes(kw)
    sd = {k: v for k, v in TB.model_state(shapes[:[k for k, _ in shapes].index("output_proj.weight")], seed=21).items()}
    gen = torch.Generator().manual_seed(50 + b + t + n + e)
    x = TB.features(b, t, n, TB.EMBED_F, gen, TB.EMBED_SPD, wild=True, nan=cin == 1)
    dx0 = torch.randn(b * t * n, d, generator=gen)
    dims = R._lib.StaeDims(b, t, n, TB.EMBED_F, cin, e, tod, dow, s, a, TB.EMBED_SPD, TB.EMBED_DPW, d // 32, 32, 1, 1, 1, 1, 1e-5)
    return dims, sd, x, dx0, d


def _embed_oracle(sd, x, dx0, dtype):
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    out = embed(p, x, dtype, clamp=True)
    grads = torch.autograd.grad(out, list(p.values()), dx0.view(out.shape).to(dtype))
    return out.detach(), dict(zip(p, grads))


# input_dim = 1 keeps the NaN entries of the two index columns out of the input projection, where they would poison every reference
@pytest.mark.parametrize("shape,widths,cin", [(s_, w_, TB.EMBED_CIN) for s_ in TB.EMBED_SHAPES for w_ in TB.EMBED_WIDTHS] +
                         [(s_, w_, 1) for s_ in TB.EMBED_SHAPES for w_ in TB.EMBED_WIDTHS[:2]])
def test_embed_forward_and_backward(shape, widths, cin):
    dims, sd, x, dx0, d = _embed_case(shape, widths, cin)
    o64, g64 = _embed_oracle(sd, x, dx0, torch.float64)
    o32, g32 = _embed_oracle(sd, x, dx0, torch.float32)
    order = ["node_emb", "adaptive_embedding", "input_proj.weight", "input_proj.bias", "tod_embedding.weight", "dow_embedding.weight"]
    params = [sd[k].to(DEV) if k in sd else None for k in order]
    out = ops.stae_embed(dims, x.to(DEV), params)
    runs = [ops.stae_embed_backward(dims, x.to(DEV), dx0.to(DEV)) for _ in range(2)]
    torch.cuda.synchronize()
    TB.forward_bar(out.view(o64.shape), o64, o32, f"embed forward {shape} {widths}")
    assert [g is None for g in runs[0]] == [k not in sd for k in order]
    got = {k: g for k, g in zip(order, runs[0]) if g is not None}
    TB.assert_blocks(got, g64, g32, f"embed backward {shape} {widths}", d)
    if "dow_embedding.weight" in got:
        hit = set(x[..., 2].nan_to_num(0).long().clamp(0, TB.EMBED_DPW - 1).reshape(-1).tolist())
        missed = [r for r in range(TB.EMBED_DPW) if r not in hit]
        assert missed, "every table row is hit: the case does not test the zero rows"
        assert bool((got["dow_embedding.weight"].cpu()[missed] == 0).all())
    assert all(a is None and b is None or torch.equal(a, b) for a, b in zip(runs[0], runs[1])), "two runs differ"


# ---- output projection ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", TB.PROJ_CASES)
def test_output_proj_backward(case):
    b, t, n, d, o, c = case
    dims = R._lib.StaeDims(b, t, n, 8, 3, d, 0, 0, 0, 0, 288, 7, d // 32, 32, 1, o, c, 1, 1e-5)
    gen = torch.Generator().manual_seed(sum(case))
    x = torch.randn(b * t * n, d, generator=gen)
    w = (torch.rand(o * c, t * d, generator=gen) * 2 - 1) / (t * d) ** 0.5
    bias = 0.4 * (torch.rand(o * c, generator=gen) - 0.5)
    dout = torch.randn(b, o, n, c, generator=gen)

    def oracle(dtype):
        xx, ww, bb = (z.detach().to(dtype).requires_grad_(True) for z in (x, w, bias))
        rows = xx.view(b, t, n, d).transpose(1, 2).reshape(b, n, t * d)
        out = (rows @ ww.T + bb).view(b, n, o, c).transpose(1, 2)
        return out.detach(), dict(zip(("dx_proj", "dw", "db"), torch.autograd.grad(out, (xx, ww, bb), dout.to(dtype))))

    (o64, g64), (o32, g32) = oracle(torch.float64), oracle(torch.float32)
    out = ops.stae_output_proj(dims, x.to(DEV), w.to(DEV), bias.to(DEV))
    TB.forward_bar(out, o64, o32, f"output_proj forward {case}")
    buf = torch.full((b + 1, o + 1, n + 2, c + 3), float("nan"), device=DEV)          # dout as a strided window of a NaN-filled buffer
    win = buf[1:, :o, 1:n + 1, 2:c + 2]
    win.copy_(dout)
    runs = [ops.stae_output_proj_backward(dims, x.to(DEV), w.to(DEV), win) for _ in range(2)]
    torch.cuda.synchronize()
    got = dict(zip(("dx_proj", "dw", "db"), runs[0]))
    TB.assert_blocks(got, g64, g32, f"output_proj backward {case}", d)
    assert all(torch.equal(a, b_) for a, b_ in zip(runs[0], runs[1])), "two runs differ"
    assert ops.stae_output_proj_backward(dims, x.to(DEV), w.to(DEV), win, need_dx=False)[0] is None


# ---- the model ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(TB.MODEL_CASES))
def test_model_gradients_against_float64(name):
    case, (o64, g64), (o32, g32) = TB.model_case(name)
    mod = TB.make_model(case)
    out, grads = TB.run_model_backward(mod, case["x"], case["dout"], case["keep"])
    TB.forward_bar(out, o64, o32, f"model forward {name}")
    assert set(grads) == set(g64) and all(g is not None for g in grads.values())
    TB.assert_blocks(grads, g64, g32, f"model backward {name}", case["dim"], case["scales"])
    if case["keep"] is not None:
        assert mod.last_keep is not None and torch.equal(mod.last_keep.cpu(), case["keep"])
        out2, grads2 = TB.run_model_backward(mod, case["x"], case["dout"], case["keep"])                 # replay: equal bits
        assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
        torch.manual_seed(1)
        a = mod(case["x"].to(DEV)).detach()
        k1 = mod.last_keep
        b = mod(case["x"].to(DEV)).detach()
        assert not torch.equal(k1, mod.last_keep) and not torch.equal(a, b), "two fresh draws agree"
        assert torch.equal(mod(case["x"].to(DEV), keep=k1).detach(), a)


@pytest.mark.parametrize("tag", TB.GOLDEN_RECORDS)
def test_model_reproduces_the_reference_train_mode_records(tag):
    """out, run.py's per-snapshot losses and every recorded parameter gradient of the reference in train mode; r1 with its keep words."""
    case, (o_ref, l_ref, g_ref), (o64, l64, g64), (o32, l32, g32) = TB.golden_case(tag)
    mod = TB.make_model(case)
    mod.zero_grad(set_to_none=True)
    out = mod(case["x"].to(DEV), keep=None if case["keep"] is None else case["keep"].to(DEV))
    losses = ((out - case["y"].to(DEV).unsqueeze(1)) ** 2).mean(dim=(1, 2, 3))          # run.py:184-186 per snapshot
    losses.sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in mod.named_parameters()}
    TB.forward_bar(out, o64, o32, f"golden {tag}: out against float64")
    TB.forward_bar(losses, l64, l32, f"golden {tag}: losses against float64")
    TB.assert_blocks(grads, g64, g32, f"golden {tag}: gradients", case["dim"], case["scales"], max_ill=0.0)
    # against the recorded fp32 values themselves: both sides are within the forward bar of float64, so within twice it of each other
    for got, ref, r64, r32, what in ((out, o_ref, o64, o32, "out"), (losses, l_ref, l64, l32, "loss")):
        bar = 2 * (1e-5 + TB.K_GAP * float((r32.double() - r64).abs().max()))
        err = float((got.detach().cpu().double() - ref.double()).abs().max())
        print(f"golden {tag}: {what} against the recorded values: max |error| {err:.3g} (bar {bar:.3g})")
        assert err <= bar, (tag, what, err, bar)


def test_model_eval_path_is_the_parents_and_gradients_accumulate():
    case, _, _ = TB.model_case("drop")
    mod = TB.make_model(case)
    parent = TB.make_model(case, R.STAEformer).eval()
    x = case["x"].to(DEV)
    mod.eval()
    with torch.no_grad():
        assert torch.equal(mod(x, keep=case["keep"].to(DEV)), parent(x))
    with pytest.raises(NotImplementedError, match="inference only"):
        parent(x)
    mod.train()
    _, once = TB.run_model_backward(mod, case["x"], case["dout"], case["keep"])
    once = {k: v.clone() for k, v in once.items()}
    mod.zero_grad(set_to_none=True)
    with F_.grad_accumulation_in_backward():
        for _ in range(2):
            mod(x, keep=case["keep"].to(DEV)).backward(case["dout"].to(DEV))
    torch.cuda.synchronize()
    for k, p in mod.named_parameters():
        assert torch.equal(p.grad, once[k] + once[k]), k
    # every parameter frozen and x asking for a gradient: the composed path runs, x has no gradient to get, nothing raises
    for p in mod.parameters():
        p.requires_grad_(False)
    xr = x.clone().requires_grad_(True)
    mod(xr, keep=case["keep"].to(DEV)).backward(case["dout"].to(DEV))
    assert xr.grad is None and all(p.grad is None or not p.requires_grad for p in mod.parameters())
    for p in mod.parameters():
        p.requires_grad_(True)
    with pytest.raises(R.RegtError):
        mod(x, keep=case["keep"].to(DEV)[:, :5])
    with pytest.raises(ValueError):
        mod(x[:, :2])


def test_train_epoch_staeformer_batched_equals_sequential_and_float64():
    case, _, _ = TB.model_case("drop")
    kw, d = case["kw"], case["dim"]
    n, t, o, layers, p = kw["num_nodes"], kw["in_steps"], kw["out_steps"], kw["num_layers"], kw["dropout"]
    gen = torch.Generator().manual_seed(321)
    xs = [TB.features(1, t, n, 8, gen, 288)[0].permute(1, 2, 0).contiguous() for _ in range(4)]           # (N, F, T) snapshots
    ys = [torch.randn(n, o, generator=gen) for _ in range(4)]
    keeps = TM.pack_keep(torch.rand(4 * layers, 4, t * n, d, generator=gen) >= p)
    store = R.train.WindowStore([x.to(DEV) for x in xs], [y.to(DEV) for y in ys])
    res = {}
    for sb in (1, 4):
        mod = TB.make_model(case)
        opt = torch.optim.SGD(mod.parameters(), lr=0.0)                          # the step changes nothing: .grad is read before it
        grads = {}
        hooks = [p_.register_post_accumulate_grad_hook(lambda q, k=k: grads.__setitem__(k, q.grad.clone())) for k, p_ in mod.named_parameters()]
        last, per = R.train.train_epoch_staeformer(mod, store, opt, sb, keeps=keeps.to(DEV))
        torch.cuda.synchronize()
        [h.remove() for h in hooks]
        assert torch.equal(last, per[-1]) and len(per) == 4
        res[sb] = (torch.stack(per).cpu(), {k: v.cpu() for k, v in grads.items()})
    x4 = torch.stack(xs).permute(0, 3, 1, 2)
    y4 = torch.stack(ys)
    k4 = keeps.reshape(4 * layers, -1, d // 32)
    _, l64, g64 = TM.model_grads(case["sd"], x4, o, keep=k4, drop=p, y=y4)
    _, l32, g32 = TM.model_grads(case["sd"], x4, o, keep=k4, drop=p, y=y4, dtype=torch.float32)
    scales = TM.key_bias_scales(case["sd"], x4, o, keep=k4, drop=p, y=y4)
    for sb in (1, 4):
        TB.forward_bar(res[sb][0], l64, l32, f"per-snapshot losses, snap_batch {sb}")
        TB.assert_blocks(res[sb][1], g64, g32, f"accumulated gradients, snap_batch {sb}", d, scales)


def test_command_lines_train_then_evaluate(tmp_path):
    fixture = os.path.join(ROOT, "tests", "golden", "tpims_fixture.npz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--fixture", fixture, "--num_timesteps_in", "6", "--num_timesteps_out", "1", "--snap_batch", "8"]
    train = ["timeout", "-k", "10", "150", sys.executable, "-m", "regtgcn_amd.train_staeformer", *common, "--tr", "0.1", "--tf", "occrate", "--epochs", "1",
             "--out_dir", str(tmp_path)]
    r = subprocess.run(train, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Train Loss:")]
    assert len(lines) == 2, r.stdout                                              # epochs 0 and 1: two epochs
    ckpt = os.path.join(str(tmp_path), "occrate", "STAEformer", "model_in6_out1_epoch0.pt")
    assert os.path.exists(ckpt), os.listdir(str(tmp_path))
    ev = ["timeout", "-k", "10", "150", sys.executable, "-m", "regtgcn_amd.evaluate", "--fixture", fixture, "--checkpoint", ckpt, "--model", "STAEformer",
          "--num_timesteps_in", "6", "--num_timesteps_out", "1", "--tr", "0.9", "--snap_batch", "8"]
    r = subprocess.run(ev, cwd=str(tmp_path), env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "MAE:" in r.stdout and "nan" not in r.stdout.lower()
