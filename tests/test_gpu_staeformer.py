"""STAEformer inference on the GPU: the reference module's eval-mode goldens with the run.py / predict.py metrics, the attention
and add+LayerNorm entry points against the float64 restatement (ragged and multiple key tiles, head counts, batches, odd sequence
counts, strided windows of one buffer, large scores, poisoned surroundings, sentinels, bit-reproducibility), the embedding and
output projection through whole-model comparisons at small sizes, and the evaluation command.

Tolerances, all absolute.  Against the reference goldens: 1e-5 + GAP on outputs and metrics (GAP is the fp32-vs-float64 gap of the
reference on the goldens, tests/test_staeformer_cpu.py) and 1e-3 on MAPE, which predict.py scales by 100.  Against the float64
restatement: 1e-5 + K_GAP x the fp32-vs-float64 gap of the same restatement evaluated in fp32 on the same inputs, with K_GAP = 4 as
for STNorm and STID: torch sums a dot product in pairwise blocks, the kernels on the matrix unit in sequence, and the online
softmax rescales partial sums tile by tile.  Every comparison prints the K it needed (max |error| / gap); a restatement is computed
once per case on the host."""
import os

import numpy as np
import pytest
import torch

from conftest import load_npz
from staeformer_math import add_layernorm, attention, golden_state_dict, staeformer
from test_staeformer_cpu import GAP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["in6_out1", "in12_out3_b2"]
DEV = "cuda:0"
K_GAP = 4
SENTINEL = -777.0


def _bar(got, r64, r32, what):
    """|got - r64| <= 1e-5 + K_GAP * max|r32 - r64|; prints the K the case needed."""
    got, r64 = got.detach().cpu().double(), r64.double()
    gap = float((r32.double() - r64).abs().max())
    err = float((got - r64).abs().max())
    print(f"{what}: max |error| {err:.3g}, fp32 restatement gap {gap:.3g}, K needed {err / max(gap, 1e-30):.2f} (bar K_GAP = {K_GAP} + 1e-5)")
    assert torch.isfinite(got).all(), what
    assert err <= 1e-5 + K_GAP * gap, (what, err, gap)


def _module(g):
    import regtgcn_amd as R
    mod = R.STAEformer(num_nodes=int(g["nodes"]), in_steps=int(g["t_in"]), out_steps=int(g["t_out"]), tod_embedding_dim=0,
                       num_layers=int(g["num_layers"]))
    mod.load_state_dict(golden_state_dict(g), strict=True)
    return mod.to(DEV).eval()


# ---- the reference's goldens ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_eval_output_and_metrics_match_reference_golden(tag):
    from regtgcn_amd.evaluate import predict_metrics_staeformer
    g = load_npz(f"golden_staeformer_{tag}.npz")
    mod = _module(g)
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    with torch.no_grad():
        out = mod(x)
    assert tuple(out.shape) == tuple(g["eval__out"].shape)
    err = float((out.cpu() - torch.from_numpy(g["eval__out"])).abs().max())
    print(f"{tag}: eval out max |diff| {err:.3g} (bound {1e-5 + GAP:.3g})")
    assert err <= 1e-5 + GAP
    for k in range(x.shape[0]):                                                   # run.py:217-222
        assert abs(float(((out[k][0] - y[k]) ** 2).mean()) - g["eval__test_mse"][k]) <= 1e-5 + GAP
    xs = [x[k].permute(1, 2, 0).contiguous() for k in range(x.shape[0])]          # back to the (N, F, T) snapshots
    mae, rmse, mape = predict_metrics_staeformer(mod, xs, list(y), snap_batch=x.shape[0])
    assert abs(mae - g["eval__mae"][0]) <= 1e-5 + GAP
    assert abs(rmse - np.sqrt(g["eval__mse"][0])) <= 1e-5 + GAP
    assert abs(mape - g["eval__mape"][0]) <= 1e-3
    mae1, rmse1, mape1 = predict_metrics_staeformer(mod, xs, list(y), snap_batch=1)            # one snapshot per call: the same numbers
    assert abs(mae1 - mae) <= 1e-6 and abs(rmse1 - rmse) <= 1e-6 and abs(mape1 - mape) <= 1e-4


def test_inference_only_refusals():
    import regtgcn_amd as R
    g = load_npz("golden_staeformer_in12_out3_b2.npz")
    mod = _module(g)
    x = torch.from_numpy(g["x"]).to(DEV)
    with pytest.raises(NotImplementedError, match="inference only"):
        mod(x)                                                    # grad mode on, parameters require grad
    with torch.no_grad():
        ref = mod(x)
        with pytest.raises(NotImplementedError, match="inference only"):
            mod.train()(x)                                        # dropout 0.1 would draw masks
    for p in mod.parameters():
        p.requires_grad_(False)
    mod.eval()
    assert torch.equal(mod(x), ref)                               # nothing requires grad: no autograd record, the call runs
    with pytest.raises(NotImplementedError, match="inference only"):
        mod(x.clone().requires_grad_(True))
    torch.manual_seed(3)
    m0 = R.STAEformer(num_nodes=7, in_steps=4, out_steps=2, tod_embedding_dim=0, num_layers=1, dropout=0).to(DEV)
    x0 = torch.rand(2, 4, 7, 3, device=DEV)
    with torch.no_grad():
        a = m0.train()(x0)
        b = m0.eval()(x0)
    assert torch.equal(a, b)
    with pytest.raises(R.RegtError):
        m0(x0.cpu())
    with torch.no_grad(), pytest.raises(R.RegtError):
        R.STAEformer(num_nodes=7, in_steps=4, out_steps=2, tod_embedding_dim=0, num_layers=1).eval()(x0)      # parameters on the host


# ---- the attention entry point ----------------------------------------------------------------------------------------------------

def _attention_case(b, t, n, heads, axis, seed=0, q_scale=1.0, pad=8, tail_rows=0):
    """Q | K | V as column windows of one (M + tail_rows, 3 D + pad) buffer (row stride > 3 D), the restatement in float64 and fp32."""
    d, m = 32 * heads, b * t * n
    gen = torch.Generator().manual_seed(1000 * axis + seed)
    buf = torch.randn(m + tail_rows, 3 * d + pad, generator=gen)
    buf[:, :d] *= q_scale
    q, k, v = (buf[:m, i * d:(i + 1) * d].reshape(b, t, n, d) for i in range(3))
    r64 = attention(q, k, v, axis).reshape(m, d)
    r32 = attention(q, k, v, axis, dtype=torch.float32).reshape(m, d)
    return buf, r64, r32


def _run_attention(buf, b, t, n, heads, axis):
    """The op on the windows of ``buf``; out is a window of a sentinel-filled buffer, returned with that buffer."""
    from regtgcn_amd import ops
    d, m = 32 * heads, b * t * n
    dbuf = buf.to(DEV)
    q, k, v = (dbuf[:m, i * d:(i + 1) * d] for i in range(3))
    obuf = torch.full((m + 2, d + 8), SENTINEL, device=DEV)
    out = ops.stae_attention(q, k, v, b, t, n, heads, axis, out=obuf[1:m + 1, 4:4 + d])
    torch.cuda.synchronize()
    return out, obuf


def _check_window(obuf, m, d):
    """Nothing outside the M x D window of the sentinel-filled buffer was written."""
    o = obuf.cpu()
    assert bool((o[0] == SENTINEL).all()) and bool((o[m + 1] == SENTINEL).all())
    assert bool((o[:, :4] == SENTINEL).all()) and bool((o[:, 4 + d:] == SENTINEL).all())


@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("length", [1, 2, 12, 31, 32, 33, 64, 65, 104, 257])
def test_attention_over_sequence_lengths(length, axis):
    """Ragged and multiple key tiles; N = 5 sequences per batch element on the temporal axis and T = 3 on the spatial axis are no
    multiple of a workgroup's four waves."""
    b, t, n = (1, length, 5) if axis == 1 else (1, 3, length)
    buf, r64, r32 = _attention_case(b, t, n, 4, axis, seed=length)
    out, obuf = _run_attention(buf, b, t, n, 4, axis)
    _bar(out, r64, r32, f"attention axis {axis} L {length}")
    _check_window(obuf, b * t * n, 128)


@pytest.mark.parametrize("axis", [1, 2])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("heads", [1, 4, 8])
def test_attention_over_heads_and_batches(heads, batch, axis):
    b, t, n = (batch, 33, 5) if axis == 1 else (batch, 3, 33)
    buf, r64, r32 = _attention_case(b, t, n, heads, axis, seed=10 * heads + batch)
    out, obuf = _run_attention(buf, b, t, n, heads, axis)
    _bar(out, r64, r32, f"attention axis {axis} heads {heads} B {batch}")
    _check_window(obuf, b * t * n, 32 * heads)


@pytest.mark.parametrize("axis", [1, 2])
def test_attention_with_large_scores_is_stable(axis):
    """Q scaled by 30: scores reach the hundreds, exp() of them would overflow without the running maximum."""
    b, t, n = (2, 65, 5) if axis == 1 else (2, 3, 65)
    buf, r64, r32 = _attention_case(b, t, n, 4, axis, seed=77, q_scale=30.0)
    m = b * t * n
    q0, k0 = buf[:m, :32].reshape(b, t, n, 32), buf[:m, 128:160].reshape(b, t, n, 32)          # head 0
    scores = torch.einsum("blnd,bmnd->bnlm" if axis == 1 else "btld,btmd->btlm", q0, k0) / 32 ** 0.5
    assert float(scores.abs().max()) > 100
    out, _ = _run_attention(buf, b, t, n, 4, axis)
    _bar(out, r64, r32, f"attention axis {axis} Q x 30")


@pytest.mark.parametrize("axis", [1, 2])
def test_attention_reads_no_padding_key_and_no_foreign_row(axis):
    """Rows beyond the M rows hold NaN throughout; then the V rows of every other sequence are set to 1e30: the first and the last
    sequence's outputs do not change by a bit.  A padding key read into a result (0 x NaN, or a score of 0 instead of -inf) or a
    foreign row would show."""
    b, t, n = (2, 33, 5) if axis == 1 else (2, 3, 33)
    d, m = 128, b * t * n
    buf, r64, r32 = _attention_case(b, t, n, 4, axis, seed=5, tail_rows=40)
    buf[m:] = float("nan")
    out, _ = _run_attention(buf, b, t, n, 4, axis)
    _bar(out, r64, r32, f"attention axis {axis} with NaN rows behind the tensor")
    rows = torch.arange(m).reshape(b, t, n)
    for seq in ((0, 0), (b - 1, (n if axis == 1 else t) - 1)):
        own = rows[seq[0], :, seq[1]] if axis == 1 else rows[seq[0], seq[1], :]
        poisoned = buf.clone()
        foreign = torch.ones(m + 40, dtype=torch.bool)
        foreign[own] = False
        foreign[m:] = False
        poisoned[foreign, 2 * d:3 * d] = 1e30
        out2, _ = _run_attention(poisoned, b, t, n, 4, axis)
        assert torch.equal(out2[own.to(DEV)], out[own.to(DEV)]), (axis, seq)


def test_attention_is_bit_reproducible():
    for axis, (b, t, n) in ((1, (2, 12, 104)), (2, (2, 12, 104))):
        buf, _, _ = _attention_case(b, t, n, 4, axis, seed=9)
        a, _ = _run_attention(buf, b, t, n, 4, axis)
        c, _ = _run_attention(buf, b, t, n, 4, axis)
        assert torch.equal(a, c)


# ---- add + LayerNorm --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("d", [32, 128, 256])
def test_add_layernorm(d, m):
    from regtgcn_amd import ops
    gen = torch.Generator().manual_seed(d + m)
    r, y = torch.randn(m, d, generator=gen) * 2, torch.randn(m, d, generator=gen) + 0.5
    gamma, beta = 1 + 0.5 * torch.randn(d, generator=gen), torch.randn(d, generator=gen)
    r64 = add_layernorm(r, y, gamma, beta)
    r32 = add_layernorm(r, y, gamma, beta, dtype=torch.float32)
    rd, yd, gd, bd = (z.to(DEV) for z in (r, y, gamma, beta))
    obuf = torch.full((m + 2, d), SENTINEL, device=DEV)
    out = ops.stae_add_layernorm(rd, yd, gd, bd, out=obuf[1:m + 1])
    _bar(out, r64, r32, f"add_layernorm D {d} M {m}")
    assert bool((obuf[0] == SENTINEL).all()) and bool((obuf[m + 1] == SENTINEL).all())
    assert torch.equal(rd.cpu(), r)                                               # out of place: the residual is left alone
    inplace = ops.stae_add_layernorm(rd, yd, gd, bd, out=rd)
    assert inplace.data_ptr() == rd.data_ptr() and torch.equal(inplace, out)      # in place: the same bits


def test_add_layernorm_constant_row_is_finite():
    from regtgcn_amd import ops
    r = torch.full((3, 128), 0.3)
    y = torch.full((3, 128), 1.7)
    gamma, beta = torch.full((128,), 1.5), torch.full((128,), -0.25)
    out = ops.stae_add_layernorm(r.to(DEV), y.to(DEV), gamma.to(DEV), beta.to(DEV))
    assert torch.isfinite(out).all()
    _bar(out, add_layernorm(r, y, gamma, beta), add_layernorm(r, y, gamma, beta, dtype=torch.float32), "add_layernorm constant rows")


# ---- embedding and output projection through the whole model ----------------------------------------------------------------------

def _model_case(n, t, b, o, nl, seed, f=8, dow_values=None, **kw):
    import regtgcn_amd as R
    torch.manual_seed(seed)
    kw.setdefault("tod_embedding_dim", 0)
    mod = R.STAEformer(num_nodes=n, in_steps=t, out_steps=o, num_layers=nl, **kw)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith("bias"):
                p.copy_((torch.rand(p.shape, generator=gen) - 0.5) * 0.4)
            elif ".ln" in name:
                p.copy_(1.0 + (torch.rand(p.shape, generator=gen) - 0.5) * 0.5)
    x = torch.randn(b, t, n, f, generator=gen)
    x[..., 1] = torch.rand(b, t, n, generator=gen) * 0.999                         # time of day in [0, 1)
    x[..., 2] = torch.randint(0, 7, (b, t, n), generator=gen).float() + 0.25       # day of week, truncated by .long()
    if dow_values is not None:
        x[..., 2] = torch.tensor(dow_values)[torch.randint(0, len(dow_values), (b, t, n), generator=gen)]
    return mod, x


def _check_model(mod, x, what, clamp=False):
    sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    with torch.no_grad():
        r64 = staeformer(sd, x, mod.out_steps, mod.output_dim, clamp=clamp)
        r32 = staeformer(sd, x, mod.out_steps, mod.output_dim, dtype=torch.float32, clamp=clamp)
        out = mod.to(DEV).eval()(x.to(DEV))
    assert tuple(out.shape) == (x.shape[0], mod.out_steps, mod.num_nodes, mod.output_dim) == tuple(r64.shape)
    _bar(out, r64, r32, what)
    return out


@pytest.mark.parametrize("n,t,b,o,nl", [(1, 1, 1, 1, 1), (5, 6, 2, 3, 2), (104, 12, 1, 1, 1), (104, 6, 2, 3, 1), (5, 12, 1, 3, 2),
                                        (1, 6, 2, 1, 1), (104, 1, 1, 3, 1)])
def test_model_matches_restatement_at_small_sizes(n, t, b, o, nl):
    mod, x = _model_case(n, t, b, o, nl, seed=n + 10 * t + b + o + nl)
    _check_model(mod, x, f"model N {n} T {t} B {b} O {o} layers {nl}")


def test_model_with_spatial_embedding():
    mod, x = _model_case(37, 6, 2, 2, 1, seed=71, spatial_embedding_dim=32, adaptive_embedding_dim=48)
    assert mod.model_dim == 128 and "node_emb" in mod.state_dict()
    _check_model(mod, x, "model with node_emb")


def test_model_with_time_of_day_embedding_and_wider_output():
    mod, x = _model_case(37, 6, 2, 2, 1, seed=72, tod_embedding_dim=32, adaptive_embedding_dim=48, output_dim=3, input_dim=2, f=5)
    assert mod.model_dim == 128 and "tod_embedding.weight" in mod.state_dict()
    _check_model(mod, x, "model with tod_embedding, output_dim 3")


def test_out_of_range_table_indices_are_clamped():
    """x[..., 2] of 6.9, -0.5 and 9.0: .long() gives 6, 0 and 9; the kernel clamps 9 to the last row, 6 (the reference raises).
    The result is finite and equals the restatement given the clamped index; time of day 1.5 and -2.0 clamp to rows 287 and 0."""
    mod, x = _model_case(9, 6, 2, 1, 1, seed=73, dow_values=[6.9, -0.5, 9.0], tod_embedding_dim=32, adaptive_embedding_dim=48)
    x[0, 0, 0, 1], x[0, 0, 1, 1] = 1.5, -2.0
    assert {6, 0, 9} == set(x[..., 2].long().unique().tolist())
    out = _check_model(mod, x, "model with clamped indices", clamp=True)
    assert torch.isfinite(out).all()


def test_model_is_bit_reproducible():
    mod, x = _model_case(104, 12, 2, 3, 1, seed=74)
    mod = mod.to(DEV).eval()
    with torch.no_grad():
        assert torch.equal(mod(x.to(DEV)), mod(x.to(DEV)))


# ---- evaluation ---------------------------------------------------------------------------------------------------------------------

def test_evaluate_command_prints_finite_metrics(tmp_path, capsys):
    import regtgcn_amd as R
    torch.manual_seed(5)
    mod = R.STAEformer(num_nodes=104, in_steps=6, out_steps=1, tod_embedding_dim=0)
    ck = os.path.join(tmp_path, "staeformer.pt")
    torch.save(mod.state_dict(), ck)
    R.evaluate.main(["--model", "STAEformer", "--fixture", os.path.join(ROOT, "tests", "golden", "tpims_fixture.npz"), "--checkpoint", ck,
                     "--num_timesteps_in", "6", "--num_timesteps_out", "1", "--tr", "0.9", "--snap_batch", "8"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line.startswith("MAE:")
    values = [float(v.split(":")[1]) for v in line.split(",")]
    assert len(values) == 3 and all(np.isfinite(values)), line
