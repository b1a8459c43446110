"""The window backward on the host: its dring bar recomputed (tests/window_bwd_math.py), the planted corruptions, the order guarantee of
the restatement, the new symbols and host-side refusals, and the EPOCH IDENTITY of streamed training on the float64 oracle -- the sum
of per-window autograd gradients equals the form factored through the per-step cell outputs."""
import os

import pytest
import torch

import window_bwd_math as B
from conftest import region_lists
from grad_bars import REL
from oracle import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table():
    return B.bar_table()


def test_bar_is_four_times_the_worst_restatement_rounded_up(table):
    rows, bar = table
    assert bar == B.BAR_DRING
    worst = max(r for _, r in rows)
    assert 4 * worst <= B.BAR_DRING < 8 * worst or B.BAR_DRING == B.grad_bars.CAP["default"]


def test_docstring_and_profile_hold_the_table(table):
    rows, bar = table
    text = open(os.path.join(ROOT, "profiles", "window_bwd_bars.txt")).read()
    for case, r in rows:
        line = f"{str(case):<50} {r:.2e}"
        assert line in B.__doc__, line
        assert line in text, line
    assert f"2 ** {int(torch.log2(torch.tensor(bar)).item())}" in B.__doc__


def test_cases_reach_every_edge():
    import regtgcn_amd as R
    lib = R.load_library()
    assert lib.regt_window_backward_max_t() == B.MAX_T and lib.regt_window_chunk(2) == B.WC
    assert set(c for c in B.W.CASES if c[2] <= B.MAX_T) <= set(B.CASES)
    assert any(w < t for _, _, t, _, _, w in B.CASES) and any(w == 1 for *_, w in B.CASES)
    assert any(w + t - 1 == B.WC for _, _, t, _, _, w in B.CASES) and any(w + t - 1 == B.WC + 1 for _, _, t, _, _, w in B.CASES)
    assert any(t == B.MAX_T for _, _, t, _, _, _ in B.CASES) and any(t == 1 for _, _, t, _, _, _ in B.CASES)
    assert any(f + w + t - 1 > r for _, _, t, r, f, w in B.CASES)                 # a covered range that wraps
    for n, c, t, r, f, w in B.CASES:
        assert c % 4 == 0 and 1 <= t <= B.MAX_T and 0 <= f < r and w + t - 1 <= r


@pytest.mark.parametrize("kind", B.CORRUPTIONS)
def test_planted_corruption_breaks_its_bar(kind):
    worst_d = worst_a = 0.0
    for case in B.CASES:
        x = B.inputs(case)
        ref = B.reference64(x, case, True)
        dring, d_att = B.restatement32(x, ref["dhidden"], case, True, corrupt=kind)
        cov = B.covered(case)
        assert not bool(torch.isnan(dring[cov]).any()) or kind == "no_wrap"
        worst_d = max(worst_d, B.dring_ratio(torch.nan_to_num(dring), ref, case))
        worst_a = max(worst_a, B.att_ratio(d_att, ref))
    if kind == "no_mean":
        assert worst_a > 2 * REL["attention"], (kind, worst_a)
    else:
        assert worst_d > 2 * B.BAR_DRING, (kind, worst_d)


def test_clean_restatement_meets_both_bars_and_leaves_other_slots_alone():
    for case in B.CASES:
        x = B.inputs(case)
        for acc in (False, True):
            ref = B.reference64(x, case, acc)
            dring, d_att = B.restatement32(x, ref["dhidden"], case, acc)
            assert B.dring_ratio(dring, ref, case) <= B.BAR_DRING
            assert B.att_ratio(d_att, ref) <= REL["attention"]
            other = torch.ones(case[3], dtype=torch.bool)
            other[B.covered(case)] = False
            if acc:
                assert torch.equal(dring[other], x["carried"][other])
            else:
                assert bool(torch.isnan(dring[other]).all())


def test_restatement_is_the_same_bits_however_the_windows_are_split():
    """The stated order is per slot: one call, or the same windows over consecutive accumulating calls, or a rotated ring."""
    case = (3, 8, 6, 30, 4, 20)
    n, c, t, ring_len, first, windows = case
    x = B.inputs(case)
    ref = B.reference64(x, case, True)
    whole, _ = B.restatement32(x, ref["dhidden"], case, True)
    for cuts in ((7,), (3, 11)):
        run = dict(x)
        lo = 0
        for hi in list(cuts) + [windows]:
            part = (n, c, t, ring_len, (first + lo) % ring_len, hi - lo)
            out, _ = B.restatement32(run, ref["dhidden"][lo:hi], part, True)
            run = dict(run, carried=out)
            lo = hi
        assert torch.equal(run["carried"], whole), cuts
    rolled = dict(x, carried=torch.roll(x["carried"], 5, dims=0), ring=torch.roll(x["ring"], 5, dims=0))
    out, _ = B.restatement32(rolled, ref["dhidden"], (n, c, t, ring_len, (first + 5) % ring_len, windows), True)
    assert torch.equal(torch.roll(out, -5, dims=0), whole)


def test_symbols_flag_and_host_side_refusals():
    import regtgcn_amd as R
    from regtgcn_amd import _lib
    lib = R.load_library()
    assert _lib.DIMS_NO_HEAD == 16 and _lib.ABI_VERSION == 8 and lib.regt_abi_version() == 8
    need = lib.regt_window_backward_workspace_bytes(104, 256, 128, 1, 15, 6)
    assert need > 15 * 104 * (256 + 2 * 128) * 4
    assert lib.regt_window_backward_workspace_bytes(104, 256, 128, 1, 15, 33) == 0 and b"T <= 32" in lib.regt_last_error()
    assert lib.regt_window_backward_workspace_bytes(104, 254, 128, 1, 15, 6) == 0
    one = 256                                                # a non-NULL, 16-byte aligned dummy that is never dereferenced
    args = [one, 20, 0, 15, 104, 6, 256, 1, 128] + [one] * 8 + [1] + [one] * 6 + [need, None]
    bad = list(args); bad[5] = 33; bad[1] = 60
    assert lib.regt_window_backward(*bad) != 0 and b"exceeds the 32 periods" in lib.regt_last_error()
    bad = list(args); bad[1] = 19
    assert lib.regt_window_backward(*bad) != 0 and b"would wrap" in lib.regt_last_error()
    bad = list(args); bad[-2] = need - 1
    assert lib.regt_window_backward(*bad) != 0 and b"workspace" in lib.regt_last_error()
    bad = list(args); bad[16] = None
    assert lib.regt_window_backward(*bad) != 0 and b"NULL" in lib.regt_last_error()
    with pytest.raises(R.RegtError):
        R.ops.window_backward(torch.zeros(1), 0, 1, *[torch.zeros(1)] * 8, True, *[torch.zeros(1)] * 5)      # CPU tensors
    for f in ("period_gradients",):
        assert hasattr(R.RegionalTemporalGCN, f) and hasattr(R.TemporalGCN, f)
    assert callable(R.train.train_epoch_streamed)


def test_train_command_refuses_streamed_train_where_it_does_not_apply(monkeypatch):
    import regtgcn_amd as R
    base = ["--fixture", "none.npz", "--num_timesteps_in", "6", "--num_timesteps_out", "1", "--streamed_train"]
    for extra, word in ((["--model", "GAT"], "--streamed_train covers"), (["--model", "STID"], "--streamed_train covers"),
                        (["--model", "TemporalGCN", "--fused_step"], "--fused_step"),
                        (["--model", "RegionalTemporalGCN", "--snap_batch", "4"], "--snap_batch")):
        with pytest.raises(SystemExit, match=word):
            R.train.main(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one GPU"):
        R.train.main(base + ["--model", "TemporalGCN"])
    a = R.train.build_parser().parse_args(["--streamed_train"])
    assert a.streamed_train and not a.streamed


def test_epoch_identity_on_the_float64_oracle(tpims):
    """2 T + 3 windows of the fixture: the sum of the per-window autograd gradients of oracle.model equals the factored form --
    S_s from a T = 1 cell with one logit, hidden_w = sum_p prob_p S_{w+p}, the head, and per-step dS pushed through the T = 1 cell."""
    t_in, t_out = 6, 1
    count = 2 * t_in + 3
    dt = torch.float64
    nd = tpims["node_data"].to(dt)
    n = nd.shape[0]
    ri, rw = region_lists(tpims)
    rw = [w.to(dt) for w in rw]
    ei = tpims["edge_index"]
    p0 = M.init_params("RegionalTemporalGCN", 8, t_in, t_out, num_nodes=n, seed=11)
    # per window
    pw = {k: v.detach().to(dt).requires_grad_(True) for k, v in p0.items()}
    losses = []
    for w in range(count):
        pred, _ = M.regional_temporal_gcn(pw, nd[:, :, w:w + t_in].contiguous(), ei, ri, rw)
        loss = torch.mean((pred - nd[:, -1, w + t_in:w + t_in + t_out]) ** 2)
        loss.backward()
        losses.append(float(loss.detach()))
    want = {k: v.grad for k, v in pw.items()}
    # factored
    pf = {k: v.detach().to(dt).requires_grad_(True) for k, v in p0.items()}
    one = dict(pf)
    one["tgnn._attention"] = torch.zeros(1, dtype=dt)
    steps = count + t_in - 1
    with torch.no_grad():
        s_all = torch.stack([M.regional_temporal_gcn(one, nd[:, :, s:s + 1].contiguous(), ei, ri, rw)[1] for s in range(steps)])
    s_leaf = s_all.clone().requires_grad_(True)
    prob = torch.softmax(pf["tgnn._attention"], dim=0)
    total = 0.0
    for w in range(count):
        hidden = (prob.view(-1, 1, 1) * s_leaf[w:w + t_in]).sum(dim=0)
        pred = M.head(pf, hidden)
        lw = torch.mean((pred - nd[:, -1, w + t_in:w + t_in + t_out]) ** 2)
        assert abs(float(lw.detach()) - losses[w]) <= 1e-12 * max(1.0, abs(losses[w]))
        total = total + lw
    total.backward()                                          # d attention, d head, dS
    d_s = s_leaf.grad
    for s in range(steps):
        _, s_s = M.regional_temporal_gcn(one, nd[:, :, s:s + 1].contiguous(), ei, ri, rw)
        (s_s * d_s[s]).sum().backward()                       # adds the step's cell and embedding gradients to pf's .grad
    checked = 0
    for k, g in want.items():
        got = pf[k].grad
        if g is None or float(g.abs().max()) == 0.0:
            assert got is None or float(got.abs().max()) == 0.0, k
            continue
        assert got is not None, k
        scale = float(g.abs().max())
        assert float((got - g).abs().max()) <= 1e-11 * scale, (k, float((got - g).abs().max()), scale)
        checked += 1
    assert checked >= 20
