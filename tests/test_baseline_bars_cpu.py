"""grad_bars.assert_grads_conditioned on the three baselines (STNorm, STID, SpatialGCN) without a GPU.

For every gradient comparison of tests/test_gpu_stnorm.py, test_gpu_stid.py and test_gpu_spatial.py -- both goldens of each model,
every parametrised restatement case, the snapshot-batching runs, the kernel pair's shapes and the cfg-3 shapes of STID and
SpatialGCN -- the references decide here, before any GPU run, which blocks are ill-conditioned: none in a golden, none in any case
but STID's cfg-3 shape (17 of its 1609 blocks, one ReLU that fp32 takes the other way), and at most 5 % of the blocks of a file.
With the fp32 restatement standing in for the kernels the bar itself cannot fail (a well-conditioned block's fp32 error is under
CAP / 4, which is under REL; an ill-conditioned one is held to 4 x that same error): the content of these tests is the list of
ill-conditioned blocks and the printed ratios.  STNorm's cfg-3 shape (100 000 nodes) costs 40 s of float64 autograd on the host
and is left to its GPU test, which asserts an empty list itself (measured on the host: 0 of 25 172 blocks; folding them into
STNorm's share would only dilute it).  test_gpu_spatial draws its training masks on the device; here they come from a seeded
host generator.

Then seven corruptions of the fp32 gradients -- each a wrong term of the kind a rewritten backward kernel can produce -- fail the
assertion.  Next to every corruption stands what the comparison the GPU tests already make says to it (the goldens' absolute
1e-5; the restatement cases' 1e-5 + 4 x the whole tensor's fp32 gap; the kernel pair's rounding bound): that records which of
them the old bars let through."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_spatial as SP
import test_gpu_stid as SI
import test_gpu_stnorm as SN
from conftest import load_npz
from grad_bars import REL, assert_grads_conditioned, conditioned_rows, grad_blocks, grad_class, ill_conditioned

K_GAP = 4
assert SN.K_GAP == SI.K_GAP == SP.K_GAP == K_GAP
ILL_SHARE = 0.05


@functools.lru_cache(maxsize=None)
def _tpims():
    return {k: torch.from_numpy(v) for k, v in load_npz("tpims_fixture.npz").items() if v.ndim > 0}


def _host_mask(rows, seed):
    """(rows, 2) int32 keep words, every bit a fair coin: what draw_keep_mask gives, from a seeded host generator."""
    return torch.randint(-2 ** 31, 2 ** 31, (rows, 2), generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(torch.int32)


def _spatial_pair(i, masked):
    import regtgcn_amd as R
    if i is None:                                          # the cfg-3 shape of test_cfg3_shape_matches_restatement
        n, t, f = 100_000, 12, 32
        g = R.data.synthetic_regional_graph(n, 1_000_000, 5, seed=31)
        ei, ea, (x, w0, w1, b, ds) = g.edge_index, g.edge_attr, SP._inputs(n, t, f, seed=32)
    else:
        n, t, f = SP.KERNEL_PAIR_SHAPES[i]
        ei, ea, x, w0, w1, b, ds = SP.kernel_pair_inputs(R, n, t, f)
    keep = _host_mask(n * t, n + t) if masked else None
    _ref, g64, g32, allow = SP.embed_case(x, ei, ea, w0, w1, b, keep, ds)
    return g64, g32, dict(allow=allow)


# file -> [(case id, golden?, builder of (g64, g32, keywords of the assertion))]
def _cases():
    c = {"stnorm": [], "stid": [], "spatial": []}
    for tag in SN.TAGS:
        c["stnorm"].append((f"golden-{tag}", True, lambda tag=tag: SN.golden_case(tag) + ({},)))
        c["stid"].append((f"golden-{tag}", True, lambda tag=tag: SI.golden_case(tag) + (dict(input_dim=3),)))
        for mode in ("eval", "train"):
            c["spatial"].append((f"golden-{tag}-{mode}", True, lambda tag=tag, mode=mode: tuple(SP.golden_case(_tpims(), tag, mode)) + ({},)))
    for kw in SN.RESTATEMENT_CASES:
        def build(kw=kw):
            r = SN.restatement_case(**kw)
            return r["g64"], r["g32"], {}
        c["stnorm"].append(("-".join(f"{k}{v}" for k, v in kw.items()), False, build))
    c["stnorm"].append(("snapshot-batching", False, lambda: SN.snapshot_batching_case(SN.snapshot_batching_base())[2:] + ({},)))
    for kw in SI.RESTATEMENT_CASES:
        def build(kw=kw):
            r = SI.restatement_case(**kw)
            return r["g64"], r["g32"], dict(input_dim=r["input_dim"])
        c["stid"].append(("-".join(f"{k}{v}" for k, v in kw.items()), False, build))
    c["stid"].append(("snapshot-batching", False, lambda: SI.snapshot_batching_case()[4:] + (dict(input_dim=3),)))

    def stid_cfg3():
        r = SI.restatement_case(**SI.CFG3_CASE)
        return r["g64"], r["g32"], dict(input_dim=r["input_dim"])
    c["stid"].append(("cfg3", False, stid_cfg3))
    c["spatial"].append(("cfg3-train", False, lambda: _spatial_pair(None, True)))
    for i, (n, t, f) in enumerate(SP.KERNEL_PAIR_SHAPES):
        for masked in (False, True):
            c["spatial"].append((f"pair-{n}-{t}-{f}-{'train' if masked else 'eval'}", False, lambda i=i, masked=masked: _spatial_pair(i, masked)))
    return c


CASES = _cases()
ALL = [(f, cid) for f, lst in CASES.items() for cid, _g, _b in lst]


@functools.lru_cache(maxsize=None)
def _result(file, cid):
    """(ill-conditioned labels, number of blocks, worst fp32 ratio per class over the well-conditioned blocks) of one case."""
    golden, build = next((g, b) for c, g, b in CASES[file] if c == cid)
    g64, g32, kw = build()
    ill, nblocks = assert_grads_conditioned(g32, g64, g32, K_GAP, REL, f"{file} {cid}: fp32 restatement", **kw)
    worst = {}
    for label, cls, _err, scale, gap, _x in conditioned_rows(g32, g64, g32, **kw):
        if scale > 0 and not ill_conditioned(cls, scale, gap) and gap / scale > worst.get(cls, (0.0, ""))[0]:
            worst[cls] = (gap / scale, label)
    return ill, nblocks, worst, golden


@pytest.mark.parametrize("file,cid", ALL, ids=[f"{f}-{c}" for f, c in ALL])
def test_references_name_the_ill_conditioned_blocks(file, cid):
    ill, nblocks, worst, golden = _result(file, cid)
    for cls, (ratio, label) in worst.items():
        print(f"  {file} {cid}: {nblocks} blocks, worst fp32 ratio [{cls}] {ratio:.2e} at {label} (bar {REL[cls]:.2e})")
    print(f"  ill-conditioned: {ill}")
    if (file, cid) == ("stid", "cfg3"):
        assert 0 < len(ill) <= SI.CFG3_ILL_SHARE * nblocks
    else:
        assert ill == []


@pytest.mark.parametrize("file", list(CASES))
def test_ill_conditioned_blocks_stay_within_their_share_of_each_file(file):
    res = [_result(file, cid) for cid, _g, _b in CASES[file]]
    n_ill, n_blocks = sum(len(r[0]) for r in res), sum(r[1] for r in res)
    print(f"  {file}: {n_ill} ill-conditioned of {n_blocks} blocks")
    assert n_ill <= ILL_SHARE * n_blocks


def test_blocks_split_what_separate_tiles_taps_and_accumulators_produce():
    blocks = grad_blocks("node_emb", torch.zeros(130, 32))
    assert [b.shape[0] for _l, b in blocks] == [64, 64, 2] and "ragged" in blocks[-1][0] and "ragged" not in blocks[0][0]
    assert [b.shape[1] for _l, b in grad_blocks("time_series_emb_layer.weight", torch.zeros(32, 18, 1, 1), input_dim=3)] == [3] * 6
    assert [tuple(b.shape[:2]) for _l, b in grad_blocks("encoder.1.fc2.weight", torch.zeros(64, 64, 1, 1))] == [(32, 32)] * 4
    assert [tuple(b.shape[:2]) for _l, b in grad_blocks("regression_layer.weight", torch.zeros(33, 64, 1, 1))] == [(32, 32)] * 2 + [(1, 32)] * 2
    w = torch.arange(16 * 48 * 2, dtype=torch.float32).view(16, 48, 1, 2)
    blocks = grad_blocks("gate_convs.5.weight", w)
    assert len(blocks) == 6 and torch.equal(blocks[4][1], w[:, 16:32, :, 1:2])
    assert [b.shape[2] for _l, b in grad_blocks("tn.3.beta", torch.zeros(1, 16, 130, 1))] == [64, 64, 2]
    assert [b.shape[1] for _l, b in grad_blocks("gcn.lins.1.weight", torch.zeros(64, 40))] == [16, 16, 8]
    for name, t in (("gcn2.lins.1.weight", torch.zeros(256, 64)), ("sn.2.gamma", torch.zeros(16)), ("skip_convs.0.weight", torch.zeros(16, 16, 1, 1))):
        assert len(grad_blocks(name, t)) == 1
    assert grad_class("tn.6.beta") == grad_class("sn.7.gamma") == grad_class("start_conv.bias") == grad_class("gate_convs.5.weight") == "norm"
    assert grad_class("skip_convs.1.weight") == grad_class("node_emb") == grad_class("gcn.lins.1.weight") == grad_class("linear1.weight") == "default"


def test_ill_conditioned_block_is_held_to_the_fp32_gap_without_a_floor():
    want = {"start_conv.bias": torch.tensor([1e-3, -1e-3], dtype=torch.float64)}
    ref32 = {"start_conv.bias": torch.tensor([1e-3 + 4e-6, -1e-3])}                       # 4e-3 of scale > CAP / 4: ill-conditioned
    ill, n = assert_grads_conditioned({"start_conv.bias": torch.tensor([1e-3 + 1.5e-5, -1e-3])}, want, ref32, K_GAP)
    assert ill == ["start_conv.bias"] and n == 1
    with pytest.raises(AssertionError, match="ill-conditioned"):                           # 1.7e-5 > 4 x 4e-6: no 1e-5 floor helps
        assert_grads_conditioned({"start_conv.bias": torch.tensor([1e-3 + 1.7e-5, -1e-3])}, want, ref32, K_GAP)
    ref32 = {"start_conv.bias": torch.tensor([1e-3 + 1e-8, -1e-3])}                       # well-conditioned: the relative bar holds
    with pytest.raises(AssertionError, match="off their own scale"):
        assert_grads_conditioned({"start_conv.bias": torch.tensor([1e-3 + 1e-6, -1e-3])}, want, ref32, K_GAP)
    zero = {"a": torch.zeros(2, dtype=torch.float64), "b": None}
    assert_grads_conditioned({"a": torch.zeros(2), "b": None}, zero, {"a": torch.zeros(2), "b": None}, K_GAP)
    with pytest.raises(AssertionError):
        assert_grads_conditioned({"a": torch.tensor([0.0, 1e-30]), "b": None}, zero, {"a": torch.zeros(2), "b": None}, K_GAP)
    with pytest.raises(AssertionError):
        assert_grads_conditioned({"a": torch.zeros(2), "b": torch.ones(1)}, zero, {"a": torch.zeros(2), "b": None}, K_GAP)


# ---- corruptions -------------------------------------------------------------------------------------------------------------------

def _old_bar_accepts(got, want, atol, rtol=0.0):
    """The comparison the GPU tests make today, tensor by tensor: assert_allclose(atol, rtol); `atol` a number or {name: number}."""
    ok = True
    for k, w in want.items():
        if w is None:
            continue
        a = atol[k] if isinstance(atol, dict) else atol
        off = int((~np.isclose(got[k].double().numpy(), w.double().numpy(), atol=a, rtol=rtol)).sum())
        if off:
            print(f"  old bar: {k}: {off} of {w.numel()} elements off")
            ok = False
    return ok


def _restatement_atol(g64, g32):
    return {k: 1e-5 + K_GAP * float((g32[k].double() - v).abs().max()) for k, v in g64.items() if v is not None}


@functools.lru_cache(maxsize=None)
def _stnorm_two_windows():
    """The in12_out3 golden's parameters on a batch of its window and the next one (mean-squared loss over both): the golden's own
    gradient scales with a batch to lose an element from.  Returns g64, g32 and sn.7.gamma's fp32 gradient per batch element."""
    g, keys = SN._golden("in12_out3")
    fx = _tpims()
    t_in, t_out, w, n = int(g["t_in"]), int(g["t_out"]), int(g["window"]), int(g["nodes"])
    x = torch.stack([fx["node_data"][:n, :, w + k:w + k + t_in].permute(2, 0, 1) for k in range(2)]).contiguous()
    y = torch.stack([fx["node_data"][:n, -1, w + k + t_in:w + k + t_in + t_out] for k in range(2)])
    params = {k: torch.from_numpy(g[f"p__{k}"]) for k in keys}
    g64, _, _ = SN._restated_grads(params, x, lambda o: torch.mean((o - y.double().unsqueeze(1)) ** 2), torch.float64)
    g32, _, _ = SN._restated_grads(params, x, lambda o: torch.mean((o - y.unsqueeze(1)) ** 2), torch.float32)
    split = dict(params)
    split["sn.7.gamma"] = params["sn.7.gamma"].expand(2, -1).contiguous()
    per_element, _, _ = SN._restated_grads(split, x, lambda o: torch.mean((o - y.unsqueeze(1)) ** 2), torch.float32)
    return g64, g32, per_element["sn.7.gamma"]


def _tn_beta_scaled():
    g64, g32 = SN.golden_case("in12_out3")
    g = dict(g32)
    g["tn.6.beta"] = g32["tn.6.beta"] * 1.1
    return g, g64, g32, {}, 1e-5


def _sn_gamma_without_one_batch_element():
    g64, g32, per_element = _stnorm_two_windows()
    assert torch.allclose(per_element.sum(0), g32["sn.7.gamma"], rtol=1e-4, atol=1e-9)
    g = dict(g32)
    g["sn.7.gamma"] = per_element[0]
    return g, g64, g32, {}, 1e-5


def _gate_conv_tap_sign_flipped():
    g64, g32 = SN.golden_case("in12_out3")
    g = dict(g32)
    g["gate_convs.5.weight"] = g32["gate_convs.5.weight"].clone()
    g["gate_convs.5.weight"][..., 1] *= -1.0
    return g, g64, g32, {}, 1e-5


def _node_emb_wrong_in_the_ragged_tile():
    """n = 130: the last tile holds two nodes; their rows come out swapped.  Held today to 1e-5 + 4 x the whole tensor's gap."""
    r = SI.restatement_case(**next(k for k in SI.RESTATEMENT_CASES if k["n"] == 130 and k["o"] == 3))
    g64, g32 = r["g64"], r["g32"]
    g = dict(g32)
    g["node_emb"] = g32["node_emb"].clone()
    g["node_emb"][128:] = g32["node_emb"][128:].flip(0) * 1.0
    return g, g64, g32, dict(input_dim=3), _restatement_atol(g64, g32)


def _node_emb_ragged_tile_of_the_golden_scaled():
    """104 nodes: the ragged tile (nodes 64 .. 103) of the in6_out1 golden scaled by 1.004, under the goldens' 1e-5 + GRAD_GAP."""
    g64, g32 = SI.golden_case("in6_out1")
    g = dict(g32)
    g["node_emb"] = g32["node_emb"].clone()
    g["node_emb"][64:] *= 1.004
    return g, g64, g32, dict(input_dim=3), 1e-5 + SI.GRAD_GAP


def _pair_eval(i):
    import regtgcn_amd as R
    n, t, f = SP.KERNEL_PAIR_SHAPES[i]
    ei, ea, x, w0, w1, b, ds = SP.kernel_pair_inputs(R, n, t, f)
    ref, g64, g32, allow = SP.embed_case(x, ei, ea, w0, w1, b, None, ds)
    # what _check allows each element today: TOL x the sum of the absolute terms + the ReLU allowance + 1e-6
    old = {k: (SP.TOL * bnd + alw + 1e-6).numpy() for k, bnd, alw in zip(SP.EMBED_NAMES, ref[2], ref[3])}
    return (ei, ea, x, w0, w1, b, ds), g64, g32, allow, old


def _lins1_without_one_node():
    (ei, ea, x, w0, w1, b, ds), g64, g32, allow, old = _pair_eval(2)                       # 1000 nodes, 6 periods, 8 features
    only = torch.zeros_like(ds)
    only[500] = ds[500]
    share = SP._embed_reference(x, ei, ea, w0, w1, b, None, only, dtype=torch.float32)[1][1]
    assert float(share.abs().max()) > 0
    g = dict(g32)
    g["gcn.lins.1.weight"] = g32["gcn.lins.1.weight"] - share
    return g, g64, g32, dict(allow=allow), old


def _lins0_accumulator_without_the_last_period():
    (ei, ea, x, w0, w1, b, ds), g64, g32, allow, old = _pair_eval(1)                       # 300 nodes, 12 periods, 32 features
    short = SP._embed_reference(x[:, :, :-1], ei, ea, w0, w1, b, None, ds, dtype=torch.float32)[1][0]
    g = dict(g32)
    g["gcn.lins.0.weight"] = g32["gcn.lins.0.weight"].clone()
    g["gcn.lins.0.weight"][:, 16:] = short[:, 16:]
    return g, g64, g32, dict(allow=allow), old


def _old_elementwise(got, want, bound):
    ok = True
    for k, w in want.items():
        off = int(((got[k].double() - w).abs().numpy() > bound[k]).sum())
        if off:
            print(f"  old bar: {k}: {off} of {w.numel()} elements off")
            ok = False
    return ok


# (corruption, does the comparison the GPU tests make today accept it?) -- the second column is what it DOES, recorded
CORRUPTIONS = [
    (_tn_beta_scaled, True),                                  # scale 7.6e-5: a tenth of it is under 1e-5
    (_sn_gamma_without_one_batch_element, False),             # one of TWO elements is half the gradient: 15 of 16 entries above 1e-5
    (_gate_conv_tap_sign_flipped, False),                     # a flipped sign is twice the entry: 750 of 1536 entries above 1e-5
    (_node_emb_wrong_in_the_ragged_tile, False),
    (_node_emb_ragged_tile_of_the_golden_scaled, True),       # scale 2e-3: 0.4 % of it is under 1e-5
    (_lins1_without_one_node, False),
    (_lins0_accumulator_without_the_last_period, False),
]


@pytest.mark.parametrize("corrupt,old_bar_accepts", CORRUPTIONS, ids=[c.__name__.lstrip("_") for c, _ in CORRUPTIONS])
def test_corrupted_gradients_fail_the_bar(corrupt, old_bar_accepts):
    g, g64, g32, kw, old = corrupt()
    assert_grads_conditioned(g32, g64, g32, K_GAP, REL, "uncorrupted", **kw)
    with pytest.raises(AssertionError, match="off their own scale"):
        assert_grads_conditioned(g, g64, g32, K_GAP, REL, corrupt.__name__, **kw)
    if isinstance(old, dict) and isinstance(next(iter(old.values())), np.ndarray):
        accepted = _old_elementwise(g, g64, old)
    else:
        accepted = _old_bar_accepts(g, g64, old)
    print(f"  {corrupt.__name__}: the old bar {'accepts' if accepted else 'rejects'} it")
    assert accepted == old_bar_accepts
