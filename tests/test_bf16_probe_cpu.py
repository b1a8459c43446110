"""Host checks of tests/bf16_probe.py: the bars are what the references give, the references alone decide conditioning, the case table
reaches every bf16 form of the restated dispatch twice, and planted corruptions leave their bar behind by 4 x at the affected node."""
import os
import re

import pytest
import torch

import bf16_probe as P
import fused_math as FM
import op_bars as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bar_table_is_what_the_references_give():
    table = P.bar_table()
    print(table)
    for k in P.CLASSES:
        assert table[k][0] > 0.0, k
        assert B.bar_from(table[k][0]) == P.BAR[k], (k, table[k], P.BAR[k])
        assert P.BAR[k] <= P.CAP[k]
    assert P.ORDER_FACTOR == B.ORDER_FACTOR == 4.0


@pytest.mark.parametrize("name", list(P.CASES))
def test_references_alone_call_few_rows_and_tensors_ill_conditioned(name):
    share = P.ill_share(name)
    print(name, {k: v[:2] for k, v in share.items()}, share["tensors"][2])
    for key in ("rows", "tensors"):
        ill, total, _labels = share[key]
        assert ill <= 0.05 * total, (name, key, ill, total)
    assert share["dense"][0] == 0, share["dense"][2]              # (tgnn._attention apart: a class of its own)


@pytest.mark.parametrize("name", list(P.CASES))
def test_no_relu_of_a_case_depends_on_a_rounding(name):
    """The embedding's leaky relu (PRE_SHIFT) and the head's inner relu (linear1.bias + 1) in float64: every element well on its side."""
    ei, ew, ri, rw = P.graph(name)
    n = P.CASES[name][1]
    p = {k: v.double() for k, v in P.params(name).items()}
    a, ls = FM.dense_ops(ei, None if ew is None else ew.double(), ri, [w.double() for w in rw], n, torch.float64)
    seen = {}

    def tap(key, v):
        seen[key] = v.detach()
        return v

    pred, hidden = FM.forward_fused(p, P.inputs(name)[0].double(), a, ls, regional=P.regional(name), tap=tap)
    assert float((seen["y1"] + p["linear1.bias"]).min()) > 0.1
    if P.regional(name):
        assert float(seen["pre"].abs().min()) > 1.0
        assert bool((seen["pre"] > 0).any()) and bool((seen["pre"] < 0).any())            # both slopes of the leaky relu
    # and the restatement under the taps is the oracle
    ref = P.reference(name)["want"]
    assert float((hidden - ref["hidden"]).abs().max()) <= 1e-10 and float((pred - ref["pred"]).abs().max()) <= 1e-10


def test_emulation_without_rounding_is_the_oracle_and_its_gradients():
    """The autograd functions of the emulation change roundings only: with the rounding taken out they give the float64 oracle's
    outputs and gradients at fp32 accuracy."""
    name = "R-F32-T7"
    ei, ew, ri, rw = P.graph(name)
    n = P.CASES[name][1]
    p = {k: v.clone().requires_grad_(True) for k, v in P.params(name).items()}
    a, ls = FM.dense_ops(ei, ew, ri, rw, n, torch.float32)
    keep, FM.bf16_round = FM.bf16_round, (lambda v: v)
    try:
        pred, hidden = FM.forward_fused(p, P.inputs(name)[0], a, ls, regional=True, rnd=P._Rnd.apply, store=P._Rnd.apply, tap=P._emu_tap, ops=P.EMU_OPS)
        grads = P._grads(pred, hidden, p, name)
    finally:
        FM.bf16_round = keep
    want = P.reference(name)["want"]
    assert float((hidden.detach() - want["hidden"]).abs().max()) <= 1e-5 * float(want["hidden"].abs().max())
    for label, gs in grads.items():
        for k, g in gs.items():
            w = want["grads"][label][k]
            assert (g is None) == (w is None), (label, k)
            if w is not None:
                assert float((g - w).abs().max()) <= 2e-4 * float(w.abs().max()) + 1e-12, (label, k)


def test_zero_gradients_of_the_references():
    """The probe on the node without in-edge has gp = 0: linear1 / linear2 have gradient exactly 0 in float64 and in the emulation."""
    found = 0
    for name in P.CASES:
        if "no-in-edge" not in P.probe_nodes(name):
            continue
        ref = P.reference(name)
        for k in ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias"):
            assert float(ref["want"]["grads"]["no-in-edge"][k].abs().max()) == 0.0
            assert float(ref["emu"][0]["grads"]["no-in-edge"][k].abs().max()) == 0.0
            found += 1
    assert found >= 4 * 8


def test_case_table_is_what_the_issue_asks_for():
    t = {c[5] for c in P.CASES.values()}
    assert {1, 3, 5, 7, 12, 48} <= t and {c[4] for c in P.CASES.values()} == {32, 64}
    assert any((c[5] * c[4]) % 64 != 0 and c[0] == "RegionalTemporalGCN" for c in P.CASES.values())
    for name, (model, n, e, sizes, f, t_, o) in P.CASES.items():
        assert n <= 700
        m = n * t_
        assert m % 128 != 0 and m > 128, name                                    # a partial last tile behind a full one
        nodes = P.probe_nodes(name)
        assert nodes["node0"] == 0 and (n - 1) in nodes.values() and (n - 2) in nodes.values() and 128 // t_ in nodes.values()
        s = nodes.get("row128", 0) if "row128" in nodes else 128 // t_
        if t_ > 1:
            assert s * t_ < 128 < s * t_ + t_, name                              # that node's rows straddle row 128
        ei, _ew, ri, _rw = P.graph(name)
        assert int(ei[1].max()) < n - 2 and bool((ei[0] != ei[1]).all())         # no edge into the last two nodes
        if sizes:
            assert len(set(sizes)) == len(sizes) and len(sizes) in (2, 3)
            owner = torch.full((n,), -1, dtype=torch.long)
            for r, e_r in enumerate(ri):
                assert e_r.shape[1] > 0 and bool((owner[e_r[1]] < 0).all())     # no node receives edges in two regions
                owner[e_r[1].unique()] = r
            have = owner >= 0
            assert bool(have[P.region_bounds(name)[1]])                         # the first node of the second region owns in-edges
            assert torch.equal(owner[have], P.node_region(name)[have])          # node-disjoint regions, ids non-decreasing by node
            assert nodes.get("region1", P.region_bounds(name)[1]) == P.region_bounds(name)[1]
    assert P.CASES["R-F64-T48"][1] * 48 > 128 and 48 < 64 < 96                   # node 1 of the T = 48 cases spans the 64-row halves


def test_every_bf16_form_is_reached_by_two_cases():
    for pred, what in P.FORMS:
        hit = [name for name in P.CASES for key in P.runs(name) if pred(P.expected_forms(name, P.OPTION_SETS[key]), P.OPTION_SETS[key])]
        assert len(set(hit)) >= 2, (what, hit)
    assert all(P.runs(name) == ["default"] for name in P.CASES if not P.regional(name))
    assert P.runs("R-F64-T12") == list(P.OPTION_SETS)
    assert P.runs("R-F32-T7") == ["default", "fused_bwd0", "fused_rows0"]       # no row layout to switch off
    assert "fused_rows0" not in P.runs("R-F64-T48")                              # T > 16: the 64-row kernel either way


def test_expected_forms_restates_the_host_predicates():
    f = P.expected_forms
    d = f("R-F64-T12")
    assert d == {"rows": 1, "forward": "fused_rows_kernel", "weights": "fragment-order bf16", "backward": "fused_bwd_kernel", "node_sum_rows": 16}
    assert f("R-F64-T12", {"fused_rows": 0})["forward"] == "fused_fwd_kernel" and f("R-F64-T12", {"fused_rows": 0})["node_sum_rows"] == 64
    assert f("R-F64-T48")["forward"] == "fused_fwd_kernel"                                       # T <= 16 fails
    assert f("R-F32-T7")["rows"] == 0 and f("R-F32-T7")["backward"] == "fused_bwd_kernel"        # (T F) % 64 != 0; the backward does not care
    assert f("R-F64-T5")["rows"] == 1 and f("R-F32-T12")["rows"] == 1
    for opts in ({"xbf": 0}, {"no_rows_flag": 1}):
        assert f("R-F64-T12", opts)["rows"] == 0 and f("R-F64-T12", opts)["forward"].startswith("embedding + gates + candidate")
    assert f("R-F64-T12", {"fused_bwd": 0})["backward"].startswith("cell_bwd8")
    t = f("T-F64-T5")
    assert t["rows"] == 0 and t["weights"] == "fp32 [N][K]" and t["backward"].startswith("cell_bwd8") and t["node_sum_rows"] == 64
    # a shape outside the fused kernels' (C = 256, F = 32 / 64) keeps the rows fp32; one region has no region table to select from
    assert f(("RegionalTemporalGCN", 100, 1, (50, 50), 16, 12, 1))["rows"] == 0
    assert f(("RegionalTemporalGCN", 100, 1, (100,), 64, 12, 1))["rows"] == 0
    # the predicates this restates are where the docstring says they are
    with open(os.path.join(ROOT, "regt-gcn_amd", "csrc", "api_step.hip")) as fh:
        src = fh.read()
    for needle in ("fused_forward_ok(d.C, d.F) && ((long)d.T * d.F) % 64 == 0", "d.regional && d.R > 1 && !g.overlap",
                   "f.wfr = f.abf && weights_frag(d) && d.regional", "f.wfr && !b.ext && fused_backward_ok(C) && fused_bwd_wanted()",
                   "a.node_sum_rows = abf && fused_rows_form(d, g) ? 16 : 64", "REGT_DIMS_NO_BF16_ROWS) && option(OPT_XBF)"):
        assert needle in src, needle
    with open(os.path.join(ROOT, "regt-gcn_amd", "csrc", "fused_rows.hip")) as fh:
        assert re.search(r"fused_forward_rows_ok\(int C, int F, int T\) \{ return C == FR_C && \(F == 64 \|\| F == 32\) && T <= 16; \}", fh.read())


@pytest.mark.parametrize("cor,name", [
    ("k-slab", "R-F64-T12"), ("k-slab", "T-F64-T5"),
    ("swap-rows", "R-F64-T1"), ("swap-rows", "T-F64-T1"),
    ("zero-last-row", "R-F64-T5"), ("zero-last-row", "T-F64-T5"),
    ("neighbour-period", "R-F64-T5"), ("neighbour-period", "T-F64-T5"),
    ("half-wave-period", "T-F64-T3"), ("half-wave-period", "T-F64-T1"),
])
def test_planted_corruption_exceeds_its_bar_fourfold(cor, name):
    over, where = P.corruption_excess(name, cor)
    print(f"{cor} on {name}: {over:.3g} x bar at {where}")
    assert over != float("inf"), where                   # (a finite margin: not the exact-zero rule)
    assert over >= 4.0, (cor, name, over, where)
    # and the clean emulation is inside every bar at that node: the margin is the corruption's
    label, node = P.corruption_site(name, cor)
    ref = P.reference(name)
    assert not P.held_grads(ref["emu"][0]["grads"][label], ref, 0, label)[2]
    assert not P.held_rows(ref["emu"][0]["hidden"], ref, 0, "hidden")[2]
