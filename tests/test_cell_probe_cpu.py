"""Host checks of tests/cell_probe.py: the float64 restatement is the oracle's cell, the probes isolate what they claim, the bars are
what the fp32 restatement gives, the table reaches every form of the dispatch restatement, and planted corruptions are caught."""
import os

import numpy as np
import pytest
import torch

import cell_probe as P
import op_bars as B
from conftest import load_npz
from oracle import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ("M129-T3", "M132-T12", "M144-T48")


def test_float64_restatement_reproduces_the_cell_golden():
    """golden_cell.npz (the reference's own TGCN cell): T = 1, attention probability 1, hidden = the cell's output."""
    g = load_npz("golden_cell.npz")
    q = "tgnn._base_tgcn."
    p = {q + k[3:].replace("__", "."): torch.from_numpy(v).double() for k, v in g.items() if k.startswith("p__")}
    x, h = torch.from_numpy(g["x"]), torch.from_numpy(g["h"])
    n, c = h.shape
    p.update({"tgnn.conv.bias": torch.zeros(c, dtype=torch.float64), "tgnn.conv.lins.0.weight": torch.zeros(c, x.shape[1], dtype=torch.float64),
              "tgnn.conv.lins.1.weight": torch.zeros(c, x.shape[1], dtype=torch.float64), "linear1.weight": torch.zeros(4, c, dtype=torch.float64),
              "linear1.bias": torch.zeros(4, dtype=torch.float64), "linear2.weight": torch.zeros(1, 4, dtype=torch.float64),
              "linear2.bias": torch.zeros(1, dtype=torch.float64)})
    ei = torch.from_numpy(g["edge_index"])
    for tag, w in (("unit", None), ("weighted", torch.from_numpy(g["edge_weight"]))):
        ax = P.aggregate64(P.csr_of(ei, w, n), x[:, :, None])
        _pred, hidden = P.cell(p, ax, h.double(), torch.zeros(1, dtype=torch.float64), torch.float64)
        np.testing.assert_allclose(hidden.numpy(), g[f"out_{tag}"], atol=2e-6)


@pytest.mark.parametrize("name", ["M7-T1", "M129-T3", "M132-T12"])
@pytest.mark.parametrize("probe", ["full", "saturated"])
def test_float64_restatement_is_the_oracle_cell_under_autograd(name, probe):
    """oracle.model.tgcn_cell per period, attention sum and head in float64 against the restatement on the same operator (normalised
    in float64 for both): outputs and the gradient of the hidden input agree at float64 rounding."""
    n, _e, _f, t, c, _o, _ = P.CASES[name]
    p = {k: v.double() for k, v in P.params(name, probe).items()}
    x, h_in, gh, gp = P.inputs(name, probe)
    ei, ew = P.graph(name)
    h = h_in.double().requires_grad_(True)
    probs = torch.softmax(p["tgnn._attention"], dim=0)
    hv = h.view(n, t, c)
    hidden = sum(probs[k] * M.tgcn_cell(p, "tgnn._base_tgcn.", x[:, :, k].double(), ei, ew.double(), hv[:, k]) for k in range(t))
    pred = M.head(p, hidden)
    ((hidden * gh.double()).sum() + (pred * gp.double()).sum()).backward()
    ax = P.aggregate64(_csr64(ei, ew, n), x)
    h2 = h_in.double().requires_grad_(True)
    pred2, hidden2 = P.cell(p, ax, h2, p["tgnn._attention"], torch.float64)
    ((hidden2 * gh.double()).sum() + (pred2 * gp.double()).sum()).backward()
    for a, b in ((hidden2.detach(), hidden.detach()), (pred2.detach(), pred.detach()), (h2.grad, h.grad)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def _csr64(ei, ew, n):
    from oracle import graph_ops as G
    src, dst, w = G.gcn_norm_edges(ei, ew, n, torch.float64)
    order = torch.argsort(dst, stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
    return rowptr.int(), src[order].int(), w[order].contiguous()


@pytest.mark.parametrize("name", SMALL)
def test_probes_isolate(name):
    t, c = P.CASES[name][3], P.CASES[name][4]
    r = {probe: P.reference(name, probe) for probe in ("blend", "candidate", "gates")}
    assert float(r["gates"]["r32"]["drp"].abs().max()) == 0.0 and float(r["gates"]["r32"]["dq"].abs().max()) == 0.0
    assert float(r["candidate"]["r32"]["gate"].abs().max()) == 0.0
    assert float(r["candidate"]["r32"]["dq"].abs().max()) > 0.0 and float(r["gates"]["r32"]["gate"].abs().max()) > 0.0
    # blend in float64: dh_in is dhn * z, one product per element, exactly
    ref = r["blend"]
    p = {k: v.double() for k, v in P.params(name, "blend").items()}
    _x, _h, gh, gp = P.inputs(name, "blend")
    pa, want = ref["parts"], ref["want"]
    d1 = (gp.double() @ p["linear2.weight"]) * (pa["y1"] > 0)
    doh = (d1 @ p["linear1.weight"]) * (want["hidden"] > 0) + gh.double()
    n = doh.shape[0]
    dhn = (pa["probs"].view(1, t, 1) * doh.view(n, 1, c)).expand(n, t, c).reshape(n * t, c)
    assert torch.equal(want["dh_in"], dhn * pa["z"])
    assert float(ref["r32"]["gate"].abs().max()) == 0.0 and float(ref["r32"]["dq"].abs().max()) == 0.0


def test_saturated_probe_reaches_60_in_both_signs_and_stays_finite():
    for name in P.CASES:
        ref = P.reference(name, "saturated")
        for k in ("pz", "pr", "ph"):
            assert float(ref["parts"][k].min()) <= -60.0 and float(ref["parts"][k].max()) >= 60.0, (name, k)
        for k, v in ref["r32"].items():
            assert bool(torch.isfinite(v).all()), (name, k)
        z = ref["r32"]["z"]
        assert bool(((z * (1.0 - z)) == 0).any()), name              # z (1 - z) is exactly 0 somewhere
        assert float(ref["parts"]["y1"].min()) > 0.1                 # the head's inner relu is open


def test_bar_table_is_what_the_restatement_gives_and_rows_are_well_conditioned():
    table = P.bar_table()
    print(table)
    for k in P.CLASSES:
        assert B.bar_from(table[k][0]) == P.BAR[k], (k, table[k], P.BAR[k])
        assert P.BAR[k] <= P.CAP
    edge = 0
    for name in P.CASES:
        for probe in P.PROBES:
            ref = P.reference(name, probe)
            assert float(ref["parts"]["y1"].min()) > 0.1, (name, probe)
            edge += int(ref["want"]["edge_nodes"].numel())
            for tensor in ("hidden", "pred", "dh_in"):
                ill = P.ill_rows(ref, tensor)
                if probe == "saturated":
                    assert float(ill.float().mean()) <= 0.05, (name, tensor, int(ill.sum()))
                else:
                    assert not bool(ill.any()), (name, probe, tensor, int(ill.sum()))
    nodes = sum(c[0] for c in P.CASES.values()) * len(P.PROBES)
    assert edge <= 0.05 * nodes, (edge, nodes)                      # the named relu-edge nodes stay a small share too


def test_case_table_reaches_every_form():
    reached = P.table_forms()
    for mode in P.MODES:
        for k, names in P.FORM_NAMES[mode].items():
            assert names <= reached[mode][k], (mode, k, sorted(names - reached[mode][k]))
    ms = {c[0] * c[3] for c in P.CASES.values()}
    assert {7, 129, 132} <= ms and max(ms) == 8196
    assert {c[3] for c in P.CASES.values()} >= {1, 3, 12, 48, 255} and P.CASES["M510-T255"][0] == 2
    assert {c[4] for c in P.CASES.values()} == {128, 132, 256} and {c[2] for c in P.CASES.values()} == {7, 8, 32}
    assert {c[5] for c in P.CASES.values()} == {1, 3}
    ei, _ = P.graph("M132-T12")
    assert int(ei[1].max()) < P.CASES["M132-T12"][0] - 2
    # the switch is run both ways exactly where it changes the form
    assert [name for name in P.CASES if len(P.runs(name)) == 4] == ["M8196-T12"]


def test_restated_flow_is_the_recorded_launch_plan_of_the_cell_path():
    """tests/golden/step_plan.txt, case 18: the launch sequence of regt_cell_forward + regt_cell_backward (recorded with the
    generated-operand predicate true)."""
    with open(os.path.join(ROOT, "tests", "golden", "step_plan.txt")) as f:
        lines = f.read().splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith("case 18_cell"))
    names = []
    for ln in lines[start + 1:]:
        if ln.startswith("case ") or ln.startswith("stages "):
            break
        names.append(ln.split()[2])
    assert names == P.cell_launches(gen=True)
    two = P.cell_launches(gen=False)
    assert "launch_cell_bwd" in two and "launch_gemm_dgrad1" in two and "launch_gemm_dgrad1_gen" not in two


def _corrupted(name, probe, cor):
    ref = P.reference(name, probe)
    x, h, gh, gp = P.inputs(name, probe)
    out = P.cell32(P.params(name, probe), P.aggregate64(P.cpu_csr(name), x).float(), h, gh, gp, corrupt=cor)
    worst = 0.0
    for tensor in ("hidden", "pred", "dh_in"):
        err, scale = P.ref_rows(out[tensor], ref, tensor)
        worst = max(worst, float(P.row_ratio(err, scale).max()) / P.BAR[P.klass(tensor, probe)])
    return worst


@pytest.mark.parametrize("cor,name,probe", [
    ("uh-tail", "M129-T3", "candidate"),                 # C = 132: the tail is 4 of 132 k
    ("r-next-row", "M132-T12", "candidate"),
    ("one-minus-ht", "M144-T48", "candidate"),
    ("drop-blend-last-period", "M132-T12", "blend"),
    ("dzp-uz-twice", "M129-T3", "gates"),
])
def test_planted_corruption_exceeds_its_bar(cor, name, probe):
    over = _corrupted(name, probe, cor)
    print(f"{cor} on {name} {probe}: {over:.3g} x bar; on full: {_corrupted(name, 'full', cor):.3g} x bar")
    assert over >= 2.0
    assert _corrupted(name, "full", cor) >= 2.0


def test_exp_in_place_of_the_fast_forms_does_not_trip_full():
    """The negative control: expf-based sigmoid / tanh differ from the kernels' exp2 sequences by rounding alone (1e-7 of an
    element); a bar that this tripped on ``full`` would be too tight to be honest.  (It stays under every bar of every probe: the
    figures are printed.)"""
    for name in SMALL:
        for probe in P.PROBES:
            over = _corrupted(name, probe, "exp")
            print(f"exp on {name} {probe}: {over:.3g} x bar")
            if probe == "full":
                assert over <= 1.0, (name, over)
