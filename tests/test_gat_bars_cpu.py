"""Host proof of tests/gat_math.py: the bars are 4 x the fp32 restatement's worst r over CASES rounded up to a power of two, the
inputs keep the leaky-relu ambiguity under its cap (from float64 alone), CASES reaches every lane group with a full and a padded
group and every edge the table promises, the exact facts hold in the restatement, and planted corruptions of the restatement
exceed the bar of the class they are aimed at by at least 2 x."""
import numpy as np
import pytest

import gat_math as G


@pytest.fixture(scope="module")
def table():
    """{case name: (inputs, pattern, reference, restatement, {class: r})}; the grid-stride case on its stated subset of rows."""
    out = {}
    for c in G.CASES:
        inp = G.inputs(c)
        pat = G.cpu_pattern(inp.ei, c.n)
        rows, src_rows = G.case_rows(c, pat)
        ref = G.reference(inp, pat, rows, src_rows)
        got = G.restate(inp, pat, rows, src_rows)
        if c.kind == "stride":
            inp = None                          # 270 MB: the corruption test rebuilds it
        out[c.name] = (inp, pat, ref, got, {k: v[0] for k, v in G.ratios(ref, got).items()})
    return out


def test_bars_are_four_times_the_worst_restatement_rounded_up(table):
    for cls in G.CLASSES:
        name, worst = max(((n, t[4][cls]) for n, t in table.items()), key=lambda p: p[1])
        print(f"{cls}: worst restatement r {worst:.3e} ({name}, {G.kernel_name(G.CASE[name].f)}) -> bar {G.BAR[cls]:.3e}")
        assert worst <= G.BAR[cls], (cls, name, worst)
        assert G.BAR[cls] == G.bar_from(worst), (cls, name, worst)
    assert set(G.BAR) == set(G.CLASSES)


def test_ambiguity_cap_from_float64_alone(table):
    for name, (_, _, ref, _, _) in table.items():
        rows = G.ambiguous_rows(ref)
        assert rows <= G.AMBIGUOUS_ROWS_CAP * ref["rows"].size, (name, rows)
        if G.CASE[name].small:
            assert rows == 0, (name, rows)
            assert not ref["dd_allow"].any() and not ref["ds_allow"].any()


def test_cases_reach_every_group_full_and_padded_and_every_edge(table):
    forms = {(G.expected_group(c.f), G.group_form(c.f)) for c in G.CASES}
    assert forms == {(g, s) for g in (2, 4, 8, 16, 32, 64) for s in ("full", "padded")}
    assert [G.expected_group(f) for f in (4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256)] == [2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    for t in G.GENERAL_T:
        assert {c.f for c in G.CASES if c.kind == "general" and c.t == t} == set(G.GENERAL_F)
    for f in G.HUB_F:
        _, pat, _, _, _ = table[f"hub F {f}"]
        assert int(np.diff(pat[0]).max()) >= 5000 and int(np.diff(pat[2]).max()) >= 5000
    # grid stride: more rows than one pass of the capped grid covers, and the stated rows sit on both sides of the seam
    c = G.CASE["grid stride"]
    first = G.GRID_CAP * (256 // G.expected_group(c.f))
    assert c.n * c.t > first
    rows = table[c.name][2]["rows"]
    for lo in (0, first - G.STRIDE_BLOCK, first, c.n * c.t - G.STRIDE_BLOCK):
        assert np.isin(np.arange(lo, lo + G.STRIDE_BLOCK), rows).all()
    assert np.isin(np.arange(0, c.n * c.t, G.STRIDE_EVERY), rows).all()
    # the features of the small graph: a duplicate, a dropped listed self loop, two rows with the self loop alone
    inp, pat, ref, _, _ = table["general F 12 T 3"]
    rp, col = pat[0].astype(np.int64), pat[1].astype(np.int64)
    assert sorted(col[rp[11]:rp[12]]).count(3) == 2 and list(col[rp[5]:rp[6]]).count(5) == 1
    assert list(np.diff(rp)[-2:]) == [1, 1] and int(col[-1]) == inp.n - 1
    assert list(np.diff(pat[2].astype(np.int64))[-2:] > 1) == [True, False]      # the last node sends no edge, the one before does
    single = table["single node"]
    assert single[1][0].tolist() == [0, 1] and single[1][1].tolist() == [0]


def test_score_regimes_along_the_hub_row(table):
    """Float64 scores of the hub's CSR row (period 0), in order."""
    def hub_raw(name):
        ref = table[name][2]
        return ref["raw"][ref["start"][0]:ref["start"][1]], ref["alpha"][ref["start"][0]:ref["start"][1]]
    raw, _ = hub_raw("scores ascending")
    assert raw.size == G.REGIME_HUB + 1 and (np.diff(raw) > 0).all() and 59 < raw[-1] < 62
    raw, _ = hub_raw("scores descending")
    assert (np.diff(raw) < 0).all() and 59 < raw[0] < 62
    raw, _ = hub_raw("scores equal")
    assert (raw == raw[0]).all()
    raw, alpha = hub_raw("scores gap")
    big = int(np.argmax(raw))
    assert big == G.GAP_SOURCE - 1 and raw[big] - np.delete(raw, big).max() > 118
    assert np.float32(np.exp(np.float32(-(raw[big] - np.delete(raw, big).max())))) == 0 and 1 - alpha[big] < 1e-40
    raw, _ = hub_raw("scores negative")
    assert (raw < 0).all() and (np.diff(raw) < 0).all() and raw[-1] < -59
    raw, alpha = hub_raw("scores zero")
    assert (raw == 0).all() and np.allclose(alpha, 1.0 / raw.size, rtol=1e-15)


def test_exact_facts_hold_in_the_restatement(table):
    for name, (inp, pat, ref, got, _) in table.items():
        c = G.CASE[name]
        if not c.small:
            continue
        x = inp.x.reshape(-1, c.f)
        lone = np.nonzero(np.diff(ref["start"]) == 1)[0]
        assert lone.size == (1 if c.kind == "single" else 2 * c.t), name
        assert np.array_equal(got["out"][lone], x[lone]) and (got["l"][lone] == 1).all() and (got["dd"][lone] == 0).all(), name
        assert (ref["dd"][lone] == 0).all()
        only_self = lone[np.diff(pat[2].astype(np.int64))[lone // c.t] == 1]          # the last node sends no edge either
        assert only_self.size == c.t and (got["ds"][only_self] == 0).all() and (ref["ds"][only_self] == 0).all(), name
    inp, _, ref, got, _ = table["scores zero"]
    assert (got["m"] == 0).all() and (got["d"] == 0).all() and (ref["m"] == 0).all()
    inp, _, ref, got, _ = table["scores gap"]
    hub = np.arange(inp.t)                                       # rows of node 0
    assert np.array_equal(got["out"][hub], inp.x[G.GAP_SOURCE]) and (got["l"][hub] == 1).all() and (got["dd"][hub] == 0).all()


# (corruption, cases that must show it): the class is gat_math.CORRUPTIONS[corruption]
PLANTED = [("acc_rescale", ("scores ascending",)), ("final_max", ("scores ascending", "general F 16 T 1")),
           ("D_zero", ("general F 32 T 3", "hub F 132")), ("slope_pos", ("general F 64 T 1", "scores descending")),
           ("skip_last_long", ("general F 128 T 1", "hub F 32")), ("stats_next", ("general F 8 T 3", "hub F 32")),
           ("drop_lane", ("general F 4 T 1", "general F 12 T 3", "general F 20 T 1", "general F 36 T 3", "general F 68 T 1",
                          "general F 132 T 3")),
           ("stale_dsd", ("grid stride",))]


@pytest.mark.parametrize("corrupt,names", PLANTED, ids=[p[0] for p in PLANTED])
def test_planted_corruptions_exceed_their_bar_twice(table, corrupt, names):
    cls = G.CORRUPTIONS[corrupt]
    for name in names:
        c = G.CASE[name]
        inp, pat, ref, _, clean = table[name]
        inp = G.inputs(c) if inp is None else inp
        bad = G.ratios(ref, G.restate(inp, pat, ref["rows"], ref["src_rows"], corrupt=corrupt))
        print(f"{corrupt} on {name}: {cls} r = {bad[cls][0]:.3e} (clean {clean[cls]:.3e}, bar {G.BAR[cls]:.3e})")
        assert bad[cls][0] >= 2 * G.BAR[cls], (corrupt, name, bad[cls][0])
    assert set(G.CORRUPTIONS) == {p[0] for p in PLANTED}


def test_end_to_end_statistic_sees_swapped_columns(table):
    """du = dsd^T x of the restatement (the product in float64: the weight-gradient kernel has its own bar) is inside the end-to-end
    bar less the weight gradient's share.  That bar is the sum of the per-row bars, every row at its worst and with one sign, so it
    is loose by construction (a wrong slope on every entry is barely over it: the per-row bars are what sees arithmetic); what it
    is there for is the way from dsd to (du_src, du_dst) -- the two columns exchanged are outside twice the bar."""
    import op_bars
    for name in G.DU_CASES:
        c = G.CASE[name]
        inp, _, ref, got, _ = table[name]
        x = inp.x.reshape(-1, c.f).astype(np.float64)
        du_s, du_d = got["ds"].astype(np.float64) @ x, got["dd"].astype(np.float64) @ x
        clean = G.du_ratios(ref, inp, du_s, du_d)
        assert clean["ds"] <= G.BAR["ds"] and clean["dd"] <= G.BAR["dd"], (name, clean)
        bad = G.du_ratios(ref, inp, du_d, du_s)
        print(f"{name}: du r clean {clean}, columns exchanged {bad}")
        assert bad["ds"] >= 2 * (G.BAR["ds"] + op_bars.BAR["wgrad"]) and bad["dd"] >= 2 * (G.BAR["dd"] + op_bars.BAR["wgrad"]), (name, bad)


def test_statistic_rules():
    z = np.zeros(3)
    assert G._worst(z, z) == (0.0, 0)
    e = z.copy()
    e[2] = 1e-300
    assert G._worst(e, z) == (float("inf"), 2)                  # a denominator of 0 demands an exact 0
    assert G._worst(np.array([0.0, np.nan]), np.ones(2))[0] == float("inf")
    assert G._worst(np.array([1.0, 4.0]), np.array([2.0, 2.0])) == (2.0, 1)
