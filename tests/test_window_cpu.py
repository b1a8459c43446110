"""tests/window_math.py proves itself on the CPU: a correct ``linear`` written in torch against raw Window views passes every check
in every layout, and five planted defects are each caught by the check meant for them -- so what tests/test_gpu_windows.py
demands is a demand on the kernels, not an artefact of the harness.  Also: for every case listed there the fp32 CPU evaluation
of the reference meets the case's own bar against float64, i.e. the bars can be met.

(A NaN computed from poisoned words may carry their payload, so a leaked read can also look like an unwritten element; the
checks are therefore evaluated one by one here, not as a first-failure verdict.)"""
import pytest
import torch

import window_math as WM
from gru_math import rel_err

SHAPE = (37, 10, 9)             # (M, N, K): nothing a multiple of 4


def _raw(win, rows, cols):
    """rows x cols floats from the window's origin, whatever the window's own extent: what a kernel with a wrong bound touches."""
    return win.buf.view(torch.float32).as_strided((rows, cols), (win.ld, 1), win.front)


def _operands(layout):
    m, n, k = SHAPE
    a, w, b = WM.linear_inputs(m, n, k)
    wins = {"A": WM.make(layout, "a", m, k, a), "W": WM.make(layout, "in", n, k, w), "bias": WM.make(layout, "out", 1, n, b, strided=False),
            "out": WM.make(layout, "out", m, n)}
    return wins, WM.ref_linear(a, w, b, 0, torch.float64)


def _correct(wins):
    wins["out"].view.copy_(wins["A"].view @ wins["W"].view.t() + wins["bias"].view)


def _past_column(wins):
    _correct(wins)
    m, n, _ = SHAPE
    row = m - 1 if wins["out"].ld == n else 3        # dense rows follow one another: only the last row's overrun leaves the window
    _raw(wins["out"], m, n + 1)[row, n] = 1.0


def _past_row(wins):
    _correct(wins)
    m, n, _ = SHAPE
    _raw(wins["out"], m + 1, n)[m] = 2.0


def _unwritten(wins):
    _correct(wins)
    wins["out"].bits[5, 2] = WM.POISON


def _reads_column_k(wins):
    m, n, k = SHAPE
    wins["out"].view.copy_(_raw(wins["A"], m, k + 1) @ _raw(wins["W"], n, k + 1).t() + wins["bias"].view)


def _zero_times_row_after_m(wins):
    m, n, k = SHAPE
    _correct(wins)
    wins["out"].view[m - 1] += 0.0 * (_raw(wins["A"], m + 1, k)[m] @ wins["W"].view.t())


def _checks(wins, ref64):
    """{check: passed} -- the three conditions of the GPU tests, each on its own."""
    res = {}
    for name, fn in (("untouched", lambda: [w.check_untouched(k) for k, w in wins.items()]),
                     ("written", lambda: wins["out"].check_written("out"))):
        try:
            fn()
            res[name] = True
        except AssertionError:
            res[name] = False
    _, tol = WM.gap_bar(WM.ref_linear(wins["A"].view, wins["W"].view, wins["bias"].view[0], 0, torch.float32), ref64)
    res["values"] = bool(rel_err(wins["out"].get(), ref64) <= tol)          # a NaN compares false
    return res


@pytest.mark.parametrize("layout", WM.LAYOUTS)
def test_layouts_are_what_they_claim(layout):
    wins, _ = _operands(layout)
    m, n, k = SHAPE
    for name, w in wins.items():
        assert w.buf.numel() == w.total and w.front >= 128 * w.ld and w.ld >= w.cols
        assert int((w.buf != WM.POISON).sum()) == (0 if w.output else w.rows * w.cols)
    forms = {name: WM.form_of(layout, role) for name, role in (("A", "a"), ("W", "in"), ("bias", "out"), ("out", "out"))}
    for name, w in wins.items():
        if forms[name] == "dense":
            assert w.ld == w.cols and w.col_off == 0 and w.aligned16()
        elif forms[name] == "padded16":
            assert w.col_off == 4 and w.aligned16() and (name == "bias" or (w.ld % 4 == 0 and w.ld == (w.cols + 3) // 4 * 4 + 8))
        else:
            assert w.col_off == 1 and not w.aligned16() and (name == "bias" or w.ld == w.cols + 3)
    assert {"dense": set(forms.values()) == {"dense"}, "padded16": set(forms.values()) == {"padded16"},
            "odd": set(forms.values()) == {"odd"},
            "odd_out": forms == {"A": "padded16", "W": "padded16", "bias": "odd", "out": "odd"},
            "odd_in": forms == {"A": "odd", "W": "padded16", "bias": "padded16", "out": "padded16"}}[layout]


@pytest.mark.parametrize("layout", WM.LAYOUTS)
def test_correct_kernel_passes_every_check(layout):
    wins, ref64 = _operands(layout)
    _correct(wins)
    assert _checks(wins, ref64) == {"untouched": True, "written": True, "values": True}


@pytest.mark.parametrize("layout", WM.LAYOUTS)
@pytest.mark.parametrize("kernel,want", [
    (_past_column, {"untouched": False, "written": True, "values": True}),
    (_past_row, {"untouched": False, "written": True, "values": True}),
    (_unwritten, {"untouched": True, "written": False}),
    (_reads_column_k, {"untouched": True, "values": False}),
    (_zero_times_row_after_m, {"untouched": True, "values": False})], ids=lambda v: v.__name__.strip("_") if callable(v) else "")
def test_planted_defect_is_caught_by_its_check(layout, kernel, want):
    wins, ref64 = _operands(layout)
    kernel(wins)
    got = _checks(wins, ref64)
    assert {k: got[k] for k in want} == want, got


def test_check_untouched_reports_the_position_relative_to_the_window():
    w = WM.Window(4, 5, ld=9, col_off=2)
    _raw(w, 4, 9)[2, 6] = 0.0
    with pytest.raises(AssertionError, match=r"\(row 2, col 6\)"):
        w.check_untouched("w")
    w = WM.Window(4, 5, ld=9, col_off=2)
    w.buf[w.front - 9 + 1] = 0                     # one row before the window
    with pytest.raises(AssertionError, match=r"\(row -1, col 1\)"):
        w.check_untouched("w")
    w.buf[w.front - 9 + 1] = WM.POISON
    w.check_untouched("w")
    w.view.fill_(float("nan"))                     # another NaN is not the poison: the comparison is on the bits
    w.check_written("w")


def _usable(gap, tol):
    assert gap == gap and gap < float("inf") and tol > 0.0
    assert gap > 0.0 or tol == 32.0 * 2.0 ** -24                 # non-degenerate: a measured gap, or the floor in force
    assert gap <= tol                                            # the fp32 reference itself is inside the bar


@pytest.mark.parametrize("m,n,k", WM.LINEAR_SHAPES)
def test_fp32_reference_meets_the_linear_bars(m, n, k):
    acts = (0, 1, 2, 3, 4) if (m, n, k) in WM.LINEAR_ACT_SHAPES else (0,)
    for rounded in (False, True):
        for with_bias in (True, False):
            for act in acts:
                ref64, gap, tol = WM.linear_refs(m, n, k, with_bias, act, rounded)
                assert bool(torch.isfinite(ref64).all())
                if act in (3, 4):
                    a, w, b = WM.linear_inputs(m, n, k)
                    if rounded:
                        a, w = WM.bf16_round(a), WM.bf16_round(w)
                    got = WM.ref_linear(a, w, b if with_bias else None, act, torch.float32)
                    assert float((got.double() - ref64).abs().max()) <= WM.ABS_ACT_BAR and float(ref64.abs().max()) <= 1.0
                else:
                    _usable(gap, tol)
    if k > 1:       # the two products a bf16-arithmetic result may match are far apart on the scale of the bar: no kernel meets both by accident
        r0, _, tol = WM.linear_refs(m, n, k, True, 0, False)
        assert rel_err(WM.linear_refs(m, n, k, True, 0, True)[0], r0) > 4 * tol


@pytest.mark.parametrize("m,n,k", WM.WGRAD_SHAPES)
def test_fp32_reference_meets_the_wgrad_bars(m, n, k):
    for rounded in (False, True):
        for ref64, gap, tol in WM.wgrad_refs(m, n, k, rounded):
            assert bool(torch.isfinite(ref64).all())
            _usable(gap, tol)


def test_fp32_reference_meets_the_spmm_bars():
    ei, val = WM.spmm_graph()
    n = 300
    order = torch.argsort(ei[1], stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.long)
    rowptr[1:] = torch.bincount(ei[1], minlength=n).cumsum(0)
    op = WM.csr_dense(rowptr, ei[0][order], val[order], n)
    want = torch.zeros(n, n, dtype=torch.float64).index_put_((ei[1], ei[0]), val.double(), accumulate=True)
    assert torch.equal(op, want)
    assert int((op[0] != 0).sum()) == 299 and float(op[200:].abs().max()) == 0.0            # the hub, the empty rows
    assert abs(float(op[9, 7]) - float(val[-1].double() + val[-2].double())) == 0.0        # the duplicate adds up
    for width in WM.SPMM_WIDTHS + WM.DUAL_WIDTHS:
        x = torch.randn(n, width, generator=torch.Generator().manual_seed(width))
        ref64 = WM.ref_spmm(op, x, torch.float64)
        _usable(*WM.gap_bar(WM.ref_spmm(op, x, torch.float32), ref64))
        assert float(ref64[200:].abs().max()) == 0.0


@pytest.mark.parametrize("f", WM.GAT_F)
@pytest.mark.parametrize("t", WM.GAT_T)
def test_fp32_reference_meets_the_gat_bars(f, t):
    c = WM.gat_case(f, t)
    n = WM.GAT_NODES
    cnt = WM.attention_counts(c["ei"], n)
    assert int((cnt[0] > 0).sum()) == n and float(cnt[n - 2:].sum()) == 2.0 and float(cnt[11, 3]) >= 2.0 and float(cnt[5, 5]) == 1.0
    assert float(c["raw"].max()) > 4.0 and float(c["raw"].min()) < -4.0 and abs(float(c["raw"].abs().max()) - 8.0) < 1e-3
    assert float((c["out32"].double() - c["out64"]).abs().max()) <= WM.GAT_OUT_BAR
    scale = max(1.0, float(c["dus64"].abs().max()), float(c["dud64"].abs().max()))
    for k in ("dus", "dud"):
        ok, ratio = WM.gat_grad_ok(c[k + "32"], c[k + "64"], scale)
        assert ok and ratio > 0.0, (k, ratio)
        assert float(c[k + "64"].abs().max()) > 0.0
    # the host contraction the GPU test uses for the score gradients is the chain rule of the dense formula: with exact per-row
    # score gradients it reproduces autograd
    xp = c["xp"].double().requires_grad_(True)
    us, ud = c["us"].double(), c["ud"].double()
    s = (xp.detach() @ us).requires_grad_(True)
    d = (xp.detach() @ ud).requires_grad_(True)
    outs = []
    for tt in range(t):
        score = torch.nn.functional.leaky_relu(d[:, tt].view(-1, 1) + s[:, tt].view(1, -1), 0.2)
        w = cnt * torch.exp(score - score.max(dim=1, keepdim=True).values)
        outs.append((w / w.sum(dim=1, keepdim=True)) @ xp.detach()[:, tt, :])
    (torch.stack(outs, dim=1) * c["go"].double()).sum().backward()
    assert torch.allclose(torch.einsum("nt,ntf->f", s.grad, xp.detach()), c["dus64"], rtol=1e-9, atol=1e-9)
    assert torch.allclose(torch.einsum("nt,ntf->f", d.grad, xp.detach()), c["dud64"], rtol=1e-9, atol=1e-9)


def test_case_counts():
    assert len(WM.LINEAR_SHAPES) == 6 and len(WM.WGRAD_SHAPES) == 6 and len(WM.LAYOUTS) == 5 and len(WM.MODES) == 3
    assert len(WM.GAT_F) * len(WM.GAT_T) == 10
