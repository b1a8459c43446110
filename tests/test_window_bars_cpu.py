"""The window sum's bar (tests/window_bars.py) recomputed on the host: the table, the committed profile, the planted corruptions."""
import os

import pytest
import torch

import window_bars as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table():
    return W.bar_table()


def test_bar_is_four_times_the_worst_restatement_rounded_up(table):
    rows, bar = table
    assert bar == W.BAR_WINDOW
    worst = max(r for _, r in rows)
    assert 4 * worst <= W.BAR_WINDOW < 8 * worst or W.BAR_WINDOW == W.grad_bars.CAP["default"]


def test_docstring_and_profile_hold_the_table(table):
    rows, bar = table
    text = open(os.path.join(ROOT, "profiles", "window_bars.txt")).read()
    for case, r in rows:
        line = f"{str(case):<50} {r:.2e}"
        assert line in W.__doc__, line
        assert line in text, line
    assert f"2 ** {int(torch.log2(torch.tensor(bar)).item())}" in W.__doc__


def test_cases_reach_every_edge():
    shapes = {c: c for c in W.CASES}
    assert any(t == 1 for _, _, t, _, _, _ in shapes)
    assert any(t == 255 for _, _, t, _, _, _ in shapes)
    assert any(w == 1 and f + t > r for _, _, t, r, f, w in shapes)                 # a single window that wraps
    assert any(w > 1 and w + t - 1 == r for _, _, t, r, _, w in shapes)             # exactly full
    assert any(w > 2 * t for _, _, t, _, _, w in shapes)
    assert any(w == W.WC + 1 for _, _, _, _, _, w in shapes)
    assert any(c % 4 == 0 and c % 64 != 0 and n % 64 != 0 for n, c, _, _, _, _ in shapes)
    for n, c, t, r, f, w in W.CASES:
        assert c % 4 == 0 and 1 <= t <= 255 and r >= t and 0 <= f < r and (w == 1 or w + t - 1 <= r)


@pytest.mark.parametrize("kind", W.CORRUPTIONS)
def test_planted_corruption_exceeds_the_bar(kind):
    worst = 0.0
    for case in W.CASES:
        ring, att = W.inputs(case)
        want, den = W.reference64(ring, att, case)
        worst = max(worst, W.ratio(W.restatement32(ring, att, case, corrupt=kind), want, den))
    assert worst > 2 * W.BAR_WINDOW, (kind, worst)


def test_restatement_does_not_depend_on_how_a_window_is_reached():
    """The stated order is per output element: a window computed inside many, alone, or from a rotated ring is the same bits."""
    case = (5, 16, 6, 30, 3, 20)
    ring, att = W.inputs(case)
    full = W.restatement32(ring, att, case)
    for w in (0, 7, 19):
        alone = W.restatement32(ring, att, (5, 16, 6, 30, (3 + w) % 30, 1))
        assert torch.equal(alone[0], full[w])
    slabs = ring[W.slots((5, 16, 6, 30, 3 + 7, 1))[0]]                               # window 7's six slabs in a ring of six, rotated
    rolled = torch.roll(slabs, 2, dims=0).contiguous()
    assert torch.equal(W.restatement32(rolled, att, (5, 16, 6, 6, 2, 1))[0], full[7])


def test_pred_ratio_accepts_the_float64_head_and_sees_a_wrong_layer():
    case = W.CASES[3]
    ring, att = W.inputs(case)
    want, den = W.reference64(ring, att, case)
    c = case[1]
    l1w, l1b, l2w, l2b = W.head_inputs(c)
    rows, dr = want.reshape(-1, c), den.reshape(-1, c)
    y1 = torch.relu(torch.relu(rows) @ l1w.double().t() + l1b.double())
    pred = y1 @ l2w.double().t() + l2b.double()
    assert W.pred_ratio(pred.float(), rows, dr, l1w, l1b, l2w, l2b) <= 1.0
    no_relu = (torch.relu(rows) @ l1w.double().t() + l1b.double()) @ l2w.double().t() + l2b.double()
    assert W.pred_ratio(no_relu.float(), rows, dr, l1w, l1b, l2w, l2b) > 2.0
