"""regt_window_forward / ops.window_forward on the GPU: the window sum held to tests/window_bars.py's bar against float64, the head to
its linear-style allowance, bit-identity across runs / window counts / ring placements, untouched surroundings, the C-level refusals."""
import ctypes as C

import pytest
import torch

import window_bars as W

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd
    regtgcn_amd.load_library()
    return regtgcn_amd


_REF = {}


def _case(case):
    """CPU inputs, the float64 reference and the head of one case, computed once and left unchanged."""
    if case not in _REF:
        ring, att = W.inputs(case)
        want, den = W.reference64(ring, att, case)
        _REF[case] = (ring, att, want, den, W.head_inputs(case[1]))
    return _REF[case]


def _run(R, case, ring=None, first=None, windows=None):
    ring_c, att, _, _, head = _case(case)
    ring = ring_c.cuda() if ring is None else ring
    return R.ops.window_forward(ring, case[4] if first is None else first, case[5] if windows is None else windows, att.cuda(),
                                *[t.cuda() for t in head])


@pytest.mark.parametrize("case", W.CASES, ids=str)
def test_hidden_and_pred_within_their_bars(R, case):
    _, _, want, den, head = _case(case)
    pred, hidden = _run(R, case)
    n, c, _, _, _, windows = case
    assert hidden.shape == (windows, n, c) and pred.shape == (windows, n, head[2].shape[0])
    r = W.ratio(hidden.cpu(), want, den)
    rp = W.pred_ratio(pred.cpu().reshape(windows * n, -1), want.reshape(-1, c), den.reshape(-1, c), *head)
    print(f"{case}: hidden r = {r:.3e} (bar {W.BAR_WINDOW:.3e}), pred error / allowance = {rp:.3f}")
    assert r <= W.BAR_WINDOW
    assert rp <= 1.0


@pytest.mark.parametrize("case", W.CASES, ids=str)
def test_two_runs_are_bit_identical(R, case):
    a, b = _run(R, case), _run(R, case)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("case", [c for c in W.CASES if c[5] > 1], ids=str)
def test_each_window_is_the_same_bits_alone_and_from_a_wrapped_ring(R, case):
    n, c, t, ring_len, first, windows = case
    ring_c = _case(case)[0]
    pred, hidden = _run(R, case)
    ring = ring_c.cuda()
    for w in sorted({0, 1, windows // 2, W.WC - 1, W.WC, windows - 1} & set(range(windows))):
        p1, h1 = _run(R, case, ring, (first + w) % ring_len, 1)
        assert torch.equal(h1[0], hidden[w]) and torch.equal(p1[0], pred[w]), w
        # the same T slabs in a ring of exactly T slots, rotated so that the window wraps
        slabs = ring_c[W.slots((n, c, t, ring_len, first + w, 1))[0]]
        rot = (w + 1) % t
        p2, h2 = _run(R, case, torch.roll(slabs, rot, dims=0).contiguous().cuda(), rot, 1)
        assert torch.equal(h2[0], hidden[w]) and torch.equal(p2[0], pred[w]), w


@pytest.mark.parametrize("case", W.CASES, ids=str)
def test_unread_slots_and_surroundings(R, case):
    """Slots outside the read range hold NaN; ring, pred and hidden sit at a nonzero offset inside NaN-filled buffers."""
    n, c, t, ring_len, first, windows = case
    ring_c, att, _, _, head = _case(case)
    o = head[2].shape[0]
    clean_pred, clean_hidden = _run(R, case)
    poisoned = ring_c.clone()
    used = set(W.slots(case).flatten().tolist())
    for s in range(ring_len):
        if s not in used:
            poisoned[s] = NAN
    pad = 68                                                 # floats: 16-byte aligned, not a multiple of a 256-byte line
    big_ring = torch.full((pad + poisoned.numel() + pad,), NAN, device="cuda")
    big_ring[pad:pad + poisoned.numel()] = poisoned.flatten().cuda()
    ring = big_ring[pad:pad + poisoned.numel()].view(ring_len, n, c)
    big_h = torch.full((pad + windows * n * c + pad,), NAN, device="cuda")
    big_p = torch.full((pad + windows * n * o + pad,), NAN, device="cuda")
    hidden = big_h[pad:pad + windows * n * c].view(windows, n, c)
    pred = big_p[pad:pad + windows * n * o].view(windows, n, o)
    p, h = R.ops.window_forward(ring, first, windows, att.cuda(), *[x.cuda() for x in head], pred=pred, hidden=hidden)
    assert p.data_ptr() == pred.data_ptr() and h.data_ptr() == hidden.data_ptr()
    assert torch.equal(hidden, clean_hidden) and torch.equal(pred, clean_pred)
    for big, size in ((big_h, windows * n * c), (big_p, windows * n * o)):
        assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + size:]).all())
    assert bool(torch.isnan(big_ring[:pad]).all()) and bool(torch.isnan(big_ring[pad + poisoned.numel():]).all())
    assert torch.equal(torch.isnan(ring), torch.isnan(poisoned).cuda())       # the ring itself is only read


def _c_call(R, bufs, **over):
    """regt_window_forward on valid device buffers with some arguments replaced; returns (code, message)."""
    lib = R.load_library()
    a = dict(ring=bufs["ring"].data_ptr(), ring_len=8, first_slot=0, windows=3, N=5, T=4, C=16, O=2, H1=8,
             attention=bufs["att"].data_ptr(), h1w=bufs["h1w"].data_ptr(), h1b=bufs["h1b"].data_ptr(), h2w=bufs["h2w"].data_ptr(),
             h2b=bufs["h2b"].data_ptr(), pred=bufs["pred"].data_ptr(), hidden=bufs["hidden"].data_ptr(), ws=bufs["ws"].data_ptr(),
             ws_bytes=bufs["ws"].numel())
    a.update(over)
    rc = lib.regt_window_forward(a["ring"], a["ring_len"], a["first_slot"], a["windows"], a["N"], a["T"], a["C"], a["O"], a["H1"],
                                 a["attention"], a["h1w"], a["h1b"], a["h2w"], a["h2b"], a["pred"], a["hidden"], a["ws"], a["ws_bytes"],
                                 torch.cuda.current_stream().cuda_stream)
    return rc, lib.regt_last_error().decode()


def test_c_level_refusals_launch_nothing(R):
    lib = R.load_library()
    need = lib.regt_window_workspace_bytes(5, 16, 8, 2, 3)
    assert need > 0
    dev = "cuda"
    bufs = dict(ring=torch.randn(300, 5, 16, device=dev), att=torch.zeros(300, device=dev), h1w=torch.randn(8, 16, device=dev),
                h1b=torch.zeros(8, device=dev), h2w=torch.randn(2, 8, device=dev), h2b=torch.zeros(2, device=dev),
                pred=torch.full((3, 5, 2), NAN, device=dev), hidden=torch.full((3, 5, 16), NAN, device=dev),
                ws=torch.empty(need, dtype=torch.uint8, device=dev))
    refusals = [
        (dict(ring=None), "NULL"), (dict(attention=None), "NULL"), (dict(h1w=None), "NULL"), (dict(h2b=None), "NULL"),
        (dict(pred=None), "NULL"), (dict(hidden=None), "NULL"), (dict(ws=None), "NULL"),
        (dict(ring_len=3), "ring_len=3 < T=4"),
        (dict(windows=6), "would wrap"),                      # 6 + 4 - 1 = 9 > 8
        (dict(C=18), "multiple of 4"),
        (dict(T=256, ring_len=300), "exceeds 255"),
        (dict(ws_bytes=need - 1), "workspace"),
        (dict(first_slot=8), "first_slot"),
        (dict(windows=65535 * W.WC + 1, ring_len=65535 * W.WC + 4), "one call covers"),       # more chunks than one launch covers
    ]
    for over, word in refusals:
        rc, msg = _c_call(R, bufs, **over)
        assert rc != 0 and word in msg, (over, rc, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(bufs["pred"]).all()) and bool(torch.isnan(bufs["hidden"]).all())      # nothing was launched
    assert lib.regt_window_workspace_bytes(5, 16, 8, 2, 0) == 0
    rc, msg = _c_call(R, bufs)                                # the same buffers, unchanged arguments: accepted
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert not bool(torch.isnan(bufs["pred"]).any()) and not bool(torch.isnan(bufs["hidden"]).any())
    rc, msg = _c_call(R, bufs, windows=1, first_slot=6)       # a single window may wrap anywhere
    assert rc == 0, msg


def test_wrapper_validates_before_the_library(R):
    ring = torch.zeros(8, 5, 16, device="cuda")
    att = torch.zeros(4, device="cuda")
    head = [torch.zeros(8, 16, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(2, 8, device="cuda"), torch.zeros(2, device="cuda")]
    with pytest.raises(ValueError):
        R.ops.window_forward(ring.transpose(0, 1), 0, 1, att, *head)               # not contiguous
    with pytest.raises(ValueError):
        R.ops.window_forward(ring, 0, 6, att, *head)                               # would wrap
    with pytest.raises(ValueError):
        R.ops.window_forward(ring, 0, 1, att, head[0][:, :12].contiguous(), *head[1:])
    with pytest.raises(R.RegtError):
        R.ops.window_forward(ring.double(), 0, 1, att, *head)
    with pytest.raises(R.RegtError):
        R.ops.window_forward(ring, 0, 1, att.cpu(), *head)
