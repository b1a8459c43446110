"""regt_window_backward / ops.window_backward on the GPU over tests/window_bwd_math.py's cases: dring within its bar against float64,
the head's gradients within op_bars' wgrad bars, d_attention within grad_bars.REL["attention"] of its own scale; dring bit-identical
however the windows are split over accumulating calls and from a rotated ring; accumulate = 0 against 1 on zeroed buffers; untouched
slots and surroundings; two runs bit-identical; the C-level refusals."""
import pytest
import torch

import op_bars
import window_bwd_math as B
from grad_bars import REL

pytestmark = pytest.mark.gpu
NAN = float("nan")
HEAD = ("l1w", "l1b", "l2w", "l2b")


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd
    regtgcn_amd.load_library()
    return regtgcn_amd


_REF = {}


def _case(case):
    """CPU inputs and the float64 references (accumulate = 0 and 1) of one case, computed once and left unchanged."""
    if case not in _REF:
        x = B.inputs(case)
        _REF[case] = (x, B.reference64(x, case, False), B.reference64(x, case, True))
    return _REF[case]


def _outs(x, fill):
    """d_attention and the four head gradients on the GPU, filled with ``fill``."""
    return [torch.full_like(x[k], fill).cuda() for k in ("att",) + HEAD]


def _run(R, case, x, dring, accumulate, outs, ring=None, first=None, lo=0, hi=None):
    """Windows lo .. hi - 1 of the case (all by default) into ``dring`` / ``outs``."""
    n, c, t, ring_len, f0, windows = case
    hi = windows if hi is None else hi
    first = f0 if first is None else first
    ring = x["ring"].cuda() if ring is None else ring
    R.ops.window_backward(ring, (first + lo) % ring.shape[0], hi - lo, x["att"].cuda(), *[x[k].cuda() for k in HEAD],
                          x["hidden"][lo:hi].contiguous().cuda(), x["dpred"][lo:hi].contiguous().cuda(), dring, accumulate, *outs)


@pytest.mark.parametrize("case", B.CASES, ids=str)
def test_every_gradient_within_its_bar(R, case):
    x, ref0, ref1 = _case(case)
    ring_len = case[3]
    dring = torch.full((ring_len,) + x["ring"].shape[1:], NAN).cuda()
    outs = _outs(x, NAN)
    _run(R, case, x, dring, False, outs)
    r = B.dring_ratio(dring.cpu(), ref0, case)
    a1, y1, d1 = B.head_operands(x)
    dp = x["dpred"].reshape(-1, B.O)
    head = {"d_l1w": op_bars.wgrad_ratio(outs[1].cpu(), d1.float(), a1.float()), "d_l1b": op_bars.dbias_ratio(outs[2].cpu(), d1.float()),
            "d_l2w": op_bars.wgrad_ratio(outs[3].cpu(), dp, y1.float()), "d_l2b": op_bars.dbias_ratio(outs[4].cpu(), dp)}
    ra = B.att_ratio(outs[0].cpu(), ref0)
    print(f"{case}: dring r = {r:.3e} (bar {B.BAR_DRING:.3e}), d_attention / scale = {ra:.3e} (bar {REL['attention']:.3e}), head {head}")
    assert r <= B.BAR_DRING
    assert head["d_l1w"] <= op_bars.BAR["wgrad"] and head["d_l2w"] <= op_bars.BAR["wgrad"]
    assert head["d_l1b"] <= op_bars.BAR["wgrad_bias"] and head["d_l2b"] <= op_bars.BAR["wgrad_bias"]
    assert ra <= REL["attention"]
    other = torch.ones(ring_len, dtype=torch.bool)
    other[B.covered(case)] = False
    assert bool(torch.isnan(dring.cpu()[other]).all())                      # slots outside the covered ones: not touched
    # accumulate = 1 from the carried values: the bar with |carried| in the denominator, the other slots bit-identical
    dring = x["carried"].clone().cuda()
    _run(R, case, x, dring, True, _outs(x, 0.0))
    assert B.dring_ratio(dring.cpu(), ref1, case) <= B.BAR_DRING
    assert torch.equal(dring.cpu()[other], x["carried"][other])


@pytest.mark.parametrize("case", [c for c in B.CASES if c[5] > 2], ids=str)
def test_dring_is_the_same_bits_split_over_accumulating_calls_and_from_a_rotated_ring(R, case):
    x, _, _ = _case(case)
    n, c, t, ring_len, first, windows = case
    whole = x["carried"].clone().cuda()
    _run(R, case, x, whole, True, _outs(x, 0.0))
    for cuts in ((windows // 2,), (1, windows - 1)):
        dring = x["carried"].clone().cuda()
        outs = _outs(x, 0.0)
        lo = 0
        for hi in list(cuts) + [windows]:
            if hi > lo:
                _run(R, case, x, dring, True, outs, lo=lo, hi=hi)
            lo = hi
        assert torch.equal(dring, whole), cuts
    rot = 3 % ring_len
    dring = torch.roll(x["carried"], rot, dims=0).contiguous().cuda()
    _run(R, case, x, dring, True, _outs(x, 0.0), ring=torch.roll(x["ring"], rot, dims=0).contiguous().cuda(), first=(first + rot) % ring_len)
    assert torch.equal(torch.roll(dring, -rot, dims=0), whole)


@pytest.mark.parametrize("case", B.CASES, ids=str)
def test_accumulate_on_zeros_is_plain_write_and_two_runs_are_bit_identical(R, case):
    x, _, _ = _case(case)
    res = []
    for acc, fill in ((False, NAN), (True, 0.0), (False, NAN)):
        dring = torch.full(tuple(x["ring"].shape), fill).cuda()
        outs = _outs(x, fill)
        _run(R, case, x, dring, acc, outs)
        res.append([dring[B.covered(case).cuda()]] + outs)
    for a, b, c in zip(*res):
        assert torch.equal(a, c)                                             # two runs
        assert torch.equal(a, b)                                             # 0 + g == g


def test_surroundings_stay_poisoned(R):
    """dring and the gradient outputs sit at a nonzero offset inside NaN-filled buffers; ring slots outside the covered range hold NaN."""
    case = (43, 256, 12, 40, 3, 29)
    x, ref0, _ = _case(case)
    n, c, t, ring_len, first, windows = case
    pad = 68                                                 # floats: 16-byte aligned, not a multiple of a 256-byte line
    ring = x["ring"].clone()
    used = set(B.covered(case).tolist())
    for s in range(ring_len):
        if s not in used:
            ring[s] = NAN

    def guarded(t_):
        big = torch.full((pad + t_.numel() + pad,), NAN, device="cuda")
        return big, big[pad:pad + t_.numel()].view(t_.shape)

    big_d, dring = guarded(x["ring"])
    bigs, outs = zip(*[guarded(x[k]) for k in ("att",) + HEAD])
    _run(R, case, x, dring, False, list(outs), ring=ring.cuda())
    assert B.dring_ratio(dring.cpu(), ref0, case) <= B.BAR_DRING
    assert B.att_ratio(outs[0].cpu(), ref0) <= REL["attention"]
    for big, view in [(big_d, dring)] + list(zip(bigs, outs)):
        assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + view.numel():]).all())
    assert not any(bool(torch.isnan(o).any()) for o in outs)


def _c_call(R, bufs, **over):
    lib = R.load_library()
    a = dict(ring=bufs["ring"].data_ptr(), ring_len=8, first_slot=0, windows=3, N=5, T=4, C=16, O=2, H1=8, attention=bufs["att"].data_ptr(),
             h1w=bufs["h1w"].data_ptr(), h1b=bufs["h1b"].data_ptr(), h2w=bufs["h2w"].data_ptr(), h2b=bufs["h2b"].data_ptr(),
             hidden=bufs["hidden"].data_ptr(), dpred=bufs["dpred"].data_ptr(), dring=bufs["dring"].data_ptr(), accumulate=0,
             d_att=bufs["d_att"].data_ptr(), d1w=bufs["d1w"].data_ptr(), d1b=bufs["d1b"].data_ptr(), d2w=bufs["d2w"].data_ptr(),
             d2b=bufs["d2b"].data_ptr(), ws=bufs["ws"].data_ptr(), ws_bytes=bufs["ws"].numel())
    a.update(over)
    rc = lib.regt_window_backward(a["ring"], a["ring_len"], a["first_slot"], a["windows"], a["N"], a["T"], a["C"], a["O"], a["H1"],
                                  a["attention"], a["h1w"], a["h1b"], a["h2w"], a["h2b"], a["hidden"], a["dpred"], a["dring"], a["accumulate"],
                                  a["d_att"], a["d1w"], a["d1b"], a["d2w"], a["d2b"], a["ws"], a["ws_bytes"],
                                  torch.cuda.current_stream().cuda_stream)
    return rc, lib.regt_last_error().decode()


def test_c_level_refusals_launch_nothing(R):
    lib = R.load_library()
    need = lib.regt_window_backward_workspace_bytes(5, 16, 8, 2, 3, 4)
    assert need > 0
    dev = "cuda"
    nan = lambda *s: torch.full(s, NAN, device=dev)
    bufs = dict(ring=torch.randn(300, 5, 16, device=dev), att=torch.zeros(300, device=dev), h1w=torch.randn(8, 16, device=dev),
                h1b=torch.zeros(8, device=dev), h2w=torch.randn(2, 8, device=dev), h2b=torch.zeros(2, device=dev),
                hidden=torch.randn(3, 5, 16, device=dev), dpred=torch.randn(3, 5, 2, device=dev), dring=nan(300, 5, 16), d_att=nan(300),
                d1w=nan(8, 16), d1b=nan(8), d2w=nan(2, 8), d2b=nan(2), ws=torch.empty(need, dtype=torch.uint8, device=dev))
    refusals = [
        (dict(ring=None), "NULL"), (dict(attention=None), "NULL"), (dict(h2b=None), "NULL"), (dict(hidden=None), "NULL"),
        (dict(dpred=None), "NULL"), (dict(dring=None), "NULL"), (dict(d_att=None), "NULL"), (dict(d2w=None), "NULL"), (dict(ws=None), "NULL"),
        (dict(ring_len=3), "ring_len=3 < T=4"),
        (dict(windows=6), "would wrap"),                      # 6 + 4 - 1 = 9 > 8
        (dict(windows=1, ring_len=4, first_slot=3), None),    # accepted below: exactly T slots, wrapping
        (dict(C=18), "multiple of 4"),
        (dict(T=33, ring_len=300), "exceeds the 32 periods"),
        (dict(ws_bytes=need - 1), "workspace"),
        (dict(first_slot=8), "first_slot"),
        (dict(dring=bufs["dring"].data_ptr() + 4), "16-byte aligned"),
    ]
    for over, word in refusals:
        if word is None:
            continue
        rc, msg = _c_call(R, bufs, **over)
        assert rc != 0 and word in msg, (over, rc, msg)
    torch.cuda.synchronize()
    for k in ("dring", "d_att", "d1w", "d1b", "d2w", "d2b"):
        assert bool(torch.isnan(bufs[k]).all()), k            # nothing was launched
    assert lib.regt_window_backward_workspace_bytes(5, 16, 8, 2, 0, 4) == 0
    rc, msg = _c_call(R, bufs)                                # the same buffers, unchanged arguments: accepted
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert not bool(torch.isnan(bufs["dring"][:6]).any()) and bool(torch.isnan(bufs["dring"][6:]).all())
    assert not any(bool(torch.isnan(bufs[k]).any()) for k in ("d1w", "d1b", "d2w", "d2b")) and not bool(torch.isnan(bufs["d_att"][:4]).any())
    rc, msg = _c_call(R, bufs, windows=1, ring_len=4, first_slot=3)
    assert rc == 0, msg


def test_wrapper_validates_before_the_library(R):
    case = (3, 8, 6, 10, 7, 3)
    x, _, _ = _case(case)
    dring = torch.zeros(tuple(x["ring"].shape), device="cuda")
    with pytest.raises(ValueError):
        _run(R, case, x, dring[:, :, :4], True, _outs(x, 0.0))                      # dring of another shape
    with pytest.raises(ValueError):
        _run(R, case, x, dring, True, _outs(x, 0.0), hi=6)                          # hidden / dpred hold three windows, not six
    with pytest.raises(ValueError):
        R.ops.window_backward(x["ring"].cuda(), 0, 1, torch.zeros(33, device="cuda"), *[torch.zeros(1, device="cuda")] * 6, dring, True,
                              *[torch.zeros(1, device="cuda")] * 5)                 # T over the limit
    with pytest.raises(R.RegtError):
        _run(R, case, x, dring.cpu(), True, _outs(x, 0.0))
