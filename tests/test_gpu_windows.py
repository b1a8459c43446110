"""The op-site entry points of include/regtgcn.h called directly through the C ABI on strided, offset and poisoned buffers
(tests/window_math.py): leading dimensions other than the width, pointers that are not 16-byte aligned, NULL bias / dbias,
an X with more rows than Y, in all three GEMM arithmetics -- what regtgcn_amd.ops never passes.  Every operand lives in a guarded
window; after every call no word outside any window may have changed and every output element must have been written, the
result must meet a bar derived from the float64 reference's own fp32 gap (gru_math.bar), and a second call must reproduce it
bit for bit.  tests/test_window_cpu.py shows that planted defects trip exactly these checks and that the bars can be met.

Measured on an MI355X, largest err / bar per entry point over all of its cases (the module prints every case with -s); layouts
of one shape differ only where they select another kernel, i.e. another summation order (dbias of (1037, 260, 132): 0.223 / 0.086
from the vector kernels of fp32 / bf16x3, 0.331 from the generic one that the `odd` and `odd_in` layouts take):
    regt_linear act 0 / 1 / 2     fp32 0.122   bf16x3 0.122   bf16 0.122   all at (5505, 260, 36) without bias (bf16: `odd`, fp32 kernel)
    regt_linear act 3 / 4         fp32 0.041   bf16x3 0.036   bf16 0.019   (8193, 256, 32), tanh, share of the absolute 2e-5
    regt_wgrad dW                 fp32 0.207   bf16x3 0.207   bf16 0.207   (700, 128, 33): the generic fp32 kernel in all three
    regt_wgrad dbias              fp32 0.331   bf16x3 0.331   bf16 0.331   (1037, 260, 132)
    regt_spmm_csr 0.257 (width 132)   regt_spmm_dual YA 0.060, YL 0.056   regt_pack_x bit-equal
    regt_gat_forward out 0.038   score gradients d u_src 0.027, d u_dst 0.038
No case failed and no kernel was changed.  bf16 arithmetic (mode 2), which float64 product the result met:
    the bf16-rounded operands -- regt_linear (7, 4, 4), (129, 68, 36), (8193, 256, 32), (5505, 260, 36) in `dense` and `padded16`;
      regt_wgrad dW (3000, 132, 36) and (1037, 260, 132) in `dense`, `padded16` and `odd_out` (the slab reduction alone turns scalar);
    the unrounded operands (the library's fp32 kernels) -- every `odd`, `odd_in` and, for regt_linear, `odd_out` layout; (1, 1, 1)
      and (129, 65, 33) everywhere; regt_wgrad (5, 4, 4), (700, 128, 33), (16897, 36, 32) everywhere; dbias always (the column
      sums are taken of the fp32 rows).
"""
import contextlib

import pytest
import torch

import window_math as WM
from window_math import LAYOUTS, MODES, POISON, Window

pytestmark = pytest.mark.gpu
DEV = "cuda"

LINEAR_CASES = [(s, lay, mode, bias, 0) for s in WM.LINEAR_SHAPES for lay in LAYOUTS for mode in MODES for bias in (True, False)] + \
               [(s, lay, mode, bias, act) for s in WM.LINEAR_ACT_SHAPES for lay in ("dense", "padded16") for mode in MODES
                for bias in (True, False) for act in (1, 2, 3, 4)]
WGRAD_CASES = [(s, lay, mode, bias) for s in WM.WGRAD_SHAPES for lay in LAYOUTS for mode in MODES for bias in (True, False)]
PACK_CASES = [(s, lay) for s in WM.PACK_SHAPES for lay in LAYOUTS]
GAT_CASES = [(f, t) for f in WM.GAT_F for t in WM.GAT_T]
# every listed case is a test of its own: a parametrisation that shrinks fails here
assert (len(LINEAR_CASES), len(WGRAD_CASES), len(WM.SPMM_WIDTHS), len(WM.DUAL_WIDTHS), len(PACK_CASES), len(GAT_CASES)) == (276, 180, 4, 2, 10, 10)

_FAULT = []                    # a HIP error seen by this module: nothing of it launches afterwards
_RATIOS = {}                   # (entry point, arithmetic) -> (largest err / bar, case)
_MATCHED = {}                  # bf16 arithmetic: case -> "rounded" | "unrounded"


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd
    regtgcn_amd.load_library()
    yield regtgcn_amd
    for key in sorted(_RATIOS):
        print(f"\nlargest err/bar {key[0]} mode {key[1]}: {_RATIOS[key][0]:.3f} at {_RATIOS[key][1]}", end="")
    for what in ("rounded", "unrounded"):
        print(f"\nbf16 arithmetic matched the {what} product:", sorted({c for c, w in _MATCHED.items() if w == what}), end="")
    print()


@pytest.fixture()
def lib(R):
    if _FAULT:
        pytest.fail(f"not started: an earlier case of this module ended in a GPU error ({_FAULT[0]})")
    from regtgcn_amd import _lib
    handle = _lib.load()
    prev = handle.regt_set_gemm_mode(0)
    try:
        yield handle
    finally:
        handle.regt_set_gemm_mode(prev)


def _p(win):
    import ctypes
    return None if win is None else ctypes.c_void_p(win.data_ptr())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        _FAULT.append(str(exc).splitlines()[0])
        raise


def _run(rc, what):
    from regtgcn_amd import _lib
    _lib.check(rc, what)           # the header documents no restriction on these operands: a refusal is a failure
    _sync()


_DEV_CACHE = {}


def _dev(t):
    """A reference on the device (kept: every layout of a case shares it)."""
    key = id(t)
    if key not in _DEV_CACHE:
        _DEV_CACHE[key] = (t, t.to(DEV))
    return _DEV_CACHE[key][1]


def _rel(got, ref64):
    ref = _dev(ref64)
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _note(entry, mode, ratio, case):
    print(f"{entry} {case} mode {mode}: err/bar = {ratio:.3f}")
    if not ratio <= _RATIOS.get((entry, mode), (-1.0, None))[0]:
        _RATIOS[(entry, mode)] = (ratio, case)


def _either(entry, mode, case, ratio_plain, ratio_rounded, need_rounded):
    """fp32 / bf16x3: the unrounded product.  bf16: the product of the bf16-rounded operands where the bf16 pipe runs, of the
    unrounded ones where the library falls back to its fp32 kernels -- one of the two, the rounded one where the dense tests
    already demand it."""
    if mode != 2:
        _note(entry, mode, ratio_plain, case)
        assert ratio_plain <= 1.0, (entry, case, mode, ratio_plain)
        return
    which = "rounded" if (need_rounded or not ratio_plain <= 1.0) else "unrounded"
    ratio = ratio_rounded if which == "rounded" else ratio_plain
    _MATCHED[(entry,) + tuple(case)] = which
    _note(entry, mode, ratio, case + (which,))
    assert ratio <= 1.0, (entry, case, mode, {"unrounded": ratio_plain, "rounded": ratio_rounded, "need_rounded": need_rounded})


def _check_all(wins, outputs, what):
    for name, w in wins.items():
        if w is not None:
            w.check_untouched(f"{what} {name}")
    for name in outputs:
        if wins[name] is not None:
            wins[name].check_written(f"{what} {name}")


@pytest.mark.parametrize("shape,layout,mode,with_bias,act", LINEAR_CASES)
def test_linear_windows(lib, shape, layout, mode, with_bias, act):
    m, n, k = shape
    a, w, b = WM.linear_inputs(m, n, k)
    wins = {"A": WM.make(layout, "a", m, k, a, DEV), "W": WM.make(layout, "in", n, k, w, DEV),
            "bias": WM.make(layout, "out", 1, n, b, DEV, strided=False) if with_bias else None, "out": WM.make(layout, "out", m, n, None, DEV)}
    lib.regt_set_gemm_mode(mode)
    what = f"regt_linear {shape} {layout} mode {mode} bias {with_bias} act {act}"

    def call():
        _run(lib.regt_linear(_p(wins["A"]), wins["A"].ld, m, k, _p(wins["W"]), wins["W"].ld, n, _p(wins["bias"]), act, 0.01,
                             _p(wins["out"]), wins["out"].ld, _stream()), what)
        _check_all(wins, ["out"], what)
    call()
    first = wins["out"].bits.clone()
    got = wins["out"].get()
    ratios = []
    for rounded in (False, True):
        ref64, _, tol = WM.linear_refs(m, n, k, with_bias, act, rounded)
        if act in (3, 4):
            ratios.append(float((got.double() - _dev(ref64)).abs().max()) / WM.ABS_ACT_BAR)
        else:
            ratios.append(_rel(got, ref64) / tol)
    _either("linear" if act < 3 else "linear(act 3/4)", mode, (shape, layout, with_bias, act), ratios[0], ratios[1],
            WM.must_be_rounded(layout, n, k))
    wins["out"].repoison()
    call()
    assert torch.equal(wins["out"].bits, first), what + ": not reproducible"


@pytest.mark.parametrize("shape,layout,mode,with_bias", WGRAD_CASES)
def test_wgrad_windows(lib, shape, layout, mode, with_bias):
    m, n, k = shape
    d, a = WM.wgrad_inputs(m, n, k)
    nslab = int(lib.regt_wgrad_slab_floats(m, n, k, 1 if with_bias else 0))
    wins = {"dOut": WM.make(layout, "a", m, n, d, DEV), "A": WM.make(layout, "a", m, k, a, DEV), "dW": WM.make(layout, "out", n, k, None, DEV),
            "dbias": WM.make(layout, "out", 1, n, None, DEV, strided=False) if with_bias else None,
            "slab": WM.make(layout, "out", 1, max(nslab, 1), None, DEV, strided=False)}
    lib.regt_set_gemm_mode(mode)
    what = f"regt_wgrad {shape} {layout} mode {mode} dbias {with_bias}"
    outs = ["dW", "dbias"]

    def call():
        _run(lib.regt_wgrad(_p(wins["dOut"]), wins["dOut"].ld, _p(wins["A"]), wins["A"].ld, m, n, k, _p(wins["dW"]), wins["dW"].ld,
                            _p(wins["dbias"]), _p(wins["slab"]), _stream()), what)
        _check_all(wins, outs, what)
        if nslab == 0:
            assert int(wins["slab"].bits[0, 0]) == POISON, what + ": a slab of 0 floats was written"
    call()
    first = {o: wins[o].bits.clone() for o in outs if wins[o] is not None}
    refs = [WM.wgrad_refs(m, n, k, rounded) for rounded in (False, True)]
    for idx, o in enumerate(outs):
        if wins[o] is None:
            continue
        got = wins[o].get().reshape(refs[0][idx][0].shape)
        ratios = [_rel(got, r[idx][0]) / r[idx][2] for r in refs]
        _either(f"wgrad {o}", mode, (shape, layout, with_bias), ratios[0], ratios[1], WM.must_be_rounded(layout, n, k) and o == "dW")
    # what slab, dW and dbias held on entry is irrelevant: infinities instead of the poison, same bits out
    for o in outs + ["slab"]:
        if wins[o] is not None and not (o == "slab" and nslab == 0):
            wins[o].view.fill_(float("inf"))
    call()
    for o, bits in first.items():
        assert torch.equal(wins[o].bits, bits), f"{what} {o}: depends on the buffers' contents on entry, or is not reproducible"


def _spmm_note(entry, case, got, op64, x):
    ref64 = WM.ref_spmm(op64, x, torch.float64)
    gap, tol = WM.gap_bar(WM.ref_spmm(op64, x, torch.float32), ref64)
    ratio = _rel(got, ref64) / tol
    _note(entry, "-", ratio, case)
    assert ratio <= 1.0, (entry, case, ratio)


@pytest.mark.parametrize("width", WM.SPMM_WIDTHS)
def test_spmm_csr_windows(R, lib, width):
    n, extra = 300, 40
    ei, val = WM.spmm_graph(n)
    rp, col, v = R.graph.raw_csr(ei.to(DEV), val.to(DEV), n)
    op64 = WM.csr_dense(rp, col, v, n)
    assert torch.equal(op64, torch.zeros(n, n, dtype=torch.float64).index_put_((ei[1], ei[0]), val.double(), accumulate=True))
    x = torch.randn(n, width, generator=torch.Generator().manual_seed(width))
    wins = {"X": Window(n + extra, width, data=torch.cat([x, torch.zeros(extra, width)]), device=DEV), "Y": Window(n, width, device=DEV)}
    wins["X"].bits[n:] = POISON              # rows no entry refers to: poisoned, and nrows_x says they exist
    assert wins["X"].aligned16() and wins["Y"].aligned16()
    what = f"regt_spmm_csr width {width}"

    def call():
        _run(lib.regt_spmm_csr(R._lib.ptr(rp), R._lib.ptr(col), R._lib.ptr(v), _p(wins["X"]), _p(wins["Y"]), n, n + extra, width, _stream()), what)
        _check_all(wins, ["Y"], what)
        assert bool((wins["X"].bits[n:] == POISON).all()), what + ": wrote into X"
    call()
    got = wins["Y"].get()
    _spmm_note("spmm_csr", (width,), got, op64, x)
    assert float(got[200:].abs().max()) == 0.0, what + ": a row without entries must be exactly 0"
    first = wins["Y"].bits.clone()
    wins["Y"].repoison()
    call()
    assert torch.equal(wins["Y"].bits, first), what + ": not reproducible"


@pytest.mark.parametrize("width", WM.DUAL_WIDTHS)
def test_spmm_dual_windows(R, lib, width):
    n = 300
    g = R.data.synthetic_regional_graph(n, 2400, 3, seed=n)
    pg = R.prepare_graph(g.edge_index.to(DEV), None, [t.to(DEV) for t in g.region_index], [t.to(DEV) for t in g.region_attr], n)
    assert pg.m_rowptr is not None
    x = torch.randn(n, width, generator=torch.Generator().manual_seed(width))
    wins = {"X": Window(n, width, data=x, device=DEV), "YA": Window(n, width, device=DEV), "YL": Window(n, width, device=DEV)}
    what = f"regt_spmm_dual width {width}"
    ptr = R._lib.ptr

    def call():
        _run(lib.regt_spmm_dual(ptr(pg.m_rowptr), ptr(pg.m_col), ptr(pg.m_val_a), ptr(pg.m_val_l), _p(wins["X"]), _p(wins["YA"]),
                                _p(wins["YL"]), n, width, _stream()), what)
        _check_all(wins, ["YA", "YL"], what)
    call()
    first = {}
    for o, vals in (("YA", pg.m_val_a), ("YL", pg.m_val_l)):
        _spmm_note("spmm_dual " + o, (width,), wins[o].get(), WM.csr_dense(pg.m_rowptr, pg.m_col, vals, n), x)
        first[o] = wins[o].bits.clone()
        wins[o].repoison()
    call()
    for o in first:
        assert torch.equal(wins[o].bits, first[o]), what + ": not reproducible"


@pytest.mark.parametrize("shape,layout", PACK_CASES)
def test_pack_x_windows(lib, shape, layout):
    """No leading dimension in this entry point: a layout contributes its pointer offsets alone."""
    n, f, t = shape
    x = torch.randn(n, f, t, generator=torch.Generator().manual_seed(n))
    extra = 6
    wins = {"x": WM.make(layout, "in", n, f * t, x.reshape(n, f * t), DEV, strided=False),
            "packed": WM.make(layout, "out", n + extra, t * f, None, DEV, strided=False)}
    want = x.permute(0, 2, 1).contiguous().reshape(n, t * f).to(DEV)
    what = f"regt_pack_x {shape} {layout}"
    for _ in range(2):
        _run(lib.regt_pack_x(_p(wins["x"]), _p(wins["packed"]), n, f, t, _stream()), what)
        _check_all(wins, [], what)
        assert bool((wins["packed"].bits[n:] == POISON).all()), what + ": rows past the snapshot's were written"
        assert torch.equal(wins["packed"].bits[:n], want.view(torch.int32)), what
        wins["packed"].repoison()


@pytest.mark.parametrize("f,t", GAT_CASES)
def test_gat_windows(R, lib, f, t):
    """F = 4, 12, 100, 132, 256: lane groups of 2, 4, 32, 64, 64.  The kernels read and write 16-byte pieces of packed rows: the
    dense, 16-byte aligned form is the only one the entry points take."""
    n, slope = WM.GAT_NODES, 0.2
    c = WM.gat_case(f, t)
    rows = n * t
    pat = R.graph.prepare_attention_pattern(c["ei"].to(DEV), n)
    wins = {"x": Window(rows, f, data=c["xp"].reshape(rows, f), device=DEV), "dout": Window(rows, f, data=c["go"].reshape(rows, f), device=DEV),
            "u_src": Window(1, f, data=c["us"], device=DEV, margin_words=WM.MARGIN_WORDS),
            "u_dst": Window(1, f, data=c["ud"], device=DEV, margin_words=WM.MARGIN_WORDS),
            "out": Window(rows, f, device=DEV), "stats": Window(rows, 4, device=DEV), "dsd": Window(rows, 2, device=DEV)}
    assert all(w.aligned16() for w in wins.values())
    ptr = R._lib.ptr
    what = f"regt_gat F {f} T {t}"

    def call():
        _run(lib.regt_gat_forward(ptr(pat.rowptr), ptr(pat.col), _p(wins["x"]), _p(wins["u_src"]), _p(wins["u_dst"]), slope, n, t, f,
                                  _p(wins["out"]), _p(wins["stats"]), _stream()), what + " forward")
        _check_all(wins, ["out"], what + " forward")
        wins["stats"].check_written(what + " forward stats", cols=3)
        _run(lib.regt_gat_backward(ptr(pat.rowptr), ptr(pat.col), ptr(pat.t_rowptr), ptr(pat.t_col), _p(wins["x"]), _p(wins["u_src"]), slope,
                                   n, t, f, _p(wins["dout"]), _p(wins["stats"]), _p(wins["dsd"]), _stream()), what + " backward")
        _check_all(wins, ["out", "stats", "dsd"], what + " backward")
    call()
    out = wins["out"].get().reshape(n, t, f)
    err = float((out.double() - _dev(c["out64"])).abs().max())
    _note("gat out", "-", err / WM.GAT_OUT_BAR, (f, t))
    assert err <= WM.GAT_OUT_BAR, (what, err)
    dsd = wins["dsd"].get().double().cpu().reshape(n, t, 2)
    scale = max(1.0, float(c["dus64"].abs().max()), float(c["dud64"].abs().max()))
    for idx, key in enumerate(("dus64", "dud64")):
        got = torch.einsum("nt,ntf->f", dsd[:, :, idx], c["xp"].double())          # d u = sum over rows of dsd[:, idx] * x
        ok, ratio = WM.gat_grad_ok(got, c[key], scale)
        _note("gat " + key[:3], "-", ratio, (f, t))
        assert ok, (what, key, ratio)
    first = {o: wins[o].bits.clone() for o in ("out", "stats", "dsd")}
    for o in first:
        wins[o].repoison()
    call()
    for o in first:
        assert torch.equal(wins[o].bits, first[o]), f"{what} {o}: not reproducible"
