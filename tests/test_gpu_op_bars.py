"""The op-site kernels (regt_linear, regt_wgrad, regt_spmm_csr, regt_spmm_dual, regt_spmm_dual_bf16) held to the per-element bars of
tests/op_bars.py, at the smallest shapes that take each branch of launch_fast / launch_flat, launch_wgrad_impl, launch_spmm_csr and
launch_spmm_dual_x.  Every case is labelled with op_bars.expected_kernel (a Python restatement of the dispatch: the kernel that ran is
not read back from the library), compared with float64 from the same inputs -- never with another kernel -- and run twice: the second
run must be bit-identical.  profiles/op_bars.txt holds every case's measured ratio."""
import os
import subprocess
import sys

import pytest
import torch

import op_bars as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd
    regtgcn_amd.load_library()
    return regtgcn_amd


class _Mode:
    def __init__(self, R, mode):
        self.lib, self.mode = R.load_library(), mode

    def __enter__(self):
        self.prev = self.lib.regt_set_gemm_mode(self.mode)

    def __exit__(self, *exc):
        self.lib.regt_set_gemm_mode(self.prev)


def _twice(f):
    def run(*args):
        first = f(*args)
        again = f(*args)
        for x, y in zip(first if isinstance(first, tuple) else (first,), again if isinstance(again, tuple) else (again,)):
            assert (x is None and y is None) or torch.equal(x, y), "second run differs"
        return first
    return run


def _held(rows):
    bad = []
    for cls, label, name, r, _ in rows:
        print(f"{label} [{name}] {cls}: r = {r:.3e} (bar {B.BAR[cls]:.3e})")
        if not r <= B.BAR[cls]:
            bad.append((label, name, cls, r))
    assert not bad, bad


def _hip_linear(R):
    return _twice(lambda a, w, b, act: R.ops.linear(a.cuda(), w.cuda(), b.cuda(), act))


@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("shape,acts", B.LINEAR_CASES, ids=[str(s) for s, _ in B.LINEAR_CASES])
def test_linear_per_element(R, shape, acts, mode):
    with _Mode(R, mode):
        _held(B.linear_case(shape, acts, mode, hip=_hip_linear(R), restate=False))
        if B.arithmetic_of(B.expected_kernel("linear", mode, shape)) == 2:
            # second assertion of the bf16-operand arithmetic: within 2.2 u sum|a w| of the UNROUNDED product
            a, w, b = B.linear_inputs(*shape)
            z, den = B.linear_reference(a, w, b)
            for act in acts:
                got = R.ops.linear(a.cuda(), w.cuda(), b.cuda(), act).cpu().double()
                assert bool(((got - B.act64(z, act)).abs() <= 2.2 * B.BF16_U * den + 1e-6).all()), (shape, act)


@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("k,n", B.IDENTITY_CASES)
def test_linear_identity_with_asymmetric_weight(R, k, n, mode):
    """A = I with an asymmetric W catches a transposed or shifted C write: once per kernel name and arithmetic."""
    with _Mode(R, mode):
        rows, a, w, got = B.identity_case(k, n, mode, hip=_twice(lambda a, w: R.ops.linear(a.cuda(), w.cuda())), restate=False)
    _held(rows)
    ar = B.arithmetic_of(rows[0][2])
    if ar != 1:      # one non-zero product per element: exact (bf16x3 adds three pieces, whose partial sums need not be fp32 numbers)
        assert torch.equal(got, (B.bf16_round(w) if ar == 2 else w).t().contiguous()), rows[0][2]


def test_split_kernels_on_non_cancelling_inputs(R):
    """bf16x3 (arithmetic 1) on operands whose second and third bf16 pieces are large and whose products all have one sign along the
    reduction: a split kernel that lost ANY kept partial product would be off by >= 5.7e-6 of sum|terms| in every element
    (tests/test_op_bars_cpu.py), 3 x the linear bar and 6 x the wgrad bar.  gemm_flat_split_kernel<3> with scalar descriptors and
    with the LDS table, wgrad_split_kernel<3> on full and partial tiles."""
    rows = []
    with _Mode(R, 1):
        for shape in B.SENSITIVE_LINEAR:
            rows += B.linear_case(shape, (0,), 1, hip=_hip_linear(R), restate=False, inputs=B.split_sensitive_inputs)
        for shape in B.SENSITIVE_WGRAD:
            rows += B.wgrad_case(shape, 1, False, hip=_twice(lambda d, a, wb: R.ops.wgrad(d.cuda(), a.cuda(), wb)), restate=False,
                                 inputs=B.wgrad_sensitive_inputs)
    assert [r[2].split(" ")[0] for r in rows] == ["gemm_flat_split_kernel<3>/scalar", "gemm_flat_split_kernel<3>/table",
                                                   "wgrad_split_kernel<3>", "wgrad_split_kernel<3>"]
    _held(rows)


CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch
import op_bars as B
import regtgcn_amd as R
lib = R.load_library()
opt = {"fp32_core_wide": int(os.environ.get("REGT_FP32_CORE") == "wide"), "desc_table": int(os.environ.get("REGT_GEMM_DESC") == "table")}
def digest(*ts):
    return hashlib.sha1(b"".join(t.cpu().numpy().tobytes() for t in ts if t is not None)).hexdigest()
for mode in [int(m) for m in sys.argv[1].split(",")]:
    lib.regt_set_gemm_mode(mode)
    rows = []
    for shape in B.CHILD_SHAPES:
        def hip(a, w, b, act):
            x = R.ops.linear(a.cuda(), w.cuda(), b.cuda(), act)
            assert torch.equal(x, R.ops.linear(a.cuda(), w.cuda(), b.cuda(), act)), "second run differs"
            print("DIGEST", "linear", shape, act, mode, digest(x))
            return x
        rows += B.linear_case(shape, (0, 3), mode, hip=hip, restate=False, options=opt)
    for shape in (B.CHILD_WGRAD_SHAPES if mode == 0 else []):
        def hipw(d, a, wb):
            dw, db = R.ops.wgrad(d.cuda(), a.cuda(), wb)
            dw2, db2 = R.ops.wgrad(d.cuda(), a.cuda(), wb)
            assert torch.equal(dw, dw2) and torch.equal(db, db2), "second run differs"
            print("DIGEST", "wgrad", shape, mode, digest(dw, db))
            return dw, db
        rows += B.wgrad_case(shape, mode, True, hip=hipw, restate=False, options=opt)
    for cls, label, name, r, _ in rows:
        print(f"ROW {cls}|{label}|{name}|{r!r}")
        assert r <= B.BAR[cls], (label, name, r)
print("OK")
"""


def _child(env, modes):
    res = subprocess.run([sys.executable, "-c", CHILD, modes], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
    rows = [ln[4:].split("|") for ln in res.stdout.splitlines() if ln.startswith("ROW ")]
    digests = {ln.rsplit(" ", 1)[0]: ln.rsplit(" ", 1)[1] for ln in res.stdout.splitlines() if ln.startswith("DIGEST ")}
    return rows, digests


@pytest.fixture(scope="module")
def default_child():
    return _child({"REGT_FP32_CORE": "", "REGT_GEMM_DESC": ""}, "0,1,2")


def test_linear_and_wgrad_on_the_wide_fp32_core(default_child):
    """REGT_FP32_CORE=wide is read from the environment only: a fresh python child runs one full-tile and one ragged linear shape
    (gemm_flat_fast_kernel<FastCore>) and two weight gradients (wgrad_kernel<128>) in arithmetic 0.  The kernel names are
    expected_kernel's.  The results give no independent sign that the library honoured the variable: on the MI355X every output
    of these cases was bit-identical to the default core's (both cores carry the same k-ordered fp32 chain per element); the
    comparison is printed, not asserted, since no rule of the library promises it."""
    rows, dig = _child({"REGT_FP32_CORE": "wide"}, "0")
    for cls, label, name, r in rows:
        print(f"{label} [{name}] {cls}: r = {float(r):.3e}")
    assert {name.split(" ")[0] for _, _, name, _ in rows} == {"gemm_flat_fast_kernel<FastCore>", "wgrad_kernel<128>"}
    base = default_child[1]
    same = {k: dig[k] == base[k] for k in dig}
    print("bit-identical to the default core:", same)


def test_linear_with_the_descriptor_table_forced(default_child):
    """REGT_GEMM_DESC=table (environment only, fresh child): the LDS-table form of the split core at a K that would take scalar
    descriptors, in all three arithmetics.  That the variable was honoured rests on expected_kernel alone; the bitwise comparison
    with the default's results is printed."""
    rows, dig = _child({"REGT_GEMM_DESC": "table"}, "0,1,2")
    for cls, label, name, r in rows:
        print(f"{label} [{name}] {cls}: r = {float(r):.3e}")
    assert {name for cls, _, name, _ in rows if cls == "linear"} == {f"gemm_flat_split_kernel<{m}>/table" for m in (0, 3, 1)}
    print("bit-identical to the scalar-descriptor form:", {k: dig[k] == default_child[1][k] for k in dig})


@pytest.mark.parametrize("mode", B.MODES)
@pytest.mark.parametrize("with_bias", [True, False], ids=["dbias", "nodbias"])
@pytest.mark.parametrize("shape", B.WGRAD_CASES, ids=str)
def test_wgrad_per_element(R, shape, with_bias, mode):
    hip = _twice(lambda d, a, wb: R.ops.wgrad(d.cuda(), a.cuda(), wb))
    with _Mode(R, mode):
        _held(B.wgrad_case(shape, mode, with_bias, hip=hip, restate=False))


# ---- SpMM on the structured graph --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_graph():
    return tuple(t.cuda() for t in B.graph(B.SPMM_N))


@pytest.mark.parametrize("width", B.SPMM_WIDTHS)
def test_spmm_csr_per_element(R, small_graph, width):
    rp, col, va, vl = small_graph
    x = B.spmm_x(B.SPMM_N, width).cuda()
    name = B.expected_kernel("spmm_csr", 0, (B.SPMM_N, B.SPMM_N, width))
    rows = []
    for tag, val in (("A", va), ("L", vl)):
        got = _twice(lambda: R.ops.spmm_csr(rp, col, val, x))()
        rows.append(("spmm", f"spmm_csr n {B.SPMM_N} width {width} {tag}", name, B.spmm_ratio(got, B.csr_reference(rp, col, val, x)), None))
    _held(rows)


@pytest.mark.parametrize("width", B.DUAL_WIDTHS)
def test_spmm_dual_per_element(R, small_graph, width):
    rp, col, va, vl = small_graph
    x = B.spmm_x(B.SPMM_N, width).cuda()
    name = B.expected_kernel("spmm_dual", 0, (B.SPMM_N, width))
    ya, yl = _twice(lambda: R.ops.spmm_dual(rp, col, va, vl, x))()
    _held([("spmm", f"spmm_dual n {B.SPMM_N} width {width} {tag}", name, B.spmm_ratio(y, B.csr_reference(rp, col, val, x)), None)
           for tag, y, val in (("A", ya, va), ("L", yl, vl))])


# ---- the large-X branches: X above 24 MB, the degree plan embedded in 41003 nodes, a hub row past the row-block kernel's LDS ------

@pytest.fixture(scope="module")
def large_graph():
    return tuple(t.cuda() for t in B.graph(B.LARGE_N, B.HUB))


def _with_rows(R, on, f):
    lib = R.load_library()
    prev = lib.regt_set_option(b"spmm_rows", on)
    try:
        return f()
    finally:
        lib.regt_set_option(b"spmm_rows", prev)


@pytest.mark.parametrize("width", B.LARGE_WIDTHS)
def test_spmm_large_x_branches_per_element(R, large_graph, width):
    """Single operator, stacked operator (2 n rows over n rows of X) and dual form, each on the panel kernels and on the row-block
    kernel (spmm_rows = 1, restored): float64 from the CSR, and the row-block results bit-equal to the panel ones."""
    rp, col, va, vl = large_graph
    n = B.LARGE_N
    x = B.spmm_x(n, width).cuda()
    ref = {"A": B.csr_reference(rp, col, va, x), "L": B.csr_reference(rp, col, vl, x)}
    srp, scol, sval = B.stacked(rp, col, va, vl)
    rows, outs = [], {}
    for on in (0, 1):
        opt = {"spmm_rows": on}
        single = _with_rows(R, on, _twice(lambda: R.ops.spmm_csr(rp, col, vl, x)))
        stack = _with_rows(R, on, _twice(lambda: R.ops.spmm_csr(srp, scol, sval, x)))
        ya, yl = _with_rows(R, on, _twice(lambda: R.ops.spmm_dual(rp, col, va, vl, x)))
        outs[on] = (single, stack, ya, yl)
        k1 = B.expected_kernel("spmm_csr", 0, (n, n, width), opt)
        k2 = B.expected_kernel("spmm_csr", 0, (2 * n, n, width), opt)
        kd = B.expected_kernel("spmm_dual", 0, (n, width), opt)
        rows += [("spmm", f"spmm_csr n {n} width {width} L", k1, B.spmm_ratio(single, ref["L"]), None),
                 ("spmm", f"spmm_csr stacked 2 x {n} width {width} A", k2, B.spmm_ratio(stack[:n], ref["A"]), None),
                 ("spmm", f"spmm_csr stacked 2 x {n} width {width} L", k2, B.spmm_ratio(stack[n:], ref["L"]), None),
                 ("spmm", f"spmm_dual n {n} width {width} A", kd, B.spmm_ratio(ya, ref["A"]), None),
                 ("spmm", f"spmm_dual n {n} width {width} L", kd, B.spmm_ratio(yl, ref["L"]), None)]
    _held(rows)
    assert all(torch.equal(p, q) for p, q in zip(outs[0], outs[1])), "row-block kernel differs from the panel kernel"


@pytest.mark.parametrize("width", B.LARGE_BF16_WIDTHS)
def test_spmm_dual_bf16_rows_per_element(R, large_graph, width):
    """bf16 rows: the stored value is one RNE rounding of an fp32 sum that is inside the spmm bar (per element), on the panel and on the
    row-block kernel, and bit-equal to the fp32 dual kernel's result rounded once (which also pins the direction on ties)."""
    rp, col, va, vl = large_graph
    n = B.LARGE_N
    x = B.spmm_x(n, width, bf16=True).cuda()
    ref = {"A": B.csr_reference(rp, col, va, x), "L": B.csr_reference(rp, col, vl, x)}
    fa, fl = R.ops.spmm_dual(rp, col, va, vl, x.float().contiguous())
    rows = [("spmm", f"spmm_dual n {n} width {width} (bf16 values) {tag}", B.expected_kernel("spmm_dual", 0, (n, width)), B.spmm_ratio(y, ref[tag]), None)
            for tag, y in (("A", fa), ("L", fl))]
    for on in (0, 1):
        ya, yl = _with_rows(R, on, _twice(lambda: R.ops.spmm_dual_bf16(rp, col, va, vl, x)))
        name = B.expected_kernel("spmm_dual_bf16", 0, (n, n, width), {"spmm_rows": on})
        rows += [("bf16_store", f"spmm_dual_bf16 n {n} width {width} {tag}", name, B.bf16_store_ratio(y, ref[tag]), None)
                 for tag, y in (("A", ya), ("L", yl))]
        assert torch.equal(ya, fa.to(torch.bfloat16)) and torch.equal(yl, fl.to(torch.bfloat16)), name
    _held(rows)
