"""The whole-model input gradient (regt_input_gradient) on a host without a GPU: the float64 restatement of its five formulas
(tests/input_grad_math.py) against torch.autograd through the oracle for both models, the input conditions of the device test (a missing
transpose cannot pass; no head relu sits on its edge), the bar derived from the fp32 restatement, the two symbols, and every refusal the
header lists that needs no earlier device call -- none touches a device pointer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cell_probe as CP
import input_grad_math as IG
import regtgcn_amd as R
from regtgcn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("regt_input_gradient_scratch_bytes", "regt_input_gradient")


# ---- the formulas ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(IG.CASES))
def test_restatement_is_autograd_through_the_oracle(name):
    ref = IG.reference(name)
    c = IG.CASES[name]
    assert tuple(ref["dx"].shape) == (c["n"] * c["copies"], c["f"], c["t"])
    scale = float(ref["dx"].abs().max())
    assert scale > 0
    # the formulas in float64 against the oracle's autograd: the algebra is exact
    np.testing.assert_allclose(ref["r64"].numpy(), ref["dx"].numpy(), atol=1e-11 * scale, rtol=1e-9)
    np.testing.assert_allclose(ref["fused_autograd64"].numpy(), ref["dx"].numpy(), atol=1e-11 * scale, rtol=1e-9)


def test_both_forms_of_temporal_gcn_and_both_models_are_covered():
    forms = {(c["model"], bool(c["collapse"]) if c["model"] == "tgcn" else None) for c in IG.CASES.values()}
    assert forms == {("regional", None), ("tgcn", True), ("tgcn", False)}
    assert {c["mode"] for c in IG.CASES.values()} == {0, 1}
    assert {(c["n"], c["t"]) for c in IG.CASES.values()} == {(130, 1), (43, 3), (9, 150)}
    assert {c["c"] for c in IG.CASES.values()} == {16, 48, 256}
    assert {c["f"] for c in IG.CASES.values()} == {7, 8, 32, 36, 64}
    assert any(c["copies"] == 2 for c in IG.CASES.values())
    assert {(c["r"], c["order"]) for c in IG.CASES.values() if c["model"] == "regional"} == {(1, "sorted"), (3, "sorted"), (3, "shuffled")}


@pytest.mark.parametrize("name", [k for k, c in IG.CASES.items() if c["model"] == "regional" and c["r"] > 1])
def test_region_ids_are_sorted_or_shuffled_as_named(name):
    ei, _ew, ri, _rw, n = IG.full_graph(name)
    owner = R.graph.node_regions(ri, n)
    ascending = bool(np.all(owner[1:] >= owner[:-1]))
    c = IG.CASES[name]
    assert ascending == (c["order"] == "sorted" and c["copies"] == 1), name     # (copies repeat the ascending run: a region boundary per copy)
    assert len(set(owner.tolist())) == c["r"]


# ---- input conditions of the device test ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(IG.CASES))
def test_a_missing_transpose_cannot_pass(name):
    """The float64 dx computed with the UNTRANSPOSED operators is off by more than 100 x the bar on at least one row."""
    ref = IG.reference(name)
    err, scale = CP.row_stats(IG.rows(ref["plain64"]), IG.rows(ref["dx"]))
    assert float(CP.row_ratio(err, scale).max()) > 100 * IG.bar(), name
    ei, ew, _ri, rw, _n = IG.full_graph(name)
    for w in ([ew] if ew is not None else []) + list(rw):
        assert float(w.max() - w.min()) > 0.1                                      # asymmetric weights


@pytest.mark.parametrize("name", list(IG.CASES))
def test_no_head_relu_sits_on_its_edge(name):
    """No element of the float64 hidden state or of the head's inner pre-activation is close enough to 0 for an fp32 result inside the
    bars to take the relu on the other side: the float64 reference is the one reference."""
    assert IG.reference(name)["edge"] > IG.EDGE, name


def test_structural_rows_of_the_graph():
    ei, _w = IG.base_graph(43, 1)
    n = 43
    src, dst = ei
    assert not bool(((src == n - 1) | (dst == n - 1) | (src == n - 2) | (dst == n - 2)).any())       # two isolated nodes
    assert bool((dst == n - 3).any()) and not bool((src == n - 3).any())                               # in-edges only
    assert bool((src == 0).any()) and not bool((dst == 0).any())                                       # out-edges only
    assert bool((src == dst).any())                                                                    # a self loop
    pairs = (src * n + dst).tolist()
    assert len(set(pairs)) < len(pairs)                                                                # a duplicate edge
    # an isolated node's gradient is its own term alone, and it is not zero
    ref = IG.reference("regt-N43-T3-F7-C48-shuffled")
    assert float(ref["dx"][n - 1].abs().max()) > 0


# ---- the bar ----------------------------------------------------------------------------------------------------------------------------------

def test_bar_follows_from_the_fp32_restatement():
    measured = IG.measured_fp32()
    worst = max(measured.values())
    print({k: f"{v:.3e}" for k, v in measured.items()})
    print(f"worst fp32 restatement row ratio {worst:.3e}; x {IG.ORDER_FACTOR:g} = {IG.ORDER_FACTOR * worst:.3e}; cell_probe dh_in bar {CP.BAR['dh_in']:.3e}")
    assert 0 < worst < 1e-4
    want = CP.BAR["dh_in"] if IG.ORDER_FACTOR * worst <= CP.BAR["dh_in"] else IG.ORDER_FACTOR * worst
    assert IG.bar() == want
    assert IG.bar() <= CP.CAP
    # the fp32 restatement itself is held by it, with the x 4 to spare
    for name in IG.CASES:
        assert IG.ORDER_FACTOR * measured[name] <= IG.bar(), name


# ---- symbols ----------------------------------------------------------------------------------------------------------------------------------

def test_symbols_in_header_bindings_and_library():
    lib = R.load_library()
    text = open(os.path.join(ROOT, "include", "regtgcn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/regtgcn.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert lib.regt_abi_version() == 8 == _lib.ABI_VERSION                       # additive entries
    assert "#define REGT_ABI_VERSION 8" in text
    import regtgcn_amd.build as B
    assert "model_dx.hip" in B.SOURCES and "spmm_dual_t.hip" in B.SOURCES


def test_transpose_csr_carries_further_value_arrays():
    rowptr = torch.tensor([0, 2, 2, 5], dtype=torch.int32)
    col = torch.tensor([1, 2, 0, 1, 1], dtype=torch.int32)
    va = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0])
    vl = -va
    t3 = R.graph.transpose_csr(rowptr, col, va, 3, 3)
    t4 = R.graph.transpose_csr(rowptr, col, va, 3, 3, vl)
    assert len(t3) == 3 and len(t4) == 4
    assert all(torch.equal(u, v) for u, v in zip(t3, t4[:3]))
    assert torch.equal(t4[3], -t4[2])
    assert t4[0].tolist() == [0, 1, 4, 5] and t4[1].tolist() == [2, 0, 2, 2, 0] and t4[2].tolist() == [3.0, 1.0, 4.0, 5.0, 2.0]


# ---- refusals: fake, aligned, never dereferenced device pointers --------------------------------------------------------------------------------
P = 1 << 20
N, T, F, C = 10, 3, 8, 16


def _dims(n=N, t=T, f=F, c=C, r=1, regional=1, arith=_lib.ARITH_FP32, flags=0):
    return _lib.Dims(n, t, f, c, r, 1, 4, regional, 0.01, arith, flags)


def _graph(overlap=0, node_region=P):
    g = _lib.Graph()
    g.rowptr, g.col, g.val, g.node_region = P, P, P, node_region
    g.overlap = overlap
    return g


def _params(regional=True):
    s = _lib.Params()
    for i in range(3):
        s.conv_lin_w[i], s.conv_bias[i], s.gate_w[i], s.gate_b[i] = P, P, P, P
    s.attention = s.cheb_w0 = s.cheb_w1 = s.cheb_bias = s.head1_w = s.head1_b = s.head2_w = s.head2_b = P
    if regional:
        s.region_w = s.region_b = P
    return s


def _call(lib, d, g=None, ps=None, t=(P, P, P, P), dx=P, ws=P, wsb=None, scratch=P, sb=None):
    g, ps = g or _graph(), ps or _params()
    base = _dims()
    wsb = lib.regt_workspace_bytes(ctypes.byref(base), 0, 0) if wsb is None else wsb
    sb = lib.regt_input_gradient_scratch_bytes(ctypes.byref(base)) if sb is None else sb
    return lib.regt_input_gradient(ctypes.byref(d), ctypes.byref(g), ctypes.byref(ps), t[0], t[1], t[2], t[3], dx, ws, wsb, scratch, sb, None)


def _refused(lib, rc, *words):
    msg = lib.regt_last_error()
    assert rc != 0 and msg, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_scratch_size():
    lib = R.load_library()
    need = lib.regt_input_gradient_scratch_bytes(ctypes.byref(_dims()))
    assert need >= 3 * N * T * F * 4 and need % 256 == 0
    assert lib.regt_input_gradient_scratch_bytes(ctypes.byref(_dims(flags=_lib.DIMS_NO_HEAD))) == need
    for bad, word in ((_dims(arith=_lib.ARITH_BF16), "bf16"), (_dims(f=68), "F <= 64"), (_dims(f=7), "multiple of 4"), (_dims(t=256), "T=256"),
                      (_dims(flags=_lib.DIMS_FORWARD_ONLY), "FORWARD_ONLY")):
        assert lib.regt_input_gradient_scratch_bytes(ctypes.byref(bad)) == 0
        assert word.encode() in lib.regt_last_error()
    assert lib.regt_input_gradient_scratch_bytes(None) == 0 and lib.regt_last_error()
    # the step's own workspace is what it was
    assert lib.regt_workspace_bytes(ctypes.byref(_dims()), 0, 0) > 0


def test_refusals_touch_no_device_pointer():
    lib = R.load_library()
    _refused(lib, _call(lib, _dims(arith=_lib.ARITH_BF16)), "bf16")
    _refused(lib, _call(lib, _dims(f=68)), "F <= 64")
    _refused(lib, _call(lib, _dims(c=18)), "multiple of 4")
    _refused(lib, _call(lib, _dims(flags=_lib.DIMS_FORWARD_ONLY)), "FORWARD_ONLY")
    _refused(lib, _call(lib, _dims(), g=_graph(overlap=1)), "overlap")
    _refused(lib, _call(lib, _dims(r=3), g=_graph(node_region=None)), "node_region")
    ps = _params()
    ps.cheb_w1 = None
    _refused(lib, _call(lib, _dims(), ps=ps), "NULL")
    _refused(lib, _call(lib, _dims(), t=(None, None, None, None)), "transposed")
    _refused(lib, _call(lib, _dims(), t=(P, P, P, None)), "transposed")
    _refused(lib, _call(lib, _dims(), dx=None), "NULL")
    _refused(lib, _call(lib, _dims(), ws=None), "NULL")
    _refused(lib, _call(lib, _dims(), scratch=None), "NULL")
    _refused(lib, _call(lib, _dims(), dx=P + 4), "16-byte")
    _refused(lib, _call(lib, _dims(), scratch=P + 8), "16-byte")
    _refused(lib, _call(lib, _dims(), ws=P + 4), "16-byte")
    need = lib.regt_workspace_bytes(ctypes.byref(_dims()), 0, 0)
    _refused(lib, _call(lib, _dims(), wsb=need - 1), "workspace")
    sb = lib.regt_input_gradient_scratch_bytes(ctypes.byref(_dims()))
    _refused(lib, _call(lib, _dims(), sb=sb - 1), "scratch")
    lib_null = lib.regt_input_gradient(None, None, None, P, P, P, P, P, P, need, P, sb, None)
    _refused(lib, lib_null, "dims")
    g = lib.regt_input_gradient(ctypes.byref(_dims()), None, ctypes.byref(_params()), P, P, P, P, P, P, need, P, sb, None)
    _refused(lib, g, "graph")
