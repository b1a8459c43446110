"""The cell-only entry points (regt_tgcn_*) on a host without a GPU: the float64 restatement behind the device tests against the
reference's golden and the oracle under autograd, the three symbols, and every refusal the header lists -- none touches a device pointer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import regtgcn_amd as R
import tgcn_math as TM
from conftest import load_npz
from oracle import model as M
from regtgcn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-6          # tests/test_oracle_goldens.py: the oracle against the same golden
NEW = ("regt_tgcn_workspace_bytes", "regt_tgcn_forward", "regt_tgcn_backward")


def _golden():
    g = load_npz("golden_cell.npz")
    p = {k[3:].replace("__", "."): torch.from_numpy(v) for k, v in g.items() if k.startswith("p__")}
    return g, p, torch.from_numpy(g["edge_index"]), torch.from_numpy(g["edge_weight"]), torch.from_numpy(g["x"]), torch.from_numpy(g["h"])


@pytest.mark.parametrize("tag", ["unit", "weighted"])
def test_restatement_reproduces_the_cell_golden(tag):
    g, p, ei, ew, x, h = _golden()
    p64 = {k: v.double() for k, v in p.items()}
    a = TM.dense_from_edges(ei, None if tag == "unit" else ew, x.shape[0])
    s = TM.step(p64, a, x.double(), h.double())
    np.testing.assert_allclose(s["out"].numpy(), g[f"out_{tag}"], atol=TOL)
    _dx, _dh, grads = TM.backward(p64, a, s, 2 * s["out"])              # loss = (out ** 2).sum(), as the golden's
    assert sorted(grads) == sorted(p)
    for name, got in grads.items():
        np.testing.assert_allclose(got.numpy(), g[f"g_{tag}__" + name.replace(".", "__")], atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize("tag", ["unit", "weighted"])
def test_restatement_dx_dh_are_autograd_through_the_oracle_cell(tag):
    _g, p, ei, ew, x, h = _golden()
    w = None if tag == "unit" else ew.double()
    p64 = {k: v.double() for k, v in p.items()}
    xl, hl = x.double().requires_grad_(True), h.double().requires_grad_(True)
    pl = {k: v.clone().requires_grad_(True) for k, v in p64.items()}
    out = M.tgcn_cell(pl, "", xl, ei, w, hl)
    gen = torch.Generator().manual_seed(3)
    d = torch.randn(out.shape, generator=gen, dtype=torch.float64)
    (out * d).sum().backward()
    a = TM.dense_from_edges(ei, w, x.shape[0])
    s = TM.step(p64, a, x.double(), h.double())
    dx, dh, grads = TM.backward(p64, a, s, d)
    np.testing.assert_allclose(s["out"].numpy(), out.detach().numpy(), atol=1e-13)
    np.testing.assert_allclose(dx.numpy(), xl.grad.numpy(), atol=1e-12, rtol=1e-12)
    np.testing.assert_allclose(dh.numpy(), hl.grad.numpy(), atol=1e-12, rtol=1e-12)
    for name in TM.NAMES:
        np.testing.assert_allclose(grads[name].numpy(), pl[name].grad.numpy(), atol=1e-12, rtol=1e-12)
    # H = None is H = zeros
    np.testing.assert_array_equal(TM.step(p64, a, x.double(), None)["out"].numpy(), TM.step(p64, a, x.double(), torch.zeros_like(hl))["out"].numpy())


def test_unrolled_restatement_is_autograd_through_the_oracle_cell():
    _g, p, ei, ew, x, h = _golden()
    p64 = {k: v.double() for k, v in p.items()}
    gen = torch.Generator().manual_seed(5)
    xs = [torch.rand(x.shape, generator=gen, dtype=torch.float64).requires_grad_(True) for _ in range(3)]
    h0 = h.double().requires_grad_(True)
    pl = {k: v.clone().requires_grad_(True) for k, v in p64.items()}
    hh = h0
    for xt in xs:
        hh = M.tgcn_cell(pl, "", xt, ei, ew.double(), hh)
    (hh ** 2).sum().backward()
    a = TM.dense_from_edges(ei, ew, x.shape[0])
    last, dh0, dxs, grads = TM.unroll(p64, a, [t.detach() for t in xs], h.double())
    np.testing.assert_allclose(last.numpy(), hh.detach().numpy(), atol=1e-13)
    np.testing.assert_allclose(dh0.numpy(), h0.grad.numpy(), atol=1e-11, rtol=1e-11)
    for t in range(3):
        np.testing.assert_allclose(dxs[t].numpy(), xs[t].grad.numpy(), atol=1e-11, rtol=1e-11)
    for name in TM.NAMES:
        np.testing.assert_allclose(grads[name].numpy(), pl[name].grad.numpy(), atol=1e-11, rtol=1e-11)


def test_symbols_in_header_bindings_and_library():
    lib = R.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "regtgcn.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/regtgcn.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert lib.regt_abi_version() == 8 == _lib.ABI_VERSION
    assert "#define REGT_ABI_VERSION 8" in open(os.path.join(ROOT, "include", "regtgcn.h")).read()


# ---- refusals: fake, aligned, never dereferenced device pointers --------------------------------------------------------------------------
P = 1 << 20           # a 16-byte aligned stand-in for a device pointer
N, F, C = 10, 8, 16


def _dims(n=N, t=1, f=F, c=C, regional=0, arith=_lib.ARITH_FP32, flags=0):
    return _lib.Dims(n, t, f, c, 0, 0, 0, regional, 0.0, arith, flags)          # R, O, H1 = 0: ignored


def _graph():
    g = _lib.Graph()
    g.rowptr, g.col, g.val = P, P, P
    return g


def _tables(cls):
    s = cls()
    for i in range(3):
        s.conv_lin_w[i], s.conv_bias[i], s.gate_w[i], s.gate_b[i] = P, P, P, P
    return s


def _fwd(lib, d, g=None, ps=None, x=P, h_in=P, h_out=P, ws=P, wsb=None):
    g, ps = g or _graph(), ps or _tables(_lib.Params)
    wsb = lib.regt_tgcn_workspace_bytes(ctypes.byref(_dims())) if wsb is None else wsb
    return lib.regt_tgcn_forward(ctypes.byref(d), ctypes.byref(g), ctypes.byref(ps), x, h_in, h_out, ws, wsb, None)


def _bwd(lib, d, gr=None, dh_out=P, h_in=P, h_out=P, t=(P, P, P), dx=P, dh_in=P, ws=P, wsb=None, ps=None):
    g, ps, gr = _graph(), ps or _tables(_lib.Params), gr or _tables(_lib.Grads)
    wsb = lib.regt_tgcn_workspace_bytes(ctypes.byref(_dims())) if wsb is None else wsb
    return lib.regt_tgcn_backward(ctypes.byref(d), ctypes.byref(g), ctypes.byref(ps), ctypes.byref(gr), dh_out, h_in, h_out, t[0], t[1], t[2],
                                  dx, dh_in, ws, wsb, None)


def _refused(lib, rc, *words):
    msg = lib.regt_last_error()
    assert rc != 0 and msg, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_workspace_sizes():
    lib = R.load_library()
    full = lib.regt_tgcn_workspace_bytes(ctypes.byref(_dims()))
    fwd = lib.regt_tgcn_workspace_bytes(ctypes.byref(_dims(flags=_lib.DIMS_FORWARD_ONLY)))
    assert 0 < fwd < full
    assert full >= N * C * 4 * 9                                   # the training layout's nine (N x C) element arrays
    for bad, word in ((_dims(t=2), "T="), (_dims(regional=1), "regional"), (_dims(c=18), "multiple of 4"), (_dims(f=7), "multiple of 4"),
                      (_dims(arith=_lib.ARITH_BF16), "bf16")):
        assert lib.regt_tgcn_workspace_bytes(ctypes.byref(bad)) == 0
        assert word.encode() in lib.regt_last_error()
    assert lib.regt_tgcn_workspace_bytes(None) == 0 and lib.regt_last_error()


def test_forward_refusals_touch_no_device_pointer():
    lib = R.load_library()
    _refused(lib, _fwd(lib, _dims(t=2)), "T=2")
    _refused(lib, _fwd(lib, _dims(regional=1)), "regional")
    _refused(lib, _fwd(lib, _dims(c=18)), "multiple of 4")
    _refused(lib, _fwd(lib, _dims(arith=_lib.ARITH_BF16)), "bf16")
    _refused(lib, _fwd(lib, _dims(), x=None), "NULL")
    _refused(lib, _fwd(lib, _dims(), h_out=None), "NULL")
    _refused(lib, _fwd(lib, _dims(), ws=None), "NULL")
    ps = _tables(_lib.Params)
    ps.gate_w[1] = None
    _refused(lib, _fwd(lib, _dims(), ps=ps), "gate_w")
    g = _lib.Graph()
    _refused(lib, _fwd(lib, _dims(), g=g), "graph")
    _refused(lib, _fwd(lib, _dims(), h_out=P + 4), "16-byte")
    need = lib.regt_tgcn_workspace_bytes(ctypes.byref(_dims()))
    _refused(lib, _fwd(lib, _dims(), wsb=need - 1), "workspace")
    fo = lib.regt_tgcn_workspace_bytes(ctypes.byref(_dims(flags=_lib.DIMS_FORWARD_ONLY)))
    _refused(lib, _fwd(lib, _dims(flags=_lib.DIMS_FORWARD_ONLY), wsb=fo - 1), "workspace")
    _refused(lib, _fwd(lib, _dims(), wsb=fo), "workspace")         # the training call needs the training size


def test_backward_refusals_touch_no_device_pointer():
    lib = R.load_library()
    _refused(lib, _bwd(lib, _dims(t=3)), "T=3")
    _refused(lib, _bwd(lib, _dims(regional=1)), "regional")
    _refused(lib, _bwd(lib, _dims(c=18)), "multiple of 4")
    _refused(lib, _bwd(lib, _dims(arith=_lib.ARITH_BF16)), "bf16")
    _refused(lib, _bwd(lib, _dims(), dh_out=None), "NULL")
    _refused(lib, _bwd(lib, _dims(), h_out=None), "NULL")
    _refused(lib, _bwd(lib, _dims(), ws=None), "NULL")
    gr = _tables(_lib.Grads)
    gr.conv_bias[2] = None
    _refused(lib, _bwd(lib, _dims(), gr=gr), "conv_bias")
    _refused(lib, _bwd(lib, _dims(), t=(None, None, None)), "transposed")
    _refused(lib, _bwd(lib, _dims(), t=(P, P, None)), "transposed")
    _refused(lib, _bwd(lib, _dims(), dx=P + 8), "16-byte")
    _refused(lib, _bwd(lib, _dims(), dh_in=P + 4), "16-byte")
    _refused(lib, _bwd(lib, _dims(), h_out=P + 4), "16-byte")
    need = lib.regt_tgcn_workspace_bytes(ctypes.byref(_dims()))
    _refused(lib, _bwd(lib, _dims(), wsb=need - 1), "workspace")
    _refused(lib, _bwd(lib, _dims(flags=_lib.DIMS_FORWARD_ONLY)), "FORWARD_ONLY")


def test_module_surface_on_the_host():
    """The reference's signature; CPU tensors and the other base blocks are refused with the documented errors; the state_dict is unchanged."""
    cell = R.nn.TGCN(8, 16)
    assert list(cell.state_dict()) == [f"{m}.{s}" for k in "zrh" for m, s in ((f"conv_{k}", "bias"), (f"conv_{k}", "lin.weight"),
                                                                             (f"linear_{k}", "weight"), (f"linear_{k}", "bias"))]
    x, ei = torch.zeros(10, 8), torch.zeros(2, 0, dtype=torch.long)
    with pytest.raises(R.RegtError):
        cell(x, ei)
    with pytest.raises(R.RegtError):
        cell(x, ei, None, torch.zeros(10, 16))
    for block, owner in (("gat", "GATTemporal"), ("graphsage", "GraphSAGETemporalGCN")):
        with pytest.raises(NotImplementedError, match=owner):
            R.nn.TGCN(8, 16, baseblock=block)(x, ei, None, torch.zeros(10, 16))
    with pytest.raises(R.RegtError):
        R.nn.A3TGCN(8, 16, 3)(torch.zeros(10, 8, 3), ei, None, None)
    with pytest.raises(R.RegtError):
        R.nn.RegionalA3TGCN(8, 16, 10, 3, num_regions=2)(torch.zeros(10, 8, 3), ei, ei, ei, None, None)
    with pytest.raises(TypeError):
        R.nn.RegionalA3TGCN(8, 16, 10, 3, num_regions=2)(torch.zeros(10, 8, 3), ei, ei)
