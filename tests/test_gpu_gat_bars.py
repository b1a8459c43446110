"""The kernels of csrc/gat.hip (gat_fwd_kernel, gat_bwd_dst_kernel, gat_bwd_src_kernel) held to the per-row bars of
tests/gat_math.py on every case of gat_math.CASES: out, the four saved statistics (m, l, d and, after the backward, D) and both
columns of dsd against the sparse float64 reference of the same fp32 inputs, never against another kernel.  Every case is labelled
with gat_math.kernel_name (a restatement of pick_group).  profiles/gat_bars.txt holds every case's measured ratio."""
import numpy as np
import pytest
import torch

import gat_math as G
import op_bars

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd
    regtgcn_amd.load_library()
    return regtgcn_amd


def _case(R, c):
    """(inputs, pattern, float64 reference, HIP results) with the pattern checked against the host's restatement of it."""
    inp = G.inputs(c)
    cpu = G.cpu_pattern(inp.ei, c.n)
    rows, src_rows = G.case_rows(c, cpu)
    pat, got, fwd_d = G.run_hip(R, c, inp, rows, src_rows)
    for name, a, b in zip(("rowptr", "col", "t_rowptr", "t_col"), pat, cpu):
        assert np.array_equal(a, b), f"{c.name}: {name} of prepare_attention_pattern differs from gat_math.cpu_pattern"
    assert not fwd_d.any(), f"{c.name}: stats[:, 3] is not 0 after the forward alone"
    return inp, pat, G.reference(inp, pat, rows, src_rows), got


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_gat_rows_inside_their_bars(R, name):
    c = G.CASE[name]
    inp, pat, ref, got = _case(R, c)
    bad = []
    for cls, label, kernel, r, where in G.measure(c, inp, pat, ref, got):
        print(f"{label} [{kernel}] {cls}: r = {r:.3e} (bar {G.BAR[cls]:.3e}) at {where}")
        if not r <= G.BAR[cls]:
            bad.append((cls, r, G.BAR[cls], where, kernel))
    assert not bad, (name, bad)
    # the exact facts
    x = inp.x.reshape(-1, c.f)
    deg = np.diff(ref["start"])
    if c.small:
        lone = np.nonzero(deg == 1)[0]                          # the self loop alone: out = x_i, l = 1, dd = 0
        assert lone.size == (1 if c.kind == "single" else 2 * c.t)
        assert np.array_equal(got["out"][lone], x[lone]) and (got["l"][lone] == 1).all() and (got["dd"][lone] == 0).all(), name
        # a node that sends no edge either (the last one): ds_i is its own self-loop term, alpha = 1 and g - D = 0 recomputed by
        # gat_bwd_src_kernel from the saved (m, l, D), exactly 0
        only_self = lone[np.diff(pat[2].astype(np.int64))[lone // c.t] == 1]
        assert only_self.size == c.t and (got["ds"][only_self] == 0).all(), name
    if c.regime == "zero":                                       # uniform attention: m = d = 0 and l = degree exactly, out is the row mean
        assert (got["m"] == 0).all() and (got["d"] == 0).all() and np.array_equal(got["l"], deg.astype(np.float32)), name
        x64 = x.astype(np.float64)
        mean = np.add.reduceat(x64[ref["src"]], ref["start"][:-1], axis=0) / deg[:, None]
        mean_abs = np.add.reduceat(np.abs(x64[ref["src"]]), ref["start"][:-1], axis=0) / deg[:, None]
        assert G._worst(np.abs(got["out"] - mean), mean_abs)[0] <= G.BAR["out"], name
    if c.regime == "gap":                                        # alpha is exactly 0 / 1 on the hub's rows
        hub = np.arange(c.t)
        assert np.array_equal(got["out"][hub], inp.x[G.GAP_SOURCE]) and (got["l"][hub] == 1).all(), name
        assert (got["dd"][hub] == 0).all(), name                # de = 1 * (g - D) with D = g, and 0 * ... for every other entry


@pytest.mark.parametrize("name", G.DU_CASES)
def test_score_vector_gradients_end_to_end(R, name):
    """du_src, du_dst through GatAggregateFunction (gat_backward, then the weight-gradient kernel on the (N T, 2, F) shape)."""
    c = G.CASE[name]
    inp = G.inputs(c)
    dev = torch.device("cuda")
    pattern = R.graph.prepare_attention_pattern(torch.from_numpy(inp.ei).to(dev), c.n)
    us = torch.from_numpy(inp.us).to(dev).requires_grad_(True)
    ud = torch.from_numpy(inp.ud).to(dev).requires_grad_(True)
    out = R.functional.GatAggregateFunction.apply(torch.from_numpy(inp.x).to(dev), us, ud, pattern, G.SLOPE)
    out.backward(torch.from_numpy(inp.dout).to(dev))
    pat = tuple(t.cpu().numpy() for t in (pattern.rowptr, pattern.col, pattern.t_rowptr, pattern.t_col))
    r = G.du_ratios(G.reference(inp, pat), inp, us.grad.cpu().numpy(), ud.grad.cpu().numpy())
    for key, val in r.items():
        bar = G.BAR[key] + op_bars.BAR["wgrad"]
        print(f"{name} [{G.kernel_name(c.f)}] du from {key}: r = {val:.3e} (bar {bar:.3e})")
        assert val <= bar, (name, key, val, bar)
