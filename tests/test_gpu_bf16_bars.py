"""The bf16 arithmetic (regt_set_gemm_mode(2)) of RegionalTemporalGCN and TemporalGCN held to the per-row and per-node bars of
tests/bf16_probe.py against float64 alone: ``hidden`` and ``pred`` per node, every parameter gradient under an upstream gradient that
lives on one probe node (node 0, the last node, the node across row 128, a node of the partial last tile, the first node of the second
region, a node without in-edge) and once under a dense one.  Every case runs under each option set that changes its form
(regt_set_option("xbf" / "fused_bwd" / "fused_rows", .) and REGT_DIMS_NO_BF16_ROWS on the call; all put back and checked), labelled with
bf16_probe.expected_forms (the kernel that ran is not read back).  Every forward is repeated per probe and the dense backward twice:
all must be bit-identical (T <= 64 everywhere here: DESIGN.md section 5, Determinism).  profiles/bf16_bars.txt holds every measured
ratio (tools/bf16_bars.py)."""
import pytest

import bf16_probe as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd
    regtgcn_amd.load_library()
    return regtgcn_amd


def _settings(lib):
    mode = lib.regt_set_gemm_mode(0)
    lib.regt_set_gemm_mode(mode)
    opts = {}
    for k in P.LIB_OPTIONS:
        opts[k] = lib.regt_set_option(k.encode(), 1)
        lib.regt_set_option(k.encode(), opts[k])
    return mode, opts


@pytest.mark.parametrize("name,key", [(name, key) for name in P.CASES for key in P.runs(name)])
def test_bf16_rows_and_probe_nodes_are_inside_their_bars(R, name, key):
    lib = R.load_library()
    before = _settings(lib)
    m = P.measure(R, name, key)
    label = P.form_label(m["forms"])
    for what, cls, r, ill in m["ratios"]:
        print(f"{name} {key} [{label}] {what}: r = {r:.3e} (bar {P.BAR[cls]:.3e}{', ill-conditioned: held to 4 x its gap' if ill else ''})")
    for line in m["named"]:
        print("named:", line)
    assert not m["bad"], m["bad"][:8]
    assert m["identical"], f"{name} {key}: two runs differ"
    assert _settings(lib) == before                    # the arithmetic and the switches are back where they were
