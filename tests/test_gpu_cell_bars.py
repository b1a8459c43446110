"""The GRU cell behind regt_cell_forward / regt_cell_backward (functional.CellFunction on a prepare_gcn_operator graph) held to the
per-row bars of tests/cell_probe.py: ``hidden`` and ``pred`` per node, ``dh_in`` -- the output of cell_bwd, dgrad_candidate and
dgrad_gates with no reduction over rows in between -- per (node, period) row, against float64 from the same inputs.  Every case of the
table x probe runs in both fp32-storage arithmetics (regt_set_gemm_mode, restored) and under each data-gradient form that a runtime
switch selects for them (regt_set_option("dgrad1_gen", .), restored: DESIGN.md 6b), labelled with cell_probe.expected_forms (the kernel
that ran is not read back).  Every run is repeated and must be bit-identical, except at T > 64, where DESIGN.md records the float
atomics into ``hidden`` as ordered by arrival.  profiles/cell_bars.txt holds every measured ratio (tools/cell_bars.py)."""
import pytest
import torch

import cell_probe as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import regtgcn_amd
    regtgcn_amd.load_library()
    return regtgcn_amd


@pytest.mark.parametrize("probe", P.PROBES)
@pytest.mark.parametrize("name", list(P.CASES))
def test_cell_rows_are_inside_their_bars(R, name, probe):
    lib = R.load_library()
    mode0, gen0 = lib.regt_set_gemm_mode(0), lib.regt_set_option(b"dgrad1_gen", 1)
    lib.regt_set_gemm_mode(mode0)
    lib.regt_set_option(b"dgrad1_gen", gen0)
    bad = []
    for mode, gen in P.runs(name):
        m = P.measure(R, name, probe, mode, gen)
        for tensor, r in m["ratios"].items():
            print(f"{name} {probe} mode {mode} dgrad1_gen {gen} [{P.form_label(m['forms'])}] {tensor}: r = {r:.3e} "
                  f"(bar {P.BAR[P.klass(tensor, probe)]:.3e})")
        for line in m["named"]:
            print("named:", line)
        bad += m["bad"]
        if m["identical"] is not None:
            assert m["identical"], f"{name} {probe} mode {mode} dgrad1_gen {gen}: two runs differ"
        if probe == "blend":
            print(f"{name} blend mode {mode} dgrad1_gen {gen}: dh_in against dhn32 * z32 per element r = {m['blend']:.3e}")
            assert m["blend"] <= P.BAR["dh_in_blend"], (name, mode, gen, m["blend"])
        if probe != "saturated":
            assert not any("ill-conditioned" in line for line in m["named"]), m["named"]
    assert not bad, bad[:8]
    # the switches are back where they were
    assert lib.regt_set_gemm_mode(mode0) == mode0 and lib.regt_set_option(b"dgrad1_gen", gen0) == gen0


def test_padded_feature_rows_are_what_the_unpadded_reference_sees(R):
    """M129-T3 has F = 7: the device runs it with one zero feature row and zero weight columns; the float64 reference never pads."""
    x, _h, _gh, _gp = P.inputs("M129-T3")
    assert x.shape[1] == 7 and P.expected_forms(P.CASES["M129-T3"], 0)["gates"] == "gemm_flat_kernel<vec=1>"
    _op, csr = P.device_case(R, "M129-T3")
    host = P.cpu_csr("M129-T3")
    # the library's operator and the oracle's normalisation describe the same matrix (entry order within a row may differ)
    a = torch.zeros(43, 43, dtype=torch.float64)
    b = torch.zeros(43, 43, dtype=torch.float64)
    for mat, (rp, col, val) in ((a, csr), (b, host)):
        rows = torch.repeat_interleave(torch.arange(43), (rp[1:] - rp[:-1]).long())
        mat.index_put_((rows, col.long()), val.double(), accumulate=True)
    assert float((a - b).abs().max()) <= 2.0 ** -22
