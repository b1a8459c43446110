"""Forward-only calls (REGT_DIMS_FORWARD_ONLY, regt_forward_only_workspace_bytes): what can be checked without a GPU -- the symbol,
the workspace sizes of the two layouts against the training layout, the host-side refusals.  The sizing function reads only host
fields of regt_graph (and whether pointers are NULL), so dummy non-NULL pointers stand in for device arrays here."""
import ctypes as C

import pytest

from regtgcn_amd import _lib

DUMMY = 0x1000      # never dereferenced


def _dims(arith, F, R, flags=0, **over):
    d = dict(N=100000, T=12, F=F, C=256, R=R, O=1, H1=128)
    d.update(over)
    return _lib.Dims(d["N"], d["T"], d["F"], d["C"], d["R"], d["O"], d["H1"], 1, 0.01, arith, flags)


def _graph(merged=True, region_sorted=1, overlap=0):
    g = _lib.Graph()
    g.rowptr = g.col = g.val = g.node_region = g.chunk_tab = g.chunk_region = DUMMY
    g.n_chunks = 64
    if merged:
        g.m_rowptr = g.m_col = g.m_val_a = g.m_val_l = DUMMY
    g.overlap, g.region_sorted = overlap, region_sorted
    return g


def _fwd_bytes(lib, d, g):
    return lib.regt_forward_only_workspace_bytes(C.byref(d), C.byref(g))


def test_symbol_and_constant_are_bound():
    lib = _lib.load()
    assert _lib.DIMS_FORWARD_ONLY == 8
    assert "regt_forward_only_workspace_bytes" in _lib.SIGNATURES
    assert lib.regt_forward_only_workspace_bytes.restype is C.c_size_t
    assert lib.regt_abi_version() == 8


def test_fp32_layout_keeps_at_most_four_of_the_nine_row_arrays():
    lib = _lib.load()
    d, g = _dims(_lib.ARITH_FP32, 32, 8), _graph()
    M, Cd = d.N * d.T, d.C
    train = lib.regt_workspace_bytes(C.byref(d), g.n_chunks, 0)
    fwd = _fwd_bytes(lib, d, g)
    assert 0 < fwd <= train - 5 * M * Cd * 4, (fwd, train)
    # the flag itself does not change the size, and the training size is what it was
    assert _fwd_bytes(lib, _dims(_lib.ARITH_FP32, 32, 8, _lib.DIMS_FORWARD_ONLY), g) == fwd


def test_bf16_fused_layout_holds_no_row_array_of_width_C():
    lib = _lib.load()
    d, g = _dims(_lib.ARITH_BF16, 64, 64), _graph()
    M = d.N * d.T
    # fixed part at R = 64, C = 256, F = 64: S (256 KB) + composed weights A0, A_r, Gzr, Gh (4.3 MB) + their fragment-order bf16
    # copies (2.9 MB) + biases: under 8 MB; K = 16 MiB as the bound
    K = 16 << 20
    fwd = _fwd_bytes(lib, d, g)
    assert 0 < fwd <= 3 * M * d.F * 2 + d.N * (d.H1 + d.C) * 4 + K, fwd
    assert fwd < M * d.C * 2 + 3 * M * d.F * 2          # not even one bf16 M x C array fits next to the three row arrays


@pytest.mark.parametrize("how", ["no_merged_operator", "unsorted_regions_without_bf16_rows", "flag_no_bf16_rows"])
def test_bf16_without_the_fused_form_needs_h(how):
    lib = _lib.load()
    fused = _fwd_bytes(lib, _dims(_lib.ARITH_BF16, 64, 64), _graph())
    if how == "no_merged_operator":
        d, g = _dims(_lib.ARITH_BF16, 64, 64), _graph(merged=False)
    elif how == "unsorted_regions_without_bf16_rows":
        d, g = _dims(_lib.ARITH_BF16, 64, 64), _graph(merged=False, region_sorted=0)
    else:
        d, g = _dims(_lib.ARITH_BF16, 64, 64, _lib.DIMS_NO_BF16_ROWS), _graph()
    M = d.N * d.T
    assert _fwd_bytes(lib, d, g) >= fused + M * d.C * 2


def test_unsorted_regions_keep_the_fused_form():
    # region_sorted = 0 with the merged operator runs the 64-row fused kernel: still no M x C array
    lib = _lib.load()
    d = _dims(_lib.ARITH_BF16, 64, 64)
    assert _fwd_bytes(lib, d, _graph(region_sorted=0)) == _fwd_bytes(lib, d, _graph())


def test_host_side_refusals():
    lib = _lib.load()
    d, g = _dims(_lib.ARITH_FP32, 32, 8), _graph()
    assert lib.regt_forward_only_workspace_bytes(None, C.byref(g)) == 0
    assert b"dims" in lib.regt_last_error()
    assert lib.regt_forward_only_workspace_bytes(C.byref(d), None) == 0
    assert b"graph" in lib.regt_last_error()
    assert _fwd_bytes(lib, _dims(_lib.ARITH_FP32, 7, 8), g) == 0
    assert b"F=7" in lib.regt_last_error()


def test_packed_sizing_follows_x_rows_and_the_row_type():
    """regt_forward_only_packed_workspace_bytes decides with the call's own x_rows and row type, as the packed forwards do."""
    lib = _lib.load()
    assert lib.regt_forward_only_packed_workspace_bytes.restype is C.c_size_t
    d, g = _dims(_lib.ARITH_BF16, 64, 64, N=10000), _graph()
    packed = lambda x_rows, bf16, dd=d: lib.regt_forward_only_packed_workspace_bytes(C.byref(dd), C.byref(g), x_rows, bf16)
    N, M, row = d.N, d.N * d.T, d.T * d.F * 2           # (row: 1536 bytes, a multiple of the layout's 256-byte rounding)
    base = _fwd_bytes(lib, d, g)
    assert packed(N, 0) == base and packed(N, 1) == base
    # fp32 rows: the fused form keeps a bf16 copy of every row, up to x_rows = 2 N; beyond that the three-launch form with h, [Z|R], q
    assert packed(N + 4000, 0) == base + 4000 * row
    assert packed(2 * N, 0) == base + N * row
    assert packed(2 * N + 1, 0) >= base + 4 * M * d.C * 2
    # bf16 rows are read in place, whatever their number
    assert packed(3 * N, 1) == base
    # refusals: fewer rows than nodes; bf16 rows where the fused form does not apply
    assert packed(N - 1, 0) == 0 and b"x_rows" in lib.regt_last_error()
    d32 = _dims(_lib.ARITH_FP32, 64, 64, N=10000)
    assert packed(N, 1, d32) == 0 and b"bf16" in lib.regt_last_error()
    assert packed(3 * N, 0, d32) == _fwd_bytes(lib, d32, g)          # fp32 arithmetic reads the caller's rows in place
    assert lib.regt_forward_only_packed_workspace_bytes(None, C.byref(g), N, 0) == 0
    assert lib.regt_forward_only_packed_workspace_bytes(C.byref(d), None, N, 0) == 0 and b"graph" in lib.regt_last_error()
