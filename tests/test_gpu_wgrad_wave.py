"""The wave-owned fp32 weight-gradient kernel (csrc/wgrad_fp32.hip wgrad_wave_kernel: one workgroup per CU, a 128 x 128 block per
wave) against the three-workgroup kernel it replaces at large M (wgrad3_kernel), on the SAME explicit row chunks: the slabs and the
column sums must agree bit for bit -- both accumulate k ascending with the same pairing of k to MFMA lanes and sum the columns in
the same fixed order.  The choice holds the new kernel to M >= 256 CUs x 4096 rows, far above anything a test should run, so the
launches go through regt_wgrad_slabs with any_rows = 1 (the launcher below that one gate; every other condition of the choice is
live), once with regt_set_option("wgrad_wave", 1) and once with 0, and the entry point reports which kernel ran.

Shapes: the smallest that reach each path of the K loop -- 3 chunks of 2 slabs (both LDS stages, the look-ahead past the chunk's
end), a ragged last chunk whose rows are no multiple of the 32-row slab, a single chunk shorter than one slab, Nout = 256 (one
output tile) and 512 (two tiles per chunk), ten chunks of two tiles (the XCD-aware block order of wgrad_block: eight chunks dealt
round-robin, two in plain order).  One fp64 product per shape keeps "both wrong alike" out:
the chunk sums are held to M x 2^-23 x |P|^T |Q| (every partial sum of the fp32 accumulation is bounded by |P|^T |Q|, each of the at
most M additions and products rounds once to 2^-24 relative)."""
import ctypes

import pytest
import torch

import regtgcn_amd as R
from regtgcn_amd import _lib

pytestmark = pytest.mark.gpu


def _slabs(P, Q, M, nout, kchunk, nchunks, colsum, wave, poison=False):
    """P, Q: 2-D views (M rows) of device buffers; returns (slab tensor (nchunks, stride), name of the kernel that ran)."""
    lib = R.load_library()
    stride = nout * 256 + (nout if colsum else 0)
    slab = torch.full((nchunks, stride), float("nan") if poison else 0.0, dtype=torch.float32, device=P.device)
    ran = ctypes.c_char_p()
    prev = lib.regt_set_option(b"wgrad_wave", wave)
    try:
        rc = lib.regt_wgrad_slabs(P.data_ptr(), P.stride(0), nout, Q.data_ptr(), Q.stride(0), 256, M, kchunk, nchunks, 1 if colsum else 0,
                                  slab.data_ptr(), 1, ctypes.byref(ran), torch.cuda.current_stream().cuda_stream)
    finally:
        lib.regt_set_option(b"wgrad_wave", prev)
    _lib.check(rc, "regt_wgrad_slabs")
    torch.cuda.synchronize()
    return slab, ran.value.decode()


def _operands(M, nout, window):
    """window: P and Q start 16 / 32 bytes into rows that are wider than the operands (P is read out of the 2C-wide dzr in the step)."""
    g = torch.Generator(device="cpu").manual_seed(1000 * nout + M)
    ldp, offp, ldq, offq = (2 * nout + 8, 4, 256 + 12, 8) if window else (nout, 0, 256, 0)
    bp = torch.randn(M, ldp, generator=g).cuda()
    bq = torch.randn(M, ldq, generator=g).cuda()
    return bp[:, offp:offp + nout], bq[:, offq:offq + 256]


# (name, Nout, M, kchunk, nchunks, colsum, window, poison)
CASES = [
    ("three_chunks_of_two_slabs", 256, 192, 64, 3, True, False, False),
    ("ragged_last_chunk_two_tiles", 512, 2 * 96 + 53, 96, 3, True, False, True),
    ("one_chunk_shorter_than_a_slab", 256, 19, 64, 1, False, False, False),
    ("poisoned_slabs", 256, 192, 64, 3, True, False, True),
    ("offset_and_wide_rows", 512, 5 * 64 + 40, 64, 6, True, True, True),
    ("ten_chunks_of_two_tiles", 512, 9 * 64 + 44, 64, 10, True, False, True),
]


@pytest.mark.parametrize("name,nout,M,kchunk,nchunks,colsum,window,poison", CASES, ids=[c[0] for c in CASES])
def test_wave_kernel_matches_wgrad3_bit_for_bit(name, nout, M, kchunk, nchunks, colsum, window, poison):
    P, Q = _operands(M, nout, window)
    new, k_new = _slabs(P, Q, M, nout, kchunk, nchunks, colsum, 1, poison)
    old, k_old = _slabs(P, Q, M, nout, kchunk, nchunks, colsum, 0, poison)
    assert k_new == "wgrad_wave_kernel" and k_old == "wgrad3_kernel", (k_new, k_old)
    assert not torch.isnan(new).any(), "a slab element was not written"
    assert not torch.isnan(old).any()
    diff = (new.view(torch.int32) != old.view(torch.int32))
    assert not diff.any(), (name, int(diff.sum()), float((new - old).abs().max()))
    # the chunk sums against one fp64 product
    Pd, Qd = P.double(), Q.double()
    got = new[:, :nout * 256].double().sum(0).view(nout, 256)
    bar = M * 2.0 ** -23 * (Pd.abs().t() @ Qd.abs())
    assert bool(((got - Pd.t() @ Qd).abs() <= bar).all())
    if colsum:
        cs = new[:, nout * 256:].double().sum(0)
        assert bool(((cs - Pd.sum(0)).abs() <= M * 2.0 ** -23 * Pd.abs().sum(0)).all())


def test_option_off_or_other_shapes_keep_the_old_kernel():
    """Below the row gate (any_rows = 1) the other conditions of the choice still hold: Nin = 128 runs wgrad3_kernel."""
    lib = R.load_library()
    P = torch.randn(192, 256, device="cuda")
    Q = torch.randn(192, 128, device="cuda")
    slab = torch.empty(3, 256 * 128, device="cuda")
    ran = ctypes.c_char_p()
    _lib.check(lib.regt_wgrad_slabs(P.data_ptr(), 256, 256, Q.data_ptr(), 128, 128, 192, 64, 3, 0, slab.data_ptr(), 1, ctypes.byref(ran),
                                    torch.cuda.current_stream().cuda_stream), "regt_wgrad_slabs")
    torch.cuda.synchronize()
    assert ran.value.decode() == "wgrad3_kernel"
    assert torch.allclose(slab.sum(0).view(256, 128), P.t() @ Q, rtol=0, atol=1e-3)
