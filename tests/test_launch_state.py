"""The native library's launch state is keyed by device (kernels.h want_dynamic_lds / device_cus, the per-device graph stream of
api_runtime.hip).  Without a GPU: the workspace sizes, which go through the one chunk calculator of wgrad_dispatch.hip, are pinned to
recorded numbers.  With two GPUs: one process drives both and gets the same bits from each."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from regtgcn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# regt_workspace_bytes of (N, T, F, C, R) with O = 1, H1 = 128, default arithmetic, for (n_chunks, overlap) in the order
# (0, 0), (0, 1), (1, 0), (1, 1), (40, 0), (40, 1).  Recorded from the library as it was before the chunk rule became one function,
# at 256 CUs: what an MI355X has, and what device_cus() answers where there is no device.
WORKSPACE_BYTES = {
    (104, 6, 8, 256, 5): [26088960, 26168832, 26088960, 26168832, 26735104, 26814976],                          # TPIMS
    (3000, 12, 32, 256, 4): [610608640, 624432640, 610608640, 624432640, 611926528, 625750528],
    (100000, 12, 32, 256, 8): [12095433216, 13170633216, 12095433216, 13170633216, 12096751104, 13171951104],   # cfg-3
    # C = 128 over M = 480 000 rows: the shape wgrad_chunk_bound was introduced for (fp32 asks for 768 chunks of dUh)
    (40000, 12, 32, 128, 4): [2688245248, 2872565248, 2688245248, 2872565248, 2688904192, 2873224192],
}


@pytest.mark.parametrize("shape", list(WORKSPACE_BYTES), ids=lambda s: "N%d_T%d_F%d_C%d_R%d" % s)
def test_workspace_bytes_are_what_they_were(shape):
    lib = _lib.load()
    n, t, f, c, r = shape
    d = _lib.Dims(n, t, f, c, r, 1, 128, 1, 0.01, 0, 0)
    got = [lib.regt_workspace_bytes(C.byref(d), n_chunks, overlap) for n_chunks in (0, 1, 40) for overlap in (0, 1)]
    assert got == WORKSPACE_BYTES[shape]


# The sizers the table above does not cover, recorded the same way from the library as it was while its host layer was one file.
# regt_forward_only_workspace_bytes of the same shapes, regional, 40 region chunks and a merged operator (so that the fused form
# can be asked for), for arith = default, bf16: (3000, 12, 32, 256, 4) and cfg-3 take the fused form under bf16.
FORWARD_ONLY_BYTES = {
    (104, 6, 8, 256, 5): [3867904, 3867904],
    (3000, 12, 32, 256, 4): [164395776, 9894656],
    (100000, 12, 32, 256, 8): [5428976384, 283243264],
    (40000, 12, 32, 128, 4): [1188368128, 1188368128],
}
# regt_forward_only_packed_workspace_bytes at (3000, 12, 32, 256, 4): (x_rows, x_is_bf16, arith) -> bytes.  bf16 rows under fp32
# arithmetic are refused; fp32 rows under bf16 are converted into the workspace, all x_rows of them.
PACKED_SHAPE = (3000, 12, 32, 256, 4)
PACKED_REFUSED = b"regt_forward_only_packed_workspace_bytes: bf16 input rows need bf16 arithmetic and a shape the fused forward covers"
FORWARD_ONLY_PACKED_BYTES = {
    (3000, 0, _lib.ARITH_DEFAULT): 164395776, (3000, 0, _lib.ARITH_BF16): 9894656,
    (3000, 1, _lib.ARITH_DEFAULT): 0, (3000, 1, _lib.ARITH_BF16): 9894656,
    (4500, 0, _lib.ARITH_DEFAULT): 164395776, (4500, 0, _lib.ARITH_BF16): 11046656,
    (4500, 1, _lib.ARITH_DEFAULT): 0, (4500, 1, _lib.ARITH_BF16): 9894656,
}
# regt_cell0_workspace_bytes of (N, T, C) with O = 1, H1 = 128 for (kz, kh) = (8, 8), (32, 64)
CELL0_BYTES = {(104, 6, 256): [2997504, 3407104], (3000, 12, 128): [82595328, 94146048]}


def _merged_graph():
    """A regt_graph whose every pointer is set: the sizers decide from NULL / non-NULL and n_chunks alone and read nothing."""
    buf = (C.c_int32 * 4)()
    g = _lib.Graph()
    for name in ("rowptr", "col", "val", "node_region", "chunk_tab", "chunk_region", "m_rowptr", "m_col", "m_val_a", "m_val_l"):
        setattr(g, name, C.addressof(buf))
    g.n_chunks = 40
    return g, buf


@pytest.mark.parametrize("shape", list(FORWARD_ONLY_BYTES), ids=lambda s: "N%d_T%d_F%d_C%d_R%d" % s)
def test_forward_only_workspace_bytes_are_what_they_were(shape):
    lib = _lib.load()
    g, _keep = _merged_graph()
    got = []
    for arith in (_lib.ARITH_DEFAULT, _lib.ARITH_BF16):
        d = _lib.Dims(*shape, 1, 128, 1, 0.01, arith, 0)
        got.append(lib.regt_forward_only_workspace_bytes(C.byref(d), C.byref(g)))
    assert got == FORWARD_ONLY_BYTES[shape]


@pytest.mark.parametrize("case", list(FORWARD_ONLY_PACKED_BYTES), ids=lambda c: "rows%d_bf16rows%d_arith%d" % c)
def test_forward_only_packed_workspace_bytes_are_what_they_were(case):
    lib = _lib.load()
    g, _keep = _merged_graph()
    x_rows, x_is_bf16, arith = case
    d = _lib.Dims(*PACKED_SHAPE, 1, 128, 1, 0.01, arith, 0)
    got = lib.regt_forward_only_packed_workspace_bytes(C.byref(d), C.byref(g), x_rows, x_is_bf16)
    assert got == FORWARD_ONLY_PACKED_BYTES[case]
    if got == 0:
        assert lib.regt_last_error() == PACKED_REFUSED


@pytest.mark.parametrize("shape", list(CELL0_BYTES), ids=lambda s: "N%d_T%d_C%d" % s)
def test_cell0_workspace_bytes_are_what_they_were(shape):
    lib = _lib.load()
    n, t, c = shape
    d = _lib.Dims(n, t, 32, c, 1, 1, 128, 0, 0.01, 0, 0)
    assert [lib.regt_cell0_workspace_bytes(C.byref(d), kz, kh) for kz, kh in ((8, 8), (32, 64))] == CELL0_BYTES[shape]


def _snapshot(dev, arith, calls, n):
    """`calls` forward + backward passes of one RegT-GCN on cuda:`dev` (every library call raises unless it returns REGT_OK);
    the last pass's pred, hidden and parameter gradients on the host."""
    import regtgcn_amd as R
    from oracle import model as M
    from test_gpu_model import _synthetic
    f, t, regions, o = 32, 12, 4, 1
    ei, ri, rw, x = _synthetic(n, 8 * n, regions, f, t, seed=21)
    y = torch.rand(n, o, generator=torch.Generator().manual_seed(5))
    p = M.init_params("RegionalTemporalGCN", f, t, o, num_nodes=n, num_regions=regions, seed=8)
    device = torch.device("cuda", dev)
    with torch.cuda.device(dev):
        mod = R.RegionalTemporalGCN(node_features=f, num_nodes=n, periods=t, output_dim=o, num_regions=regions)
        mod.load_state_dict(p, strict=True)
        mod.arithmetic = arith
        mod = mod.to(device)
        graph = mod.prepare_graph(ei.to(device), [i.to(device) for i in ri], [a.to(device) for a in rw])
        assert graph.region_sorted
        xs, ys = x.to(device), y.to(device)
        for _ in range(calls):
            mod.zero_grad(set_to_none=True)
            pred, hidden = mod.forward_prepared(xs, graph)
            R.functional.mse_loss(pred, ys).backward()
            out = [pred.detach().cpu(), hidden.detach().cpu()] + [q.grad.cpu() for q in mod.parameters() if q.grad is not None]
            del pred, hidden        # (the next call gets the same buffers: a captured launch sequence is keyed by them)
        torch.cuda.synchronize()
    return out


def _both_devices(arith, calls=1, n=300):
    try:
        first = _snapshot(0, arith, calls, n)
        replayed = _graph_stats()
        second = _snapshot(1, arith, calls, n)
    finally:
        torch.cuda.set_device(0)
    assert len(first) == len(second) > 10
    for k, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), (arith, k)
    return replayed, _graph_stats()


def _graph_stats():
    st = (C.c_int64 * 6)()
    _lib.load().regt_graph_stats(st)
    return st[2], st[5]      # forward, backward launch sequences replayed from a captured graph


def _need_two_gpus():
    if torch.cuda.device_count() < 2:
        print("skipped: one process driving two devices needs two GPUs, this machine has %d" % torch.cuda.device_count())
        pytest.skip("needs two GPUs")


# N = 300 leaves the fp32 regional embedding to the general GEMM core (embed_fp32_ok: 65 536 rows); N = 6000 launches
# embed_fp32_kernel and its 141 KB of dynamic LDS.  bf16: the row-owning fused forward (148 KB) and the fused backward at either size.
@pytest.mark.gpu
@pytest.mark.parametrize("arith,n", [("fp32", 300), ("fp32", 6000), ("bf16", 300)])
def test_one_process_two_devices_same_bits(arith, n):
    """T = 12 <= 64 periods: the library's results are bit-reproducible, and both devices are the same hardware."""
    _need_two_gpus()
    _both_devices(arith, n=n)


@pytest.mark.gpu
def test_one_process_two_devices_same_bits_with_graph_replay():
    """REGT_HIPGRAPH=2 is read from the environment at first use, hence a process of its own.  Three calls per device: plain launches,
    capture + replay, replay -- on the second device too (its launch sequences are captured on a stream of its own)."""
    _need_two_gpus()
    script = ("import sys; sys.path[:0] = [%r, %r]\n"
              "import test_launch_state as t\n"
              "after0, after1 = t._both_devices('fp32', calls=3)\n"
              "assert after0[0] >= 1 and after0[1] >= 1, after0\n"
              "assert after1[0] > after0[0] and after1[1] > after0[1], (after0, after1)\n"
              "print('OK', after0, after1)\n") % (ROOT, os.path.join(ROOT, "tests"))
    res = subprocess.run([sys.executable, "-c", script], cwd=ROOT, env=dict(os.environ, REGT_HIPGRAPH="2"), capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
