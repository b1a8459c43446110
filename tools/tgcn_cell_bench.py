#!/usr/bin/env python3
"""One TGCN cell step at N = 100 000, F = 32, C = 256 (fp32, synthetic graph with 1M edges):
    python tools/tgcn_cell_bench.py [--iters 20] > profiles/tgcn_cell.txt
  forward      regt_tgcn_forward (training layout)
  backward+dx  regt_tgcn_backward with dx and dh_in
  backward     regt_tgcn_backward with dh_in alone (no cell_dx launch, no transposed aggregation)
  cell_dx      the dAx kernel alone (the library's per-stage device time) against the bytes it must move, 3 N C 4 read + N F 4 written
  composed     what the parent commit can write for dAx: three regt_linear launches dp_k @ G_k and two adds
Times are HIP events around `iters` calls after a warm-up; the roofline is the 8 TB/s HBM peak of the MI355X."""
import argparse, ctypes, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES, EDGES, F, C = 100_000, 1_000_000, 32, 256
HBM_ROOF = 8.0e12


def timed(fn, iters: int):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def stages(lib, fn, iters: int = 5):
    import torch
    from regtgcn_amd import _lib
    lib.regt_profile_enable(1)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    lib.regt_profile_enable(0)
    buf = (ctypes.c_char * 16384)()
    _lib.check(lib.regt_profile_collect(buf, 16384), "regt_profile_collect")
    return {ln.split()[0]: float(ln.split()[2]) / iters for ln in buf.value.decode().splitlines()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    iters = ap.parse_args().iters
    import torch
    sys.path.insert(0, ROOT)
    import regtgcn_amd as R
    from regtgcn_amd import _lib, ops
    from regtgcn_amd import functional as Fn
    if not torch.cuda.is_available():
        print("no GPU: nothing measured")
        return
    lib = R.load_library()
    lib.regt_set_gemm_mode(0)
    torch.manual_seed(42)
    dev = torch.device("cuda")
    ei = torch.randint(0, NODES, (2, EDGES), device=dev)
    op = R.graph.prepare_gcn_operator(ei, torch.rand(EDGES, device=dev) + 0.5, NODES)
    cell = R.nn.TGCN(F, C).to(dev)
    tens = [t.detach() for t in cell._cell_params()]
    x, h, gh = torch.rand(NODES, F, device=dev), 0.5 * torch.randn(NODES, C, device=dev), torch.randn(NODES, C, device=dev)
    out, st = Fn._tgcn_forward_call(x, h, op, tens, False)
    grads = {k: torch.empty_like(t) for k, t in zip(Fn.PARAM_NAMES_TGCN, tens)}
    gr = Fn._fill(_lib.Grads(), grads, False)
    dx, dh = torch.empty(NODES, F, device=dev), torch.empty(NODES, C, device=dev)
    fwd = lambda: ops.tgcn_forward(st.dims, st.gs, st.ps, x, h, out, st.handle.ws)                               # noqa: E731
    bwd_dx = lambda: ops.tgcn_backward(st.dims, st.gs, st.ps, gr, gh, h, out, op, dx, dh, st.handle.ws)          # noqa: E731
    bwd = lambda: ops.tgcn_backward(st.dims, st.gs, st.ps, gr, gh, h, out, op, None, dh, st.handle.ws)           # noqa: E731
    # the composition of the parent commit: dp_k (N, C) @ G_k (C, F) as regt_linear (weight (F, C) = G_k^T), then two adds
    dp = [torch.randn(NODES, C, device=dev) for _ in range(3)]
    gt = [torch.randn(F, C, device=dev) for _ in range(3)]
    composed = lambda: ops.linear(dp[0], gt[0]) + ops.linear(dp[1], gt[1]) + ops.linear(dp[2], gt[2])             # noqa: E731
    t_f, t_bx, t_b, t_c = timed(fwd, iters), timed(bwd_dx, iters), timed(bwd, iters), timed(composed, iters)
    s = stages(lib, bwd_dx)
    nbytes = 3 * NODES * C * 4 + NODES * F * 4
    k = s["cell_dx"]
    print(f"TGCN cell step, N = {NODES}, F = {F}, C = {C}, E = {EDGES}, fp32, {torch.cuda.get_device_name(0)}, {iters} iterations")
    print(f"forward                 {t_f:8.3f} ms")
    print(f"backward with dx        {t_bx:8.3f} ms")
    print(f"backward without dx     {t_b:8.3f} ms")
    print(f"cell_dx kernel          {k * 1e3:8.1f} us   {nbytes / 1e6:.1f} MB -> {nbytes / (k * 1e-3) / 1e12:.2f} TB/s = "
          f"{100 * nbytes / (k * 1e-3) / HBM_ROOF:.0f} % of the {HBM_ROOF / 1e12:.0f} TB/s HBM roofline")
    print(f"spmm_dx (A_hat^T dAx)   {s['spmm_dx'] * 1e3:8.1f} us")
    print(f"composed dAx (3 regt_linear + 2 adds)  {t_c * 1e3:8.1f} us   cell_dx / composed = {k / t_c:.2f}")
    print("stages of the backward with dx (ms): " + ", ".join(f"{n} {v:.3f}" for n, v in sorted(s.items(), key=lambda kv: -kv[1])))


if __name__ == "__main__":
    main()
