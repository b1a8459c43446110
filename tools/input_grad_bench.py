#!/usr/bin/env python3
"""The whole-model input gradient at the cfg-3 shape (N = 100 000, T = 12, F = 32, C = 256, fp32; synthetic graph, 1M edges, 5 regions
sorted by node):
    python tools/input_grad_bench.py [--iters 20] > profiles/input_grad.txt
  step          regt_forward + regt_backward (no dx)
  dx            regt_input_gradient behind it: model_dx_kernel + spmm_dual_t_kernel, whole call and per stage (the library's device times)
  composed      what the parent commit allows for the same result: regt_linear for the four products (dzr Gzr, dhp Gh, ds A0, ds A_r -- ONE
                region block for all rows, which flatters it), two adds, regt_spmm_csr over the two transposed operators, two adds, the
                (N, T, F) -> (N, F, T) permute
  model_dx      against the bytes it must move, (4 M C + 3 M F) 4; spmm_dual_t against 4 N T F 4 + 12 nnz
Times are HIP events around `iters` calls after a warm-up; the roofline is the 8 TB/s HBM peak of the MI355X.
--shuffled: the same with region ids drawn at random per node (the per-region passes of model_dx_kernel in every tile).
--bars: the worst dx row ratio of every case of tests/input_grad_math.py on the device instead (appended to the same profile)."""
import argparse, ctypes, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES, EDGES, T, F, C, REGIONS = 100_000, 1_000_000, 12, 32, 256, 5
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
    rows = [ln.split() for ln in buf.value.decode().splitlines()]
    return {r[0]: float(r[2]) / iters for r in rows if len(r) >= 3}


def bars():
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import input_grad_math as IG
    import regtgcn_amd as R
    print(f"worst dx row ratio per case against float64 autograd of the oracle (bar {IG.bar():.3e}; fp32 restatement alongside), "
          f"{torch.cuda.get_device_name(0)}")
    fp32 = IG.measured_fp32()
    for name in IG.CASES:
        got = IG.run_hip(R, name)
        print(f"  {name:46s} HIP {IG.worst_row_ratio(got['dx'], IG.reference(name)['dx']):.3e}   fp32 restatement {fp32[name]:.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--bars", action="store_true")
    ap.add_argument("--shuffled", action="store_true", help="region ids drawn at random per node: every 128-row tile holds all R regions")
    args = ap.parse_args()
    iters = args.iters
    import torch
    sys.path.insert(0, ROOT)
    import regtgcn_amd as R
    from regtgcn_amd import _lib, ops
    from regtgcn_amd import functional as Fn
    if not torch.cuda.is_available():
        print("no GPU: nothing measured")
        return
    if args.bars:
        return bars()
    lib = R.load_library()
    lib.regt_set_gemm_mode(0)
    torch.manual_seed(42)
    dev = torch.device("cuda")
    ei = torch.randint(0, NODES, (2, EDGES), device=dev)
    part = torch.randint(0, REGIONS, (NODES,), device=dev) if args.shuffled else torch.arange(NODES, device=dev) * REGIONS // NODES
    same = part[ei[0]] == part[ei[1]]
    ri = [ei[:, same & (part[ei[1]] == k)].contiguous() for k in range(REGIONS)]
    rw = [torch.rand(r.shape[1], device=dev) + 0.5 for r in ri]
    graph = R.prepare_graph(ei, None, ri, rw, NODES)
    mod = R.RegionalTemporalGCN(node_features=F, num_nodes=NODES, periods=T, output_dim=1, num_regions=REGIONS, hidden_channels=C).to(dev)
    params = [p.detach() for p in mod._params_in_order()]
    x = torch.rand(NODES, F, T, device=dev)
    pred, hidden, st = Fn._regt_forward_call(x, graph, True, 0.01, (False, _lib.ARITH_FP32, 0), params, False)
    grads = {k: torch.empty_like(p) for k, p in zip(st.names, params)}
    gr = Fn._fill(_lib.Grads(), grads, True)
    dpred = torch.randn(NODES, 1, device=dev)
    st_ = Fn._stream()

    def step():
        _lib.check(lib.regt_forward(ctypes.byref(st.dims), ctypes.byref(st.gs), ctypes.byref(st.ps), _lib.ptr(x), _lib.ptr(pred), _lib.ptr(hidden),
                                    _lib.ptr(st.handle.ws), st.wsb, st_), "regt_forward")
        _lib.check(lib.regt_backward(ctypes.byref(st.dims), ctypes.byref(st.gs), ctypes.byref(st.ps), ctypes.byref(gr), _lib.ptr(dpred), None,
                                     _lib.ptr(hidden), None, _lib.ptr(st.handle.ws), st.wsb, st_), "regt_backward")

    t_op = graph.transposed_merged
    dx = torch.empty(NODES, F, T, device=dev)
    scratch = torch.empty(lib.regt_input_gradient_scratch_bytes(ctypes.byref(st.dims)), dtype=torch.uint8, device=dev)
    grad = lambda: ops.input_gradient(st.dims, st.gs, st.ps, t_op, dx, st.handle.ws, scratch)      # noqa: E731
    t_step = timed(step, max(3, iters // 4))
    t_dx = timed(grad, iters)
    s = stages(lib, grad)
    # the composition the parent commit allows
    m = NODES * T
    dzr, dhp, ds = torch.randn(m, 2 * C, device=dev), torch.randn(m, C, device=dev), torch.randn(m, C, device=dev)
    gzr, gh, a0, ar = (torch.randn(F, k, device=dev) for k in (2 * C, C, C, C))
    ta = R.graph.transpose_csr(graph.m_rowptr, graph.m_col, graph.m_val_a, NODES, NODES)
    tl = R.graph.transpose_csr(graph.m_rowptr, graph.m_col, graph.m_val_l, NODES, NODES)

    def composed():
        d_ax = ops.linear(dzr, gzr) + ops.linear(dhp, gh)
        d_xd, d_lx = ops.linear(ds, a0), ops.linear(ds, ar)
        out = d_xd.view(NODES, T * F) + ops.spmm_csr(ta[0], ta[1], ta[2], d_ax.view(NODES, T * F)) + ops.spmm_csr(tl[0], tl[1], tl[2], d_lx.view(NODES, T * F))
        return out.view(NODES, T, F).permute(0, 2, 1).contiguous()

    t_c = timed(composed, iters)
    nnz = int(t_op[1].numel())
    order = "shuffled" if args.shuffled else "sorted"
    b_gemm = (4 * m * C + 3 * m * F) * 4
    b_agg = 4 * NODES * T * F * 4 + 12 * nnz
    kg, ka = s["model_dx"], s["spmm_dx"]
    print(f"whole-model input gradient, N = {NODES}, T = {T}, F = {F}, C = {C}, R = {REGIONS} ({order} region ids), E = {EDGES}, merged nnz = {nnz}, fp32, "
          f"{torch.cuda.get_device_name(0)}, {iters} iterations")
    print(f"forward + backward (no dx)      {t_step:8.3f} ms")
    print(f"regt_input_gradient             {t_dx:8.3f} ms   = {100 * t_dx / t_step:.1f} % of the step")
    print(f"model_dx kernel                 {kg * 1e3:8.1f} us   {b_gemm / 1e6:.1f} MB -> {b_gemm / (kg * 1e-3) / 1e12:.2f} TB/s = "
          f"{100 * b_gemm / (kg * 1e-3) / HBM_ROOF:.0f} % of the {HBM_ROOF / 1e12:.0f} TB/s HBM roofline")
    print(f"spmm_dual_t kernel (+ unpack)   {ka * 1e3:8.1f} us   {b_agg / 1e6:.1f} MB -> {b_agg / (ka * 1e-3) / 1e12:.2f} TB/s = "
          f"{100 * b_agg / (ka * 1e-3) / HBM_ROOF:.0f} % of the roofline")
    print(f"composed (4 regt_linear, 2 regt_spmm_csr, 4 adds, permute)  {t_c:8.3f} ms   regt_input_gradient / composed = {t_dx / t_c:.2f}")


if __name__ == "__main__":
    main()
