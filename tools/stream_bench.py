#!/usr/bin/env python3
"""Streaming inference against one forward per window at cfg-3 size (synthetic, as bench.py builds it: 100k nodes, 1M edges, 8 regions,
F = 32, T = 12, fp32):
    python tools/stream_bench.py [--repeats 2] [--iters 20] > profiles/stream_inference.txt
  (a) window : the parent's way, one forward-only forward_prepared call per window at T = 12
  (b) serve  : StreamingPredictor.push per time step, split into the T = 1 forward (period_outputs) and regt_window_forward
  (c) eval64 : 64 consecutive windows through serve.window_outputs (75 time steps, 8 per period_outputs call), per window
The legs run in child processes of their own, in alternation, `repeats` times each; times are HIP events around `iters` calls after a
warm-up.  A second, untimed pass collects the library's per-stage device times: window_sum (softmax + the window kernel) gives the
kernel's achieved bytes/s for windows = 1 and for the chunked form, from the bytes the algorithm needs."""
import ctypes, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES, EDGES, REGIONS, F, T, O, C = 100_000, 1_000_000, 8, 32, 12, 1, 256
EVAL_WINDOWS, STEP_BATCH = 64, 8
HBM_ROOF = 8.0e12


def window_bytes(windows: int, wc: int):
    """(bytes read, bytes written) the window kernel needs: per chunk of nw <= wc windows nw + T - 1 slab reads and nw slab writes."""
    slab = NODES * C * 4
    reads = sum(min(wc, windows - w0) + T - 1 for w0 in range(0, windows, wc))
    return reads * slab, windows * slab


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


def child(leg: str, iters: int):
    import torch
    sys.path.insert(0, ROOT)
    import regtgcn_amd as R
    lib = R.load_library()
    lib.regt_set_gemm_mode(0)
    dev = torch.device("cuda")
    torch.manual_seed(42)
    g = R.data.synthetic_regional_graph(NODES, EDGES, REGIONS, seed=42)
    model = R.RegionalTemporalGCN(F, NODES, T, O, num_regions=REGIONS).to(dev).eval()
    ei, ri, ra = g.edge_index.to(dev), [t.to(dev) for t in g.region_index], [t.to(dev) for t in g.region_attr]
    build = lambda b: model.prepare_graph(ei, ri, ra, copies=b)      # noqa: E731
    head = (model.tgnn._attention, model.linear1.weight, model.linear1.bias, model.linear2.weight, model.linear2.bias)
    wc = lib.regt_window_chunk(EVAL_WINDOWS)      # windows per thread of the chunked kernel
    if leg == "window":
        graph, x = build(1), torch.rand(NODES, F, T, device=dev)
        with torch.no_grad():
            ms = timed(lambda: model.forward_prepared(x, graph), iters)
        print(f"(a) window  {ms:8.3f} ms per window   (one forward-only forward at T = {T})", flush=True)
    elif leg == "serve":
        graph, x = build(1), torch.rand(NODES, F, device=dev)
        sp = R.StreamingPredictor(model, graph)
        for _ in range(T):
            sp.push(x)
        ring = sp._ring
        ms = timed(lambda: sp.push(x), iters)
        ms_s = timed(lambda: model.period_outputs(x.unsqueeze(0), graph), iters)
        ms_w = timed(lambda: R.ops.window_forward(ring, 3, 1, *head), iters)
        st = stages(lib, lambda: R.ops.window_forward(ring, 3, 1, *head))
        rd, wr = window_bytes(1, 1)
        k = st["window_sum"]
        print(f"(b) serve   {ms:8.3f} ms per step     = T = 1 forward {ms_s:.3f} + regt_window_forward {ms_w:.3f}; "
              f"window_sum {k:.3f} ms head_fwd {st['head_fwd']:.3f} ms; window kernel, windows = 1: {rd / 1e9:.2f} GB read + {wr / 1e9:.2f} GB "
              f"written in {k:.3f} ms = {(rd + wr) / k / 1e9:.2f} TB/s = {100 * (rd + wr) / (k * 1e-3) / HBM_ROOF:.1f}% of the 8 TB/s roof, "
              f"{T} slab reads per window", flush=True)
    else:
        steps = EVAL_WINDOWS + T - 1
        nd = torch.rand(NODES, F, steps + O)
        get = R.train.BatchedGraphs(build).get      # one prepared graph per batch size, built on first use (the warm-up)
        run = lambda: [None for _ in R.serve.window_outputs(model, nd_dev, T, get, 0, EVAL_WINDOWS, STEP_BATCH)]      # noqa: E731
        nd_dev = nd.to(dev)
        ms = timed(run, max(2, iters // 5))
        timeline = torch.rand(steps, NODES, C, device=dev)
        one = lambda: R.ops.window_forward(timeline, 0, EVAL_WINDOWS, *head)      # noqa: E731
        ms_w = timed(one, iters)
        st = stages(lib, one)
        rd, wr = window_bytes(EVAL_WINDOWS, wc)
        k = st["window_sum"]
        print(f"(c) eval64  {ms / EVAL_WINDOWS:8.3f} ms per window   ({EVAL_WINDOWS} windows = {steps} time steps, {STEP_BATCH} per T = 1 forward: "
              f"{ms:.2f} ms in all, of which regt_window_forward {ms_w:.2f}); window_sum {k:.3f} ms head_fwd {st['head_fwd']:.3f} ms; window "
              f"kernel, chunks of {wc}: {rd / 1e9:.2f} GB read + {wr / 1e9:.2f} GB written in {k:.3f} ms = {(rd + wr) / k / 1e9:.2f} TB/s = "
              f"{100 * (rd + wr) / (k * 1e-3) / HBM_ROOF:.1f}% of the 8 TB/s roof, {rd / (NODES * C * 4) / EVAL_WINDOWS:.2f} slab reads per window "
              f"(plain form: {T})", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
        sys.exit(0)
    args, repeats, iters = sys.argv[1:], 2, 20
    while args:
        a = args.pop(0)
        if a == "--repeats":
            repeats = int(args.pop(0))
        elif a == "--iters":
            iters = int(args.pop(0))
    print(f"tools/stream_bench.py --repeats {repeats} --iters {iters} on one MI355X: cfg-3 size, fp32, one child process per leg, legs alternating.",
          flush=True)
    for rep in range(repeats):
        for leg in ("window", "serve", "eval64"):
            print(f"[#{rep}] ", end="", flush=True)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", leg, str(iters)], timeout=280)
