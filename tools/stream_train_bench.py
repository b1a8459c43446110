#!/usr/bin/env python3
"""Streamed training against one training step per window, at cfg-3 size (synthetic, as bench.py builds it: 100k nodes,
1M edges, 8 regions, F = 32, T = 12, C = 256, fp32) over 64 consecutive windows, and at TPIMS size against --snap_batch 64:
    python tools/stream_train_bench.py [--repeats 2] > profiles/stream_train.txt
  (a) window   : the parent's way, one train_epoch step (forward, loss, backward) per window at T = 12
  (b) streamed : train.train_epoch_streamed over the same 64 windows (75 time steps), per window, with its stage split: the forward-only
                 T = 1 cell (period_outputs), ops.window_forward, ops.window_backward (both kernels with the bytes the algorithm needs and
                 TB/s against the 8 TB/s roof) and the recompute + T = 1 backward (period_gradients)
  (c) tpims64  : train_epoch_batched with 64 windows per step on the TPIMS fixture (N = 104, T = 6)
  (d) tpims_s  : train_epoch_streamed on the same windows
One child process per leg, legs alternating, `repeats` times each, every child under its own time limit (a failure ends the run); times
are HIP events after a warm-up epoch."""
import ctypes, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES, EDGES, REGIONS, F, T, O, C = 100_000, 1_000_000, 8, 32, 12, 1, 256
WINDOWS, STEP_BATCH = 64, 8
HBM_ROOF = 8.0e12
os.environ.setdefault("OMP_NUM_THREADS", "16")


def adjoint_bytes(windows: int, wc: int):
    """Bytes the adjoint kernel needs (accumulating): per chunk of ns <= wc slots the windows that cover it, ns reads and ns writes of dring."""
    slab, total = NODES * C * 4, 0
    covered = windows + T - 1
    for j0 in range(0, covered, wc):
        ns = min(wc, covered - j0)
        nwin = min(j0 + ns - 1, windows - 1) - max(0, j0 - (T - 1)) + 1
        total += (nwin + 2 * ns) * slab
    return total


def attgrad_bytes(windows: int, wc: int):
    """Bytes the attention-gradient kernel needs: per chunk of nw <= wc windows nw slabs of dhidden and nw + T - 1 of the ring."""
    slab = NODES * C * 4
    return sum((2 * min(wc, windows - w0) + T - 1) * slab for w0 in range(0, windows, wc))


def timed(fn, iters: int, warm: int = 1):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def stages(lib, fn, iters: int = 3):
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


class NoStep:
    """The epoch without its optimizer step: the weights stay, the gradients are dropped."""

    def __init__(self, model):
        self.model = model

    def step(self):
        pass

    def zero_grad(self):
        for p in self.model.parameters():
            p.grad = None


def child(leg: str):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import regtgcn_amd as R
    lib = R.load_library()
    lib.regt_set_gemm_mode(0)
    dev = torch.device("cuda")
    torch.manual_seed(42)
    if leg in ("tpims64", "tpims_s"):
        d = np.load(os.path.join(ROOT, "tests", "golden", "tpims_fixture.npz"))
        nd = torch.from_numpy(d["node_data"]).to(dev)
        n, f, t_in, t_out = nd.shape[0], nd.shape[1], 6, 1
        count = min(256, nd.shape[2] - t_in - t_out + 1)
        model = R.RegionalTemporalGCN(f, n, t_in, t_out).to(dev)
        ei = torch.from_numpy(d["edge_index"]).to(dev)
        ri = [torch.from_numpy(d[f"edge_{r}_index"]).to(dev) for r in R.train.REGIONS]
        ra = [torch.from_numpy(d[f"edge_{r}_attr"]).to(dev) for r in R.train.REGIONS]
        graphs = R.train.BatchedGraphs(lambda b: model.prepare_graph(ei, ri, ra, copies=b))
        opt = NoStep(model)
        if leg == "tpims64":
            xs, ys = R.data.snapshot_windows(nd[:, :, :count + t_in + t_out - 1].cpu(), t_in, t_out)
            store = R.train.WindowStore([x.to(dev) for x in xs], [y.to(dev) for y in ys])
            ms = timed(lambda: R.train.train_epoch_batched(model, store, graphs, opt, 64), 5)
            print(f"(c) tpims64  {ms / count * 1e3:8.2f} us per window   (train_epoch_batched, --snap_batch 64, {count} windows, N = {n}, T = {t_in}: {ms:.2f} ms)",
                  flush=True)
        else:
            ms = timed(lambda: R.train.train_epoch_streamed(model, nd, t_in, t_out, graphs.get, 0, count, opt), 5)
            print(f"(d) tpims_s  {ms / count * 1e3:8.2f} us per window   (train_epoch_streamed, {count} windows = {count + t_in - 1} time steps: {ms:.2f} ms)",
                  flush=True)
        return
    g = R.data.synthetic_regional_graph(NODES, EDGES, REGIONS, seed=42)
    model = R.RegionalTemporalGCN(F, NODES, T, O, num_regions=REGIONS).to(dev)
    ei, ri, ra = g.edge_index.to(dev), [t.to(dev) for t in g.region_index], [t.to(dev) for t in g.region_attr]
    build = lambda b: model.prepare_graph(ei, ri, ra, copies=b)      # noqa: E731
    opt = NoStep(model)
    if leg == "window":
        graph, x, y = build(1), torch.rand(NODES, F, T, device=dev), torch.rand(NODES, O, device=dev)
        ms = timed(lambda: R.train.train_epoch(model, [x] * 8, [y] * 8, graph, opt), 3) / 8
        print(f"(a) window   {ms:8.3f} ms per window   (one train_epoch step at T = {T})", flush=True)
        return
    steps = WINDOWS + T - 1
    nd = torch.rand(NODES, F, steps + O, device=dev)      # device-resident, as the windows of leg (a) are
    get = R.train.BatchedGraphs(build).get
    ms = timed(lambda: R.train.train_epoch_streamed(model, nd, T, O, get, 0, WINDOWS, opt, step_batch=STEP_BATCH), 2)
    # the stage split, each stage on its own
    x = torch.rand(STEP_BATCH, NODES, F, device=dev)
    line = torch.rand(steps, NODES, C, device=dev)
    dline = torch.zeros(steps, NODES, C, device=dev)
    att, l1, l2 = model.tgnn._attention, model.linear1, model.linear2
    head = (att, l1.weight, l1.bias, l2.weight, l2.bias)
    outs = [torch.zeros_like(p) for p in head]
    with torch.no_grad():
        ms_f = timed(lambda: model.period_outputs(x, get(STEP_BATCH), out=line[:STEP_BATCH]), 5) / STEP_BATCH
    pred, hidden = R.ops.window_forward(line, 0, WINDOWS, *head)
    ms_wf = timed(lambda: R.ops.window_forward(line, 0, WINDOWS, *head, pred=pred, hidden=hidden), 5)
    dpred = torch.rand_like(pred)
    wb = lambda: R.ops.window_backward(line, 0, WINDOWS, *head, hidden, dpred, dline, True, *outs)      # noqa: E731
    ms_wb = timed(wb, 5)
    st = stages(lib, wb)
    ms_b = timed(lambda: model.period_gradients(x, get(STEP_BATCH), dline[:STEP_BATCH]), 5) / STEP_BATCH
    opt.zero_grad()
    wc = lib.regt_window_chunk(WINDOWS)
    ab, gb = adjoint_bytes(WINDOWS, wc), attgrad_bytes(WINDOWS, wc)
    ka, kg = st["window_adjoint"], st["window_attgrad"]
    print(f"(b) streamed {ms / WINDOWS:8.3f} ms per window   ({WINDOWS} windows = {steps} time steps, {STEP_BATCH} per cell call: {ms:.1f} ms per epoch); "
          f"stages: forward-only T = 1 {ms_f:.3f} ms per step, window_forward {ms_wf:.2f} ms per {WINDOWS} windows, window_backward {ms_wb:.2f} ms per "
          f"{WINDOWS} windows, recompute + T = 1 backward {ms_b:.3f} ms per step; sum over {steps} steps = "
          f"{(steps * (ms_f + ms_b) + ms_wf + ms_wb) / WINDOWS:.3f} ms per window; window_adjoint {ab / 1e9:.1f} GB in {ka:.2f} ms = "
          f"{ab / ka / 1e9:.2f} TB/s = {100 * ab / (ka * 1e-3) / HBM_ROOF:.1f}% of the 8 TB/s roof; window_attgrad {gb / 1e9:.1f} GB in {kg:.2f} ms = "
          f"{gb / kg / 1e9:.2f} TB/s = {100 * gb / (kg * 1e-3) / HBM_ROOF:.1f}% of the roof", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2])
        sys.exit(0)
    args, repeats = sys.argv[1:], 2
    while args:
        a = args.pop(0)
        if a == "--repeats":
            repeats = int(args.pop(0))
    print(f"tools/stream_train_bench.py --repeats {repeats} on one MI355X: fp32, one child process per leg, legs alternating.", flush=True)
    for rep in range(repeats):
        for leg in ("window", "streamed", "tpims64", "tpims_s"):
            print(f"[#{rep}] ", end="", flush=True)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", leg], timeout=280)
