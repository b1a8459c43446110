#!/usr/bin/env python3
"""Time of a forward under torch.no_grad() at two shapes -- cfg-3 in fp32 (100k nodes, F = 32, 8 regions) and the cfg-5 shard in
bf16 (tools/mode_bench.py's problems) -- with peak allocated memory and both workspace sizes:
    python tools/forward_bench.py [LIB_DIR ...] [--repeats 2] [--seconds 1.0]
Every LIB_DIR (REGT_LIB_DIR: a build of this or of an earlier commit; default: the in-tree build) runs in a child process of its
own, the builds in alternation, `repeats` times each.  A build without regt_forward_only_workspace_bytes (an earlier commit) runs
the training forward, which is what its evaluation paths did.  REGT_FWD_SWITCH=0 in the environment: the training forward on a
current build.  After the timed loop a second, untimed pass collects the per-stage device times (regt_profile_collect)."""
import ctypes, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(wl: str, seconds: float):
    import numpy as np, torch
    sys.path.insert(0, ROOT)
    # (an earlier build lacks the new symbol: bind what it has, run the training forward)
    libdir = os.environ.get("REGT_LIB_DIR") or os.path.join(ROOT, "regt-gcn_amd", "lib")
    has_fo = hasattr(ctypes.CDLL(os.path.join(libdir, "libregtgcn_hip.so")), "regt_forward_only_workspace_bytes")
    import regtgcn_amd as R
    from regtgcn_amd import _lib
    if not has_fo:
        _lib.SIGNATURES.pop("regt_forward_only_workspace_bytes", None)
        _lib.SIGNATURES.pop("regt_forward_only_packed_workspace_bytes", None)
    fo = has_fo and os.environ.get("REGT_FWD_SWITCH", "1") != "0"
    R.functional.set_forward_only_in_no_grad(fo)
    lib = R.load_library()
    dev = torch.device("cuda")
    torch.manual_seed(42)
    T, O = 12, 1
    if wl == "cfg5shard":
        world, F, mode = 8, 64, 2
        gn, ge, gr = 1_000_000, 10_000_000, 64
        g = R.data.synthetic_regional_graph(gn, ge, gr, seed=42)
        rpg = gr // world
        bounds = np.asarray(g.region_bounds[::rpg], dtype=np.int64)
        sh = R.dist.build_shard(g.edge_index, g.region_index, g.region_attr, gn, bounds, [r // rpg for r in range(gr)], 0, world, dev)
        graph, nodes, regions = sh.graph, sh.topo.n_local, gr
        x = torch.rand(sh.topo.x_rows, T, F, device=dev)
        run = lambda model: model.forward_packed(x, graph)
        sizer = lambda dims, gs: lib.regt_forward_only_packed_workspace_bytes(ctypes.byref(dims), ctypes.byref(gs), x.shape[0], 0)
    else:
        nodes, edges, regions, F, mode = 100_000, 1_000_000, 8, 32, 0
        g = R.data.synthetic_regional_graph(nodes, edges, regions, seed=42)
        graph = R.prepare_graph(g.edge_index.to(dev), None, [t.to(dev) for t in g.region_index], [t.to(dev) for t in g.region_attr], nodes)
        x = torch.rand(nodes, F, T, device=dev)
        run = lambda model: model.forward_prepared(x, graph)
        sizer = lambda dims, gs: lib.regt_forward_only_workspace_bytes(ctypes.byref(dims), ctypes.byref(gs))
    lib.regt_set_gemm_mode(mode)
    model = R.RegionalTemporalGCN(F, nodes, T, O, num_regions=regions).to(dev).eval()
    dims = _lib.Dims(nodes, T, F, 256, regions, O, 128, 1, 0.01, 0, 0)
    gs = R.functional._graph_struct(graph, T)
    ws_train = lib.regt_workspace_bytes(ctypes.byref(dims), gs.n_chunks, gs.overlap)
    ws_fwd = sizer(dims, gs) if has_fo else 0
    taken, acquire = [], R.functional._POOL.acquire                     # the workspace blocks the forwards actually take
    R.functional._POOL.acquire = lambda nbytes, device: (taken.append(nbytes), acquire(nbytes, device))[1]
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        for _ in range(3):
            pred, _h = run(model)
        torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        while True:
            for _ in range(10):
                pred, _h = run(model)
            n += 10
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= seconds:
                break
        peak = torch.cuda.max_memory_allocated()
        lib.regt_profile_enable(1)
        for _ in range(5):
            run(model)
        torch.cuda.synchronize()
        lib.regt_profile_enable(0)
    buf = (ctypes.c_char * 16384)()
    _lib.check(lib.regt_profile_collect(buf, 16384), "regt_profile_collect")
    stages = {ln.split()[0]: float(ln.split()[2]) / 5 for ln in buf.value.decode().splitlines()}
    pick = " ".join(f"{k}={stages[k]:.3f}" for k in ("fused_forward", "gemm_regional", "gemm_gates", "gemm_candidate", "spmm") if k in stages)
    print(f"{wl:9s} {'forward-only' if fo else 'training-fwd':12s} {1e3 * dt / n:8.3f} ms/forward ({n} calls)  peak_alloc {peak / 2**20:9.1f} MiB "
          f"(+{(peak - base) / 2**20:.1f} over the problem)  ws_train {ws_train / 2**20:.1f} MiB  ws_forward_only {ws_fwd / 2**20:.1f} MiB  block_taken {max(taken) / 2**20:.1f} MiB  "
          f"checksum {float(pred.double().sum()):.9e}  stages[ms]: {pick}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], float(sys.argv[3]))
        sys.exit(0)
    args, dirs, repeats, seconds = sys.argv[1:], [], 2, 1.0
    while args:
        a = args.pop(0)
        if a == "--repeats":
            repeats = int(args.pop(0))
        elif a == "--seconds":
            seconds = float(args.pop(0))
        else:
            dirs.append(a)
    dirs = dirs or [os.environ.get("REGT_LIB_DIR") or os.path.join(ROOT, "regt-gcn_amd", "lib")]
    for wl in ("cfg3", "cfg5shard"):
        for rep in range(repeats):
            for d in dirs:
                print(f"[{os.path.relpath(os.path.abspath(d), ROOT)} #{rep}] ", end="", flush=True)
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", wl, str(seconds)],
                                      env=dict(os.environ, REGT_LIB_DIR=os.path.abspath(d)), timeout=500)
