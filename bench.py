#!/usr/bin/env python3
"""Headline benchmark of the RegT-GCN hot path on MI355X (contract: see the task README / DESIGN.md section 6).

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Default workload "cfg3" = BASELINE.json configs[2] at N = 1 and configs[3] at N > 1: ONE synthetic regional graph of
100 000 nodes / 1 000 000 directed edges / 8 regions / 32 node features / T = 12 periods / horizon 1, fp32.  With N GPUs
the graph is split by regions (8 / N regions per GPU, one at N = 8 -- STRONG scaling, total work fixed): rank g owns a block
of regions, exchanges the packed halo rows over RCCL every step (personalised all-to-all, one step ahead on a side stream)
and all-reduces the gradient buffer once before the optimiser step.  ``value`` = whole-graph snapshots per second.
``--scaling weak`` is the opt-in in which every GPU owns a full workload-sized shard (global graph N x larger; ``value`` =
shard snapshots per second over all ranks); it is the default only for ``--workload cfg5`` (BASELINE configs[4]: the global
graph at N = 8 is 1M nodes / 10M edges / 64 regions / F = 64, bf16 GEMM operands).  ``--workload cfg5shard`` runs rank 0's
share of that 8-GPU job on ONE GPU (125k nodes, 8 of 64 regions, halo rows filled with random data, no communication).

A "step" is what the reference's run.py::train() does per snapshot: forward, mean((out-y)^2), backward with gradients
accumulating (run.py:178-191); the optimiser (RMSprop, run.py:145) steps once per epoch, here once at the end of the K timed
steps, inside the timed region.

A plain run sets up, warms up, times the K steps and prints the result line (``value``, ``ms_per_step`` = one timed step).
Everything else is measured only with ``--full`` (the ``--no-*`` options then leave out single parts):
``value`` is timed without per-stage events; the stage table and ``roofline`` come from a second pass of the same K steps with
the library's HIP events on (dominant kernel; events recorded on the stream each kernel is launched on: regt_profile_*; ``traffic`` from the tracked rocprofv3 PMC summary named in ``traffic_source`` when that file holds the
kernel this run launched, else null), the other GEMM arithmetics, the TPIMS-size and configs[4] legs, and ``cpu_baseline`` (the
oracle's eager-faithful CPU path on this box's host cores, rank 0, N = 1 only, bounded sample).

``--dump-outputs DIR`` writes what the timed steps computed, from rank 0, as DIR/<name>.npy (float32): ``pred``, ``hidden`` and
``loss`` of the last timed step, ``grad.<parameter>`` = the gradients accumulated over the K timed steps (copied once, right before
the optimiser step that closes the timed region) and ``param.<parameter>`` = the parameters after that step.  An array of more
than 2^20 elements is written as a fixed sample of them (seeded indices into the flattened array, the same in every run), so
that the files stay well under 64 MB.  The inputs are seeded: the same arguments give the same inputs in every run.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP32_MATRIX_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CUs, 2.4 GHz
PEAK_BF16_MATRIX_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA (the ~5 PF headline includes 2:1 sparsity)
PEAK_HBM_GBS = 8000.0             # HBM3E spec peak (6.3 TB/s is the measured achievable copy rate)

# HBM bytes per launch come from rocprofv3 PMC passes of this same command (tools/bench_pmc.sh -> tools/pmc_summary.py):
# 2 x FETCH_SIZE (gfx950 reports half the bytes of 16-B/lane streaming reads -- MI355X_MICROARCH.md, HBM section;
# calibrated on cell_bwd, whose 3.7 GB of float4 reads show as 2.08e6 KB) + WRITE_SIZE, both in KB in the summary.
PMC_SUMMARIES = {("cfg3", 0): "profiles/r05_cfg3_pmc_hbm_summary.txt",
                 ("cfg5shard", 2): "profiles/r05_cfg5shard_pmc_hbm_summary.txt"}

WORKLOADS = {
    # per-GPU shape: nodes, edges, regions, F, T, O; GEMM arithmetic (regt_set_gemm_mode) and the dtype it computes in
    "cfg3": dict(nodes=100_000, edges=1_000_000, regions=8, F=32, T=12, O=1, mode=0, dtype="fp32", scaling="strong"),
    "small": dict(nodes=20_000, edges=200_000, regions=8, F=32, T=12, O=1, mode=0, dtype="fp32", scaling="strong"),
    # cfg-3 with the region count of the 8-GPU weak-scaling global graph (composition cost check)
    "cfg3r64": dict(nodes=100_000, edges=1_000_000, regions=64, F=32, T=12, O=1, mode=0, dtype="fp32", scaling="strong"),
    # BASELINE configs[4] = 8 of these: 1M nodes / 10M edges / 64 regions / F=64, bf16 GEMM operands, fp32 accumulate
    "cfg5": dict(nodes=125_000, edges=1_250_000, regions=8, F=64, T=12, O=1, mode=2, dtype="bf16", scaling="weak"),
    "cfg5shard": dict(nodes=125_000, edges=1_250_000, regions=8, F=64, T=12, O=1, mode=2, dtype="bf16", scaling="weak"),
    # BASELINE configs[4] WHOLE on one GPU (the N = 1 anchor of its scaling curve): 1M nodes / 10M edges / 64 regions / F = 64, bf16
    "cfg5full": dict(nodes=1_000_000, edges=10_000_000, regions=64, F=64, T=12, O=1, mode=2, dtype="bf16", scaling="strong"),
}
MODE_NAMES = {0: "fp32 MFMA (v_mfma_f32_32x32x2_f32)", 1: "exact 3-way bf16 split, 6 x v_mfma_f32_32x32x16_bf16, fp32 accumulate",
              2: "bf16 operands (RNE at LDS staging), v_mfma_f32_32x32x16_bf16, fp32 accumulate"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="cfg3", choices=sorted(WORKLOADS))
    ap.add_argument("--scaling", default=None, choices=["weak", "strong"],
                    help="N > 1: strong (default for cfg3 = BASELINE configs[3]) splits the ONE workload graph by regions over the "
                         "GPUs; weak (default for cfg5 = configs[4]) gives every GPU a full workload-sized shard")
    ap.add_argument("--gemm-mode", type=int, default=None, choices=[0, 1, 2], help="override the workload's GEMM arithmetic")
    ap.add_argument("--force-shard-path", action="store_true",
                    help="N = 1 only: run the region-shard code path (packed input, halo pipeline, RCCL calls) with a 1-rank "
                         "process group -- a rehearsal of what N > 1 executes, not a measurement")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cfg1-cpu-epoch", action="store_true",
                    help="cpu_baseline leg only (no GPU): time the oracle over one epoch of the TPIMS fixture (SURVEY 8(d), cfg-1) and exit")
    ap.add_argument("--no-split-leg", action="store_true", help="skip the secondary bf16x3-split / bf16 measurements")
    ap.add_argument("--no-tpims-leg", action="store_true", help="skip the secondary TPIMS-scale (configs[1]) measurement")
    ap.add_argument("--no-cfg5-leg", action="store_true",
                    help="skip the secondary cfg5shard leg (one rank's share of BASELINE configs[4], bf16 arithmetic, run as a child process)")
    ap.add_argument("--no-profile", action="store_true", help="do not record per-stage HIP events")
    ap.add_argument("--cpu-baseline-only", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: per-stage events and roofline, the other GEMM arithmetics, the TPIMS-size and "
                         "configs[4] legs, cpu_baseline (the --no-* options leave parts out); a plain run measures the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the timed steps as DIR/<name>.npy (module docstring)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_MAX_ELEMENTS = 1 << 20        # per array; larger outputs are written as a fixed, seeded sample of this many elements


def dump_outputs(out_dir, arrays):
    """arrays: name -> tensor (any device / float dtype); written as float32 .npy, a seeded sample of the flattened array when it
    holds more than DUMP_MAX_ELEMENTS elements (same indices in every run: they depend on the element count only)."""
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        t = t.detach()
        n = t.numel()
        if n > DUMP_MAX_ELEMENTS:
            idx = np.unique(np.random.default_rng(n).integers(0, n, DUMP_MAX_ELEMENTS))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        a = t.float().cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a)
        total += a.nbytes
    if total > 64 << 20:
        raise SystemExit(f"--dump-outputs wrote {total / 2**20:.1f} MiB, more than the 64 MiB budget")
    return total


def host_info():
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return {"cpu_model": model, "os_cpu_count": os.cpu_count(), "affinity_cpus": avail}


def cfg1_cpu_epoch():
    """SURVEY 8(d), cfg-1 -- part of the cpu_baseline leg (the only place outside tests/ that may run the oracle): the reference CPU
    path (oracle = op-for-op restatement, run.py:163-226 loop semantics) timed over one EPOCH of the TPIMS fixture -- every window,
    train split (forward + loss + backward, one RMSprop step at the end) and test split (forward only) at --tr 0.2 as in
    scripts/RegionalTemporalGCN.sh -- at T = 6 and T = 12, with torch's default thread count and with one thread.  The authors'
    14-day dataset has 2010 windows per epoch (402 train / 1608 test); the fixture holds 60 timesteps, so the per-snapshot rates are
    what an epoch of any length costs.    python bench.py --cfg1-cpu-epoch > profiles/rNN_cfg1_cpu_epoch.txt"""
    from oracle import loop as L, model as M
    z = np.load(os.path.join(ROOT, "tests", "golden", "tpims_fixture.npz"))
    fx = {k: torch.from_numpy(z[k]) for k in z.files if z[k].ndim > 0}
    regs = ("IA", "KS", "KY", "OH", "WI")
    ri, rw = [fx[f"edge_{r}_index"] for r in regs], [fx[f"edge_{r}_attr"] for r in regs]
    n = fx["node_data"].shape[0]
    cpu = "unknown"
    for line in open("/proc/cpuinfo"):
        if line.startswith("model name"):
            cpu = line.split(":", 1)[1].strip()
            break
    default_threads = torch.get_num_threads()
    print(f"host: {cpu}; os.cpu_count() = {os.cpu_count()}; affinity = {len(os.sched_getaffinity(0))}; torch default threads = {default_threads}")
    for t_in in (6, 12):
        xs, ys = L.make_windows(fx["node_data"], t_in, 1)
        (tx, ty), (vx, vy) = L.split(xs, ys, 0.2)
        for threads in (default_threads, 1):
            torch.set_num_threads(threads)
            p = {k: v.clone().requires_grad_(True) for k, v in M.init_params("RegionalTemporalGCN", 8, t_in, 1, num_nodes=n, seed=0).items()}
            opt = torch.optim.RMSprop(list(p.values()), lr=1e-3, weight_decay=1e-4)
            fwd = lambda q, x: M.regional_temporal_gcn(q, x, fx["edge_index"], ri, rw)      # noqa: E731
            L.train_epoch(p, fwd, tx[:2], ty[:2], opt)                      # warm-up
            t0 = time.perf_counter()
            L.train_epoch(p, fwd, tx, ty, opt)
            t_train = time.perf_counter() - t0
            t0 = time.perf_counter()
            L.evaluate(p, fwd, vx, vy)
            t_test = time.perf_counter() - t0
            tr, te = len(tx) / t_train, len(vx) / t_test
            print(f"T={t_in:2d} O=1 threads={threads:3d}: train {len(tx)} snapshots in {t_train:6.2f} s = {tr:6.1f} snapshots/s (fwd+bwd); "
                  f"test {len(vx)} snapshots in {t_test:6.2f} s = {te:6.1f} snapshots/s (fwd); a 402 + 1608 epoch = {402 / tr + 1608 / te:6.1f} s")
    torch.set_num_threads(default_threads)


def cpu_baseline(nodes, edges, regions, F, T, O, seed=42, model_regions=None, scale_regions=1, note=""):
    """Oracle (op-for-op restatement of the reference CPU path) on the host cores: 1 warm-up + 3 timed runs, median.

    A full T=12 step at cfg-3 size needs > 57 GB and ~90 s, so the bounded sample is ONE period
    (T=1) of the same graph, forward + loss + backward; periods are independent in the reference
    (RegionalTemporalGCN.py:135-148), so the step time is T x the period time.  ``model_regions`` > ``regions``: the sample
    graph holds ``regions`` of the model's regions (a region shard); ``scale_regions``: the sample is 1/scale of the rank's
    node set (whole regions), per-node work is identical, so the step time is scale x the sample's."""
    import regtgcn_amd as R
    from oracle import model as M
    info = host_info()
    g = R.data.synthetic_regional_graph(nodes, edges, regions, seed=seed)
    (x, y), = R.data.synthetic_snapshots(nodes, F, 1, O, 1, seed=seed)
    mr = model_regions or regions
    p = M.init_params("RegionalTemporalGCN", F, 1, O, num_nodes=nodes, num_regions=mr, seed=seed)
    empty_i, empty_w = torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0)
    ri = list(g.region_index) + [empty_i] * (mr - regions)
    rw = list(g.region_attr) + [empty_w] * (mr - regions)

    def sample(threads, timed):
        torch.set_num_threads(threads)
        times = []
        for it in range(1 + timed):                # first run = warm-up (allocator, thread pool)
            q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
            t0 = time.perf_counter()
            pred, _ = M.regional_temporal_gcn(q, x, g.edge_index, ri, rw)
            loss = torch.mean((pred - y) ** 2)
            loss.backward()
            if it:
                times.append(time.perf_counter() - t0)
            del q, pred, loss
        return times

    # The host share of a 1-GPU box is not a given: the same sample is timed with 16 threads (3 timed runs), with min(affinity,
    # 64) and with min(affinity, 128) threads (2 timed runs each), and the FASTEST setting is the baseline -- all of them are
    # printed.  (Round 2 fixed 16 threads by assumption; the verdict asked for the measurement.)
    avail = info["affinity_cpus"]
    cand = []
    for th in (min(avail, 16), min(avail, 64), min(avail, 128)):
        if th not in cand:
            cand.append(th)
    runs = {}
    for i, th in enumerate(cand):
        ts = sample(th, 3 if i == 0 else 2)
        runs[th] = {"median_s": round(statistics.median(ts), 3), "period_s": [round(t, 3) for t in ts]}
    best = min(runs, key=lambda th: runs[th]["median_s"])
    dt = runs[best]["median_s"]
    return {"value": 1.0 / (dt * T * scale_regions), "unit": "snapshots/s", "cores": best, "kind": "port",
            "threads": best, **info, "period_s": runs[best]["period_s"], "by_threads": {str(k): v for k, v in runs.items()},
            "sample": f"1 warm-up + 2-3 timed runs per thread count {cand} (best: {best} threads, median {dt:.2f} s) of 1 of {T} periods "
                      f"(T=1 forward+loss+backward) of a {nodes}-node/{edges}-edge/{regions}-region graph{note}; periods are "
                      f"independent, step time = {T}{' x ' + str(scale_regions) if scale_regions > 1 else ''} x period time"}


def tpims_leg(dev, steps=300, warmup=30, with_cpu=True):
    """BASELINE.json configs[1]: the reference's own graph (TPIMS, 104 sites after its site filter, 5 regions, F = 8), T = 12,
    horizon 1 -- the other configuration the metric names.  Same step semantics as the headline loop; this size is bound
    by the latency of ~45 dependent small kernels, not by any roofline."""
    import regtgcn_amd as R
    z = np.load(os.path.join(ROOT, "tests", "golden", "tpims_fixture.npz"))
    fx = {k: torch.from_numpy(z[k]) for k in z.files if z[k].ndim > 0}
    regs = ("IA", "KS", "KY", "OH", "WI")
    n, T, O = fx["node_data"].shape[0], 12, 1
    torch.manual_seed(42)
    model = R.RegionalTemporalGCN(8, n, T, O).to(dev)
    graph = model.prepare_graph(fx["edge_index"].to(dev), [fx[f"edge_{r}_index"].to(dev) for r in regs],
                                [fx[f"edge_{r}_attr"].to(dev) for r in regs])
    xs, ys = R.data.snapshot_windows(fx["node_data"], T, O)
    xs, ys = [x.to(dev) for x in xs], [y.to(dev) for y in ys]
    opt = torch.optim.RMSprop(model.parameters(), lr=1e-3, weight_decay=1e-4)

    def run(k):
        for i in range(k):
            pred, _ = model.forward_prepared(xs[i % len(xs)], graph)
            torch.mean((pred - ys[i % len(xs)]) ** 2).backward()
        opt.step()
        opt.zero_grad(set_to_none=False)
        torch.cuda.synchronize()

    run(warmup)
    t0 = time.perf_counter()
    run(steps)
    dt = time.perf_counter() - t0
    # the same steps through functional.FusedTrainStep (three C-ABI calls + one axpy per step, no autograd)
    stepper = R.functional.FusedTrainStep(model, graph, 8, T)

    def run_fused(k):
        for i in range(k):
            stepper(xs[i % len(xs)], ys[i % len(xs)])
        opt.step()
        stepper.zero_grad()
        torch.cuda.synchronize()

    run_fused(warmup)
    t0 = time.perf_counter()
    run_fused(steps)
    dtf = time.perf_counter() - t0
    # snapshot batching (train.train_epoch_batched, --snap_batch B): B snapshots per forward / backward on the block-diagonal graph of B
    # copies -- the same accumulated gradients (run.py:170-192 is additive over snapshots), M = B*N*T rows per launch
    ei_d, ri_d, rw_d = fx["edge_index"].to(dev), [fx[f"edge_{r}_index"].to(dev) for r in regs], [fx[f"edge_{r}_attr"].to(dev) for r in regs]
    graphs = R.train.BatchedGraphs(lambda b: model.prepare_graph(ei_d, ri_d, rw_d, copies=b))
    batched = {}
    for B in (16, 64, 256):
        reps = (4 * B + len(xs) - 1) // len(xs)
        store = R.train.WindowStore((xs * reps)[:4 * B], (ys * reps)[:4 * B])       # 4 batches per "epoch"
        epochs = max(2, steps // (4 * B) + 1)
        R.train.train_epoch_batched(model, store, graphs, opt, B)                   # warm-up (graph build, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(epochs):
            R.train.train_epoch_batched(model, store, graphs, opt, B)
        torch.cuda.synchronize()
        dtb = time.perf_counter() - t0
        nsnap = epochs * len(store)
        batched[str(B)] = {"value": nsnap / dtb, "unit": "snapshots/s", "ms_per_batched_step": 1e3 * dtb / (epochs * 4), "snapshots": nsnap,
                           "rows_per_launch": B * n * T}
    best_b = max(batched, key=lambda k: batched[k]["value"])
    cpu = None
    if with_cpu:                                # the oracle (CPU restatement of the reference path) on the same snapshots
        from oracle import model as M
        info = host_info()
        p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()}
        ri, rw = [fx[f"edge_{r}_index"] for r in regs], [fx[f"edge_{r}_attr"] for r in regs]
        xc, yc = [x.cpu() for x in xs[:4]], [y.cpu() for y in ys[:4]]
        k_cpu, by_threads = 12, {}
        default_threads = torch.get_num_threads()
        for th in sorted({1, min(4, info["affinity_cpus"]), min(16, info["affinity_cpus"])}):     # the best thread count is the baseline
            torch.set_num_threads(th)
            rates = []
            for rep in range(4):                # first repeat = warm-up; median of the other three
                t1 = time.perf_counter()
                for i in range(k_cpu):
                    pr, _ = M.regional_temporal_gcn(p, xc[i % 4], fx["edge_index"], ri, rw)
                    torch.mean((pr - yc[i % 4]) ** 2).backward()
                if rep:
                    rates.append(k_cpu / (time.perf_counter() - t1))
            by_threads[th] = statistics.median(rates)
        torch.set_num_threads(default_threads)
        best = max(by_threads, key=by_threads.get)
        cpu = {"value": by_threads[best], "unit": "snapshots/s", "kind": "port", "cores": best, "threads": best, **info,
               "by_threads": {str(k): round(v, 2) for k, v in by_threads.items()},
               "sample": f"per thread count {sorted(by_threads)}: 1 warm-up + 3 timed repeats (median) of {k_cpu} forward+loss+backward steps "
                         f"of the oracle on the same snapshots; best = {best} threads"}
    # `value` is the run.py-faithful number -- one forward / backward per snapshot through the drop-in module, what `cpu_baseline`
    # (the unbatched oracle) is the counterpart of; snapshot batching is a different algorithm (equally open to a CPU port) and is
    # reported under its own key, with the batch size in the name
    return {"value": steps / dt, "unit": "snapshots/s", "ms_per_step": 1e3 * dt / steps, "steps": steps,
            "state": "one launch sequence per snapshot through nn.RegionalTemporalGCN + autograd, as run.py:170-192 (latency-bound: ~40 dependent launches)",
            "per_snapshot_launches": {"value": steps / dt, "unit": "snapshots/s", "ms_per_step": 1e3 * dt / steps, "steps": steps,
                                      "note": "= the leg's `value` (kept under the round-4 key for trend lines)"},
            "fused_train_step": {"value": steps / dtf, "unit": "snapshots/s", "ms_per_step": 1e3 * dtf / steps},
            "snap_batch": batched,
            "best_snap_batch": {"snap_batch": int(best_b), "value": batched[best_b]["value"], "unit": "snapshots/s",
                                "note": "train.py --snap_batch B: B snapshots per forward / backward on the block-diagonal graph (same accumulated "
                                        "gradients); NOT comparable with cpu_baseline, which runs one snapshot at a time"},
            "cpu_baseline": cpu,
            "workload": f"TPIMS fixture: {n} nodes / {fx['edge_index'].shape[1]} edges / 5 regions, F=8, T={T}, O={O} (BASELINE configs[1])"}


def cfg5shard_leg(args):
    """BASELINE.json configs[4] on the hardware the driver has: rank 0's share of the 8-GPU job (125 000 own nodes + halo rows,
    8 of 64 regions, F = 64, bf16 GEMM operands) as a child process of this bench -- its own library state, its own JSON line
    with the roofline of ITS dominant kernel.  Secondary leg: never the headline value."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--workload", "cfg5shard", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--full", "--no-cpu-baseline", "--no-split-leg", "--no-tpims-leg"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not line:
            return {"error": f"child exited {r.returncode}", "stderr_tail": r.stderr[-400:]}
        leg = json.loads(line[-1])
        leg.pop("stages", None)          # the per-stage table of the leg: `python bench.py --workload cfg5shard` prints it
        return leg
    except Exception as e:               # a secondary leg must never take the headline line down
        return {"error": repr(e)}


def cfg5full_leg(args):
    """BASELINE.json configs[4] WHOLE on one MI355X (1 000 000 nodes / 10 000 000 edges / 64 regions / F = 64, bf16): the N = 1 anchor
    of its scaling curve, as a child process (own library state, own peak-memory figure).  Secondary leg: never the headline value."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--workload", "cfg5full", "--steps", str(min(args.steps, 10)), "--warmup", str(min(args.warmup, 2)),
           "--full", "--no-cpu-baseline", "--no-split-leg", "--no-tpims-leg", "--no-cfg5-leg"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not line:
            return {"error": f"child exited {r.returncode}", "stderr_tail": r.stderr[-400:]}
        leg = json.loads(line[-1])
        keep = {k: leg[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup", "dtype", "n_gpus") if k in leg}
        keep["workload"] = leg["config"]["workload"]
        keep["peak_memory_gb"] = leg["config"].get("peak_memory_gb")
        keep["top_stages_ms"] = {k: round(v["avg_ms"], 4) for k, v in sorted(leg.get("stages", {}).items(), key=lambda kv: -kv[1]["avg_ms"])[:8]}
        return keep
    except Exception as e:               # a secondary leg must never take the headline line down
        return {"error": repr(e)}


def stage_flops(stage, M, C, F):
    if stage == "fused_forward":        # regional embedding + gates + candidate in one kernel (bf16 arithmetic, csrc/fused.hip)
        return 2.0 * M * (C * 2 * F + 2 * C * (C + F) + C * (C + F))
    if stage == "fused_backward":       # cell_bwd + dgrad_candidate + dgrad_gates in one kernel (bf16 arithmetic, csrc/fused.hip)
        return 2.0 * M * 3 * C * C
    return {
        "gemm_gates": 2.0 * M * 2 * C * (C + F), "gemm_candidate": 2.0 * M * C * (C + F),
        "gemm_regional": 2.0 * M * C * 2 * F, "dgrad_candidate": 2.0 * M * C * C, "dgrad_gates": 2.0 * M * C * 2 * C,
        "wgrad_Uh": 2.0 * M * C * C, "wgrad_Uzr": 2.0 * M * 2 * C * C, "wgrad_Gh": 2.0 * M * C * F,
        "wgrad_Gzr": 2.0 * M * 2 * C * F, "wgrad_A0": 2.0 * M * C * F, "wgrad_Ar": 2.0 * M * C * F, "wgrad_A0_Ar": 2.0 * M * C * 2 * F,
        # paired launches of the bf16-row layout (round 4): dhp^T [q | A_hat x], dzr^T [h | A_hat x]
        "wgrad_UhGh": 2.0 * M * C * (C + F), "wgrad_UzrGzr": 2.0 * M * 2 * C * (C + F),
    }.get(stage)


def stage_bytes(stage, M, C, F, mode=0, xbf=False, gen=False):
    """Algorithmic HBM bytes of one launch: every activation operand read once, every result written once; weights and
    per-node vectors are negligible.  fp32 storage (4 B) except under GEMM mode 2 (bf16), where the M x C activations
    (h, [Z|R], q, H~, dh, dhp, dzp|drp) are stored as bf16 (2 B); x, A_hat x, L~ x are fp32 rows unless ``xbf`` (the bf16-row
    layout of the fused forward).  DESIGN.md section 5."""
    a = 2.0 if mode == 2 else 4.0       # bytes per element of an M x C activation
    x = 2.0 if xbf else 4.0             # bytes per element of x, A_hat x, L~ x
    per_row = {
        "gemm_gates": a * C + x * F + a * 2 * C + a * C,            # read h, A_hat x; write [Z|R], q
        "gemm_candidate": a * C + x * F + a * C + a * C + a * C,    # read q, A_hat x, Z, h; write H~
        "gemm_regional": x * 2 * F + a * C,                         # read x, L~ x; write h
        "fused_forward": x * 3 * F + a * 5 * C,                     # read x, L~ x, A_hat x; write h, [Z|R], q, H~ -- nothing read back
        "fused_backward": a * 4 * C + a * 4 * C,                    # read Z, R, h, H~; write dhp, dzp, drp, ds
        "cell_bwd": a * 3 * C + a * 2 * C,                          # read Z, h, H~; write dhp, dzp
        # two launches: read dhp, h, Z, R; write drp, dh.  `gen` (fp32, round 4: cell_bwd folded in, gemm_dgrad1_gen_kernel):
        # read Z, H~, h, R; write dhp, dzp, drp, dh -- the left operand is formed from Z, H~, dOH while it is staged
        "dgrad_candidate": (a * 4 * C + a * 4 * C) if gen else (a * (C + C + 2 * C) + a * 2 * C),
        "dgrad_gates": a * (2 * C + C + C) + a * C,                 # read dzp|drp, dh, h; write ds
        "wgrad_Uzr": a * 3 * C, "wgrad_Uh": a * 2 * C, "wgrad_Gzr": a * 2 * C + x * F, "wgrad_Gh": a * C + x * F,
        "wgrad_A0_Ar": a * C + x * 2 * F,
        "wgrad_UhGh": a * 2 * C + x * F, "wgrad_UzrGzr": a * 3 * C + x * F,      # each operand once: dhp, q, A_hat x / dzr, h, A_hat x
    }.get(stage)
    return None if per_row is None else M * per_row


# stage -> (substring of the kernel it launches) per GEMM mode, for matching PMC summaries
def stage_kernel(stage, mode):
    """Substrings of the kernel names a stage may launch under GEMM mode ``mode`` (first match in a PMC summary wins): the
    three-workgroup core gemm_flat_split_kernel<Epi, REGION, NP> with NP = 0 (fp32 planes) / 3 (bf16x3) / 1 (bf16), or the
    8-column epilogue kernels when bf16 mode stores the activations as bf16."""
    np_ = {0: 0, 1: 3, 2: 1}[mode]
    epi = {"gemm_gates": "EpiGates", "dgrad_candidate": "EpiDgrad1", "dgrad_gates": "EpiDgrad2"}.get(stage)
    if epi:
        pats = [f"gemm_flat_split_kernel<regt::{epi}F, false, {np_}>"]
        if stage == "dgrad_candidate" and mode == 0:
            pats.insert(0, "gemm_dgrad1_gen_kernel")
        if mode == 2:
            pats.insert(0, f"gemm_flat_split8_kernel<regt::{epi}8F, false>")
        return pats
    if stage == "fused_forward":
        return ["fused_fwd_rows_kernel", "fused_fwd_kernel"]
    if stage == "fused_backward":
        return ["fused_bwd_kernel"]
    if stage == "gemm_candidate":
        return {0: ["gemm_cand_split_kernel<0>", "gemm_cand_flat_kernel<regt::FastCore"],
                1: ["gemm_cand_split_kernel<3>", "gemm_cand_flat_kernel<regt::SplitCore<false, 3>"],
                2: ["gemm_cand_split8_kernel", "gemm_cand_flat8_kernel", "gemm_cand_flat_kernel<regt::SplitCore<false, 1>"]}[mode]
    if stage in ("wgrad_Uzr", "wgrad_Uh", "wgrad_UhGh", "wgrad_UzrGzr"):
        return ["wgrad_kernel<128"] if mode == 0 else ["wgrad_bf16_ring_kernel", "wgrad_split_kernel"]
    if stage == "cell_bwd":
        return ["cell_bwd8_kernel", "cell_bwd_kernel"] if mode == 2 else ["cell_bwd_kernel"]
    if stage == "spmm":
        return ["spmm_dual_panel_bf16_kernel", "spmm_dual_panel_kernel"] if mode == 2 else ["spmm_dual_panel_kernel"]
    if stage == "gemm_regional":
        return ["embed_fp32_kernel", "gemm_flat_split_kernel<regt::EpiBiasActF, true"]
    return None


def pmc_traffic(workload, mode, stage):
    """(bytes per launch, source file) from the tracked PMC summary of this workload, or (None, None) when the file is absent
    or does not hold the kernel this run launches for ``stage`` (e.g. it was taken with an older kernel generation)."""
    path = PMC_SUMMARIES.get((workload, mode))
    pats = stage_kernel(stage, mode)
    if not path or not pats or not os.path.exists(os.path.join(ROOT, path)):
        return None, None
    with open(os.path.join(ROOT, path)) as f:
        lines = f.readlines()
    for pat in pats:
        fetch = write = None
        for line in lines:
            if pat not in line:
                continue
            m = re.search(r"FETCH_SIZE=([0-9.e+]+)", line)
            if m and fetch is None:
                fetch = float(m.group(1))
            m = re.search(r"WRITE_SIZE=([0-9.e+]+)", line)
            if m and write is None:
                write = float(m.group(1))
        if fetch is not None and write is not None:
            return 2.0 * fetch * 1024 + write * 1024, path
    return None, None


def main():
    args = parse()
    wl = dict(WORKLOADS[args.workload])
    nodes, edges, regions, F, T, O = wl["nodes"], wl["edges"], wl["regions"], wl["F"], wl["T"], wl["O"]
    mode = wl["mode"] if args.gemm_mode is None else args.gemm_mode
    dtype = {0: "fp32", 1: "fp32", 2: "bf16"}[mode]
    if args.cfg1_cpu_epoch:
        cfg1_cpu_epoch()
        return
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline(nodes, edges, regions, F, T, O)))
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        # plain `python bench.py --gpus N`: start the N ranks ourselves, as fresh children, BEFORE this process touches the GPU
        # (nothing above initialises HIP; a process that has must never exec another program on this pool), and hand back their code
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run for N>1 (or without a launcher)")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (torch.cuda.is_available() is False); there is no CPU path")
    shard_of_8 = args.workload == "cfg5shard"
    if shard_of_8 and world != 1:
        raise SystemExit("--workload cfg5shard is one rank's share on ONE GPU; use --workload cfg5 for N > 1")
    backend = os.environ.get("REGT_BENCH_BACKEND", "nccl")     # "gloo": rehearsal of the N>1 flow on a 1-GPU box
    if backend == "gloo":
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as dist
    force_shard = args.force_shard_path and world == 1 and not shard_of_8
    if force_shard:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29555")
        os.environ["REGT_DIST_FORCE"] = "1"          # collectives run even though the group has one rank
    if world > 1 or force_shard:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    import regtgcn_amd as R
    from regtgcn_amd import _lib
    lib = R.load_library()
    lib.regt_set_gemm_mode(mode)

    # ---- data: global graph (strong: the workload itself; weak: world x the workload shape), this rank's shard --------
    scaling = args.scaling or wl["scaling"]
    weak = scaling == "weak" and world > 1
    vworld = 8 if shard_of_8 else world            # cfg5shard: the shard topology of an 8-rank job, executed by one rank
    if weak or shard_of_8:
        gnodes, gedges, gregions = nodes * vworld, edges * vworld, regions * vworld
    else:
        if regions % world:
            raise SystemExit(f"--scaling strong needs the {regions} regions to divide evenly over {world} GPUs")
        gnodes, gedges, gregions = nodes, edges, regions
    g = R.data.synthetic_regional_graph(gnodes, gedges, gregions, seed=42)
    rpg = gregions // vworld                                                 # regions per GPU
    owner_bounds = np.asarray(g.region_bounds[::rpg], dtype=np.int64)        # contiguous region blocks
    n_local = int(owner_bounds[rank + 1] - owner_bounds[rank])               # this rank's node count
    C = R.nn.HIDDEN
    torch.manual_seed(42)                     # same random-init weights on every rank (run.py:71)
    model = R.RegionalTemporalGCN(node_features=F, num_nodes=n_local, periods=T, output_dim=O, num_regions=gregions)
    model = model.to(dev)
    n_snap = 4
    # the global snapshot is the concatenation of per-rank row blocks, each drawn from its own seeded stream, so a rank
    # only ever materialises its own rows (8 ranks x the 800k-node tensor would be ~40 GB of host memory)
    snaps = R.data.synthetic_snapshots(n_local, F, T, O, n_snap, seed=42 + 1000 * rank)
    xs = [x.to(dev) for x, _ in snaps]
    ys = [y.to(dev) for _, y in snaps]
    del snaps
    pipe = None
    # bf16 arithmetic at the shape the fused forward covers: x, A_hat x, L~ x are bf16 rows (a region shard packs and exchanges
    # its rows as bf16)
    rows_bf16 = mode == 2 and F in (32, 64) and (T * F) % 64 == 0 and regions > 1 and os.environ.get("REGT_XBF", "1") != "0"
    if world == 1 and not force_shard and not shard_of_8:
        graph = R.prepare_graph(g.edge_index.to(dev), None, [t.to(dev) for t in g.region_index],
                                [t.to(dev) for t in g.region_attr], n_local)
        shard = None
    else:
        region_owner = [r // rpg for r in range(gregions)]
        shard = R.dist.build_shard(g.edge_index, g.region_index, g.region_attr, gnodes, owner_bounds, region_owner,
                                   rank, vworld, dev)
        graph = shard.graph
        if shard_of_8:          # no peers: own rows packed once per snapshot, halo rows = random data (input values only)
            ext = []
            for x in xs:
                buf = torch.rand(shard.topo.x_rows, T, F, device=dev)
                if rows_bf16:
                    buf = buf.to(torch.bfloat16)
                    R.ops.pack_x_bf16_into(x, buf)
                else:
                    R.ops.pack_x_into(x, buf)
                ext.append(buf)
        else:
            pipe = R.dist.HaloPipeline(shard, T, F, dev, dtype=torch.bfloat16 if rows_bf16 else torch.float32)
    del g
    opt = torch.optim.RMSprop(model.parameters(), lr=1e-3, weight_decay=1e-4)   # run.py:145
    params = list(model.parameters())
    # run.py accumulates the gradients of an epoch's snapshots (run.py:178-194): the model's backward adds into .grad itself (one
    # multi-tensor add per step instead of one autograd add per parameter; same values, functional.py)
    R.functional.set_grad_accumulation_in_backward(os.environ.get("REGT_ACC_IN_BACKWARD", "1") != "0")      # (=0: A/B)
    counter = [0]                             # ONE monotonically increasing step index over warm-up, timed loop and extra legs
    if pipe is not None:
        pipe.submit(0, xs[0])
    dump = args.dump_outputs is not None and rank == 0
    last = {}                                 # --dump-outputs: pred / hidden of the last timed step
    with_grad, grad_copy = [], []             # --dump-outputs: (name, parameter) with a gradient, and its copy

    def step(keep=False):
        i = counter[0]
        counter[0] += 1
        x, y = xs[i % n_snap], ys[i % n_snap]
        if shard is None:
            pred, hidden = model.forward_prepared(x, graph)
        elif pipe is None:
            pred, hidden = model.forward_packed(ext[i % n_snap], graph)
        else:
            # the halo rows of snapshot i were exchanged while step i-1 computed; start snapshot i+1's exchange now
            xp_ext = pipe.acquire(i % 2)
            pipe.submit((i + 1) % 2, xs[(i + 1) % n_snap])
            pred, hidden = model.forward_packed(xp_ext, graph)
        if keep:
            last["pred"], last["hidden"] = pred.detach(), hidden.detach()
        loss = R.functional.mse_loss(pred, y, gnodes * O)   # mean over the GLOBAL graph (run.py:180): value + gradient in one kernel
        loss.backward()
        if pipe is not None:
            pipe.release(i % 2)
        return loss

    ar_events = []

    def epoch_end(keep=False):
        if world > 1 or force_shard:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            R.dist.allreduce_gradients(params)
            e1.record()
            ar_events.append((e0, e1))
        else:
            R.dist.allreduce_gradients(params)
        if keep:                              # --dump-outputs: the accumulated gradients the optimiser step consumes
            torch._foreach_copy_(grad_copy, [p.grad for _, p in with_grad])
        opt.step()
        opt.zero_grad(set_to_none=False)

    def fence():
        torch.cuda.synchronize()
        if world > 1 or force_shard:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(k, keep=False):
        # the caller holds no loss / autograd graph at this point: both pooled activation workspaces are free, the loop
        # alternates between them exactly as the warm-up did (a third one would be an 11 GB hipMalloc inside the region)
        loss = None
        fence()
        t0 = time.perf_counter()
        for j in range(k):
            loss = step(keep and j == k - 1)
        epoch_end(keep)
        fence()
        return time.perf_counter() - t0, loss

    loss = None
    for _ in range(max(args.warmup, 2)):   # never fewer than two untimed steps: each creates one of the two workspaces
        loss = step()         # keep the previous step's graph alive exactly as the timed loop does, so that both
                              # activation workspaces exist before timing starts (an 11 GB hipMalloc can take 0.3 s)
    epoch_end()
    fence()
    alloc0 = torch.cuda.memory_stats().get("num_device_alloc", 0)
    profile = args.full and not args.no_profile
    loss = None
    if dump:                                  # (the reference's unused attention parameters never receive a gradient)
        with_grad = [(n, p) for n, p in model.named_parameters() if p.grad is not None]
        grad_copy = [torch.empty_like(p.grad) for _, p in with_grad]
    if pipe is not None:
        pipe.timed = True
    # the headline: K steps WITHOUT per-stage events (they cost ~1.5 % of a step); the stage durations come from a second pass of the
    # same K steps with the library's events on (regt_profile_*), timed too and reported as `ms_per_step_with_stage_events`
    dt, loss = timed(args.steps, keep=dump)
    if pipe is not None:
        pipe.timed = False
    allocs_timed = torch.cuda.memory_stats().get("num_device_alloc", 0) - alloc0
    if dump:
        outs = {"pred": last["pred"], "hidden": last["hidden"], "loss": loss}
        outs.update({"grad." + n: g for (n, _), g in zip(with_grad, grad_copy)})
        outs.update({"param." + n: p for n, p in model.named_parameters()})
        dump_outputs(args.dump_outputs, outs)
        outs, grad_copy = None, []
        last.clear()
    stages = {}
    dt_profiled = None
    if profile:
        loss = None
        lib.regt_profile_enable(1)
        dt_profiled, loss = timed(args.steps)
        lib.regt_profile_enable(0)
        buf = (ctypes.c_char * 16384)()
        _lib.check(lib.regt_profile_collect(buf, 16384), "regt_profile_collect")
        for line in buf.value.decode().splitlines():
            name, cnt, ms = line.split()
            stages[name] = (int(cnt), float(ms))
    final_loss = float(loss.detach())
    loss = None
    # Secondary, opt-in arithmetics (never the headline): the same K steps in the other GEMM modes.  N = 1 only, after the
    # timed region.
    other_modes = {}
    if args.full and world == 1 and not args.no_split_leg and not force_shard and not rows_bf16:     # (bf16 input rows exist in mode 2 only)
        for m2 in (1, 2):
            if m2 == mode:
                continue
            lib.regt_set_gemm_mode(m2)
            l2 = None
            for _ in range(max(args.warmup, 1)):
                l2 = step()
            epoch_end()
            l2 = None
            d2, l2 = timed(args.steps)
            l2 = None
            other_modes[m2] = d2
        lib.regt_set_gemm_mode(mode)
    tpims = None
    if args.full and world == 1 and not args.no_tpims_leg and args.workload == "cfg3":
        lib.regt_set_gemm_mode(0)
        tpims = tpims_leg(dev, with_cpu=not args.no_cpu_baseline)
        lib.regt_set_gemm_mode(mode)
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
    if world > 1 or force_shard:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())

    if rank == 0:
        M = n_local * T
        if shard_of_8:
            wdesc = (f"cfg5shard: rank 0's share of BASELINE configs[4] (global {gnodes} nodes / {gedges} edges / {gregions} regions over 8 GPUs): "
                     f"{n_local} own nodes + {shard.topo.halo_rows} halo rows (random data, no communication), regions "
                     f"{graph.region_lo}..{graph.region_hi} of {gregions}")
        elif weak:
            wdesc = f"{args.workload}: synthetic regional graph, {nodes} nodes / {edges} edges / {regions} regions PER GPU (weak scaling: global graph {world} x that)"
        else:
            wdesc = (f"{args.workload}: ONE synthetic regional graph, {gnodes} nodes / {gedges} edges / {gregions} regions"
                     + (f", split by regions over {world} GPUs ({rpg} region{'s' if rpg > 1 else ''} per GPU)" if world > 1 else ""))
        out = {
            "metric": "training steps/sec (graph-snapshots/sec)", "value": (world if weak else 1) * args.steps / dt, "unit": "snapshots/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": dtype,
            "data": "synthetic",
            "config": {"workload": wdesc + f", F={F}, T={T}, O={O}, hidden=256; RegionalTemporalGCN forward+MSE+backward per "
                                   "snapshot, RMSprop step once per K steps (run.py semantics)",
                       "gemm_arithmetic": MODE_NAMES[mode],
                       "global_nodes": gnodes, "global_edges": gedges, "global_regions": gregions,
                       "parallelism": "single GPU" if world == 1 else f"region-sharded x{world}: halo-row all-to-all per step (one step ahead, side stream) + 1 grad all-reduce",
                       "final_loss": final_loss,
                       "peak_memory_gb": torch.cuda.max_memory_allocated(dev) / 1e9,
                       "ms_per_step_with_stage_events": None if dt_profiled is None else 1e3 * dt_profiled / args.steps,
                       "device_allocs_in_timed_region": allocs_timed},
        }
        if world > 1 or force_shard:
            # what a SCALE record can be checked against: the group as the collective library sees it, this rank's halo
            # rows / bytes per step, pack + exchange on the side stream (off the critical path), the gradient all-reduce
            esz = 2 if rows_bf16 else 4
            mg = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "rank0_own_nodes": n_local,
                  "rank0_halo_rows": int(shard.topo.halo_rows), "rank0_halo_bytes_per_step": int(shard.topo.halo_rows) * T * F * esz,
                  "grad_allreduce_bytes": int(sum(p.numel() for p in params) * 4)}
            if pipe is not None:
                mg["pack_and_exchange_side_stream"] = pipe.exchange_ms()
            if ar_events:
                torch.cuda.synchronize()
                ms = [a.elapsed_time(b) for a, b in ar_events]
                mg["grad_allreduce_ms"] = {"last": ms[-1], "max": max(ms), "calls": len(ms)}
            out["multi_gpu"] = mg
        if stages:
            per = {}
            gen = mode == 0 and "cell_bwd" not in stages      # fp32: cell_bwd folded into the candidate data gradient (round 4)
            for k, (c, ms) in stages.items():
                e = {"launches": c, "avg_ms": ms / c}
                if stage_flops(k, M, C, F):
                    e["tflops"] = stage_flops(k, M, C, F) / (ms / c * 1e-3) / 1e12
                if stage_bytes(k, M, C, F, mode, rows_bf16, gen):
                    e["algorithmic_gbs"] = stage_bytes(k, M, C, F, mode, rows_bf16, gen) / (ms / c * 1e-3) / 1e9
                per[k] = e
            mfma = [(ms, k) for k, (c, ms) in stages.items() if stage_flops(k, M, C, F)]
            tot_ms, dom = max(mfma)
            cnt = stages[dom][0]
            avg_s = tot_ms / cnt * 1e-3
            fl, by = stage_flops(dom, M, C, F), stage_bytes(dom, M, C, F, mode, rows_bf16, gen)
            tflops, gbs = fl / avg_s / 1e12, by / avg_s / 1e9
            traffic, src = pmc_traffic(args.workload, mode, dom)
            mfma_peak = PEAK_FP32_MATRIX_TFLOPS if mode == 0 else PEAK_BF16_MATRIX_TFLOPS
            r_mfma = {"kernel": dom, "bound": "mfma", "achieved": tflops, "peak": mfma_peak, "unit": "TFLOP/s",
                      "frac": tflops / mfma_peak, "traffic": traffic, "traffic_source": src, "avg_ms": avg_s * 1e3,
                      "flops_per_launch": fl}
            r_hbm = {"kernel": dom, "bound": "hbm", "achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                     "frac": gbs / PEAK_HBM_GBS, "traffic": traffic, "traffic_source": src, "avg_ms": avg_s * 1e3,
                     "bytes_per_launch": by}
            if mode == 1:
                r_mfma["note"] = ("fp32-equivalent FLOP/s of the exact 3-way split against the bf16 dense peak: the matrix pipe "
                                  "executes 6 bf16 products per fp32 product, so the ceiling of this arithmetic is peak / 6")
            # the bound that binds: the larger fraction of its own roof (fp32 MFMA GEMMs sit at the matrix pipe; the bf16 ones
            # at HBM, with the M x C activations stored as bf16 -- stage_bytes counts 2 bytes for them)
            if r_mfma["frac"] >= r_hbm["frac"]:
                out["roofline"], out["roofline_other_bound"] = r_mfma, r_hbm
            else:
                out["roofline"], out["roofline_other_bound"] = r_hbm, r_mfma
            if "spmm" in stages:
                c, ms = stages["spmm"]
                W = T * F
                dual = graph.m_rowptr is not None and W % 32 == 0
                nnz = int(graph.m_col.numel()) if dual else int(graph.col.numel())
                x_rows = n_local if shard is None else shard.topo.x_rows
                # read X once + CSR entries (col + 1 or 2 weights) + rowptr + write both outputs (2-byte elements in the bf16-row layout)
                eb = 2 if (rows_bf16 and dual and W % 64 == 0) else 4
                algo = x_rows * W * eb + nnz * (12 if dual else 8) + (n_local + 1) * 4 * (1 if dual else 2) + 2 * n_local * W * eb
                gbs = algo / (ms / c * 1e-3) / 1e9
                tr, src2 = pmc_traffic(args.workload, mode, "spmm") if dual else (None, None)
                out["roofline_spmm"] = {"kernel": "spmm_dual_panel (A_hat x and L~ x in one gather pass, width T*F)" if dual else "spmm_csr (stacked [A_hat; L~] x, width T*F)", "bound": "hbm", "achieved": gbs,
                                        "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS,
                                        "traffic": tr, "traffic_source": src2, "avg_ms": ms / c, "bytes_per_launch": algo}
            gemm_ms = sum(ms for k, (c, ms) in stages.items() if stage_flops(k, M, C, F))
            gemm_fl = sum(stage_flops(k, M, C, F) * c for k, (c, ms) in stages.items() if stage_flops(k, M, C, F))
            out["mfma_all_gemms"] = {"achieved": gemm_fl / (gemm_ms * 1e-3) / 1e12, "peak": mfma_peak,
                                     "unit": "TFLOP/s", "share_of_step": gemm_ms / ((dt_profiled or dt) * 1e3)}
            out["stages"] = per
        for m2, d2 in other_modes.items():
            key = {1: "opt_in_bf16x3_split", 2: "opt_in_bf16", 0: "fp32"}[m2]
            out[key] = {"value": args.steps / d2, "unit": "snapshots/s", "ms_per_step": 1e3 * d2 / args.steps,
                        "note": f"same workload with regt_set_gemm_mode({m2}): {MODE_NAMES[m2]}; NOT the headline value"
                                + ("; passes the same 1e-5 parity suite" if m2 == 1 else "; reduced precision, tolerance in tests/test_gpu_bf16.py")}
        if tpims is not None:
            out["tpims_configs1"] = tpims
        if args.full and world == 1 and args.workload == "cfg3" and not args.no_cfg5_leg and not force_shard:
            out["cfg5shard_configs4"] = cfg5shard_leg(args)
            out["cfg5full_configs4_one_gpu"] = cfg5full_leg(args)
        if args.full and world == 1 and not args.no_cpu_baseline:
            if shard_of_8:
                # the reference formulation materialises an (N, R*C) concat: 8.2 GB per period at 125k nodes x 64 regions, so
                # the bounded sample is ONE of the rank's 8 regions (its nodes and intra-region edges) with the 64-region model
                out["cpu_baseline"] = cpu_baseline(nodes // regions, edges // regions, 1, F, T, O, model_regions=gregions,
                                                   scale_regions=regions,
                                                   note=f" = 1 of the rank's {regions} regions, {gregions}-region model")
            else:
                out["cpu_baseline"] = cpu_baseline(nodes, edges, regions, F, T, O)
            out["cpu_baseline"]["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
        print(json.dumps(out))
    if world > 1 or force_shard:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
