#!/usr/bin/env python3
"""SpatialGCN training-step time on a synthetic graph, and the times of its first-layer kernel pair
(regt_spatial_embed_forward / _backward) with their fraction of 8 TB/s on algorithmic bytes (x, L~x, keep mask, S or dS).

    python tools/spatial_bench.py [nodes edges F T]        (default: 100000 1000000 32 12 = cfg-3 shape)
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import regtgcn_amd as R

nodes, edges, F, T = (int(v) for v in sys.argv[1:5]) if len(sys.argv) >= 5 else (100_000, 1_000_000, 32, 12)
HBM = 8.0e12
dev = torch.device("cuda")
R.load_library()
g = R.data.synthetic_regional_graph(nodes, edges, 8, seed=42)
torch.manual_seed(42)
model = R.SpatialGCN(F, T, 1).to(dev).train()
op = model.prepare_graph(g.edge_index.to(dev), g.edge_attr.to(dev), nodes)
snaps = [(x.to(dev), y.to(dev)) for x, y in R.data.synthetic_snapshots(nodes, F, T, 1, 2, seed=42)]
opt = torch.optim.RMSprop(model.parameters(), lr=1e-3, weight_decay=1e-4)


def step(i):
    x, y = snaps[i % 2]
    pred, _ = model.forward_prepared(x, op)
    loss = torch.mean((pred - y) ** 2)
    loss.backward()
    return loss


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for i in range(3):
    step(i)
opt.step(); opt.zero_grad(set_to_none=False)
torch.cuda.synchronize()
K = 10
t0 = time.perf_counter()
for i in range(K):
    step(i)
opt.step(); opt.zero_grad(set_to_none=False)
torch.cuda.synchronize()
step_ms = (time.perf_counter() - t0) * 1e3 / K

# the kernel pair on its own, on the model's inputs
x = snaps[0][0]
xp = R.ops.pack_x(x)
lxp = R.ops.spmm_csr(op.rowptr, op.col, op.val, xp.view(nodes, T * F)).view(nodes, T, F)
w0, w1, b = (p.detach().contiguous() for p in (model.gcn.lins[0].weight, model.gcn.lins[1].weight, model.gcn.bias))
keep = R.nn.draw_keep_mask(nodes * T, dev)
ds = torch.randn(nodes, 64, device=dev)
for _ in range(3):
    R.ops.spatial_embed_forward(xp, lxp, w0, w1, b, keep)
    R.ops.spatial_embed_backward(xp, lxp, w0, w1, b, keep, ds)
reps = 50
fwd_ms = timed(lambda i: R.ops.spatial_embed_forward(xp, lxp, w0, w1, b, keep), reps)
bwd_ms = timed(lambda i: R.ops.spatial_embed_backward(xp, lxp, w0, w1, b, keep, ds), reps)
M = nodes * T
alg_bytes = 2 * M * F * 4 + M * 8 + nodes * 64 * 4           # x, L~x, keep mask, S (forward) or dS (backward)
flops_fwd = 2.0 * M * 64 * 2 * F
res = {"shape": {"nodes": nodes, "edges": edges, "F": F, "T": T}, "train_step_ms": round(step_ms, 4),
       "embed_fwd_ms": round(fwd_ms, 4), "embed_bwd_ms": round(bwd_ms, 4), "alg_bytes_mb": round(alg_bytes / 1e6, 1),
       "embed_fwd_hbm_frac": round(alg_bytes / (fwd_ms * 1e-3) / HBM, 3), "embed_bwd_hbm_frac": round(alg_bytes / (bwd_ms * 1e-3) / HBM, 3),
       "embed_fwd_tflops": round(flops_fwd / (fwd_ms * 1e-3) / 1e12, 1), "embed_bwd_tflops": round(2 * flops_fwd / (bwd_ms * 1e-3) / 1e12, 1)}
print(json.dumps(res))
