#!/usr/bin/env python3
"""STNorm forward, backward and training-step times at the cfg-3 shape (B = 1, T = 12, N = 100 000 nodes, F = 32, O = 1), with
the algorithmic bytes and flops of the forward.  One JSON line.

    python tools/stnorm_bench.py [nodes F T]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import regtgcn_amd as R

nodes, F, T = (int(v) for v in sys.argv[1:4]) if len(sys.argv) >= 4 else (100_000, 32, 12)
HBM, FP32 = 8.0e12, 157.3e12          # MI355X peak HBM bandwidth, fp32 vector FMA rate
dev = torch.device("cuda")
R.load_library()
torch.manual_seed(42)
model = R.STNorm(num_nodes=nodes, in_dim=F, out_dim=1).to(dev).train()
x = torch.randn(1, T, nodes, F, device=dev)
y = torch.randn(nodes, 1, device=dev)
opt = torch.optim.RMSprop(model.parameters(), lr=1e-3, weight_decay=1e-4)
params = [None if p is None else p.detach() for p in model.param_table()]
running = model.running_table()
dims = R.ops.stnorm_dims(nodes, 1, 1, T, F, 1, model.blocks, model.layers, True, True, True)


def timed(fn, reps):
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def step(i):
    loss = torch.mean((model(x) - y) ** 2)
    loss.backward()
    opt.step()
    opt.zero_grad()


out, ws = R.ops.stnorm_forward(dims, x, params, running)
dout = torch.randn_like(out)
fwd_ms = timed(lambda i: R.ops.stnorm_forward(dims, x, params, running), 20)
bwd_ms = timed(lambda i: R.ops.stnorm_backward(dims, x, params, running, dout, ws), 10)
step_ms = timed(step, 10)

# forward, algorithmic: input once, every layer reads its input twice (TNorm statistics, then the convolutions) and writes its output,
# TNorm gamma / beta / running buffers read and written; flops: the two dilated convolutions, residual and skip per output column
rf = model.receptive_field
L = [max(T, rf)]
for i in range(model.blocks * model.layers):
    L.append(L[-1] - (1 << (i % model.layers)))
col = 16 * nodes * 4
fwd_bytes = T * nodes * F * 4 + L[0] * col + sum(2 * L[i] * col + L[i + 1] * col for i in range(len(L) - 1)) + 8 * 6 * 16 * nodes * 4
fwd_flops = 2.0 * nodes * (L[0] * 16 * F + sum(L[i + 1] * (2 * 16 * 96 + 2 * 16 * 16) for i in range(len(L) - 1)))
res = {"shape": {"nodes": nodes, "F": F, "T": T, "B": 1}, "fwd_ms": round(fwd_ms, 4), "bwd_ms": round(bwd_ms, 4),
       "train_step_ms": round(step_ms, 4), "fwd_alg_mb": round(fwd_bytes / 1e6, 1), "fwd_gflop": round(fwd_flops / 1e9, 2),
       "fwd_hbm_frac": round(fwd_bytes / (fwd_ms * 1e-3) / HBM, 3), "fwd_fp32_frac": round(fwd_flops / (fwd_ms * 1e-3) / FP32, 3)}
print(json.dumps(res))
