#!/usr/bin/env python3
"""StackedGRU forward and training-step times and the per-step time of the serial passes of one GRU layer, for N = 104, T = 12 at
B = 1 and B = 64 (8 B batch rows) and for the cfg-3 node count (N = 100 000) at B = 1, each against eager torch.nn.GRU + Linear with
the same parameters in the same process.  The serial pass streams W_hh (768 x 256 fp32) from L2 once per step and workgroup and
spends 2 * 8 * 768 * (256 + T) flops per step on a tile of 8 rows: the fractions of the per-CU L2 bandwidth and of one CU's fp32
rate are reported next to the per-step time.  One JSON line.

    python tools/gru_bench.py [nodes]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import regtgcn_amd as R
from regtgcn_amd import ops

big = int(sys.argv[1]) if len(sys.argv) >= 2 else 100_000
T, O, F = 12, 1, 8
CLK = 2.4e9
CU_FP32 = 256 * CLK                   # one CU: 256 fp32 flop / clk (matrix or packed-FMA vector)
CU_L2 = 64 * CLK                      # one CU's L2 read path: 64 B / clk
dev = torch.device("cuda")
R.load_library()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


class Eager(torch.nn.Module):
    def __init__(self, m):
        super().__init__()
        self.gru, self.gru2 = torch.nn.GRU(T, 256), torch.nn.GRU(T, 256)
        self.linear1, self.linear2 = torch.nn.Linear(256, 256), torch.nn.Linear(256, O)
        self.load_state_dict(m.state_dict())

    def forward(self, x):
        _, h = self.gru(x)
        out, _ = self.gru2(x, h)
        return self.linear2(torch.relu(self.linear1(out)))


def run(nodes, batch, reps):
    torch.manual_seed(42)
    model = R.StackedGRU(T, F, T, O).to(dev).train()
    eager = Eager(model).to(dev).train()
    rows = F * batch
    x = torch.randn(nodes, rows, T, device=dev)
    y = torch.randn(batch, nodes, O, device=dev)
    opt = torch.optim.RMSprop(model.parameters(), lr=1e-3, weight_decay=1e-4)
    eopt = torch.optim.RMSprop(eager.parameters(), lr=1e-3, weight_decay=1e-4)

    def loss_of(out):
        last = out.view(nodes, batch, F, O)[:, :, -1, :].permute(1, 0, 2)
        return ((last - y) ** 2).mean(dim=(1, 2)).sum()

    def step(m, o):
        loss_of(m(x)).backward()
        o.step()
        o.zero_grad()

    def fwd(m):
        with torch.no_grad():
            m(x)

    w = [q.detach() for q in model.gru2.parameters()]
    out, _, dims, ws = ops.gru_forward(x, w, None, True, False, save=True)
    dout = torch.randn_like(out)
    t = {"fwd_ms": timed(lambda: fwd(model), reps), "train_step_ms": timed(lambda: step(model, opt), reps),
         "eager_fwd_ms": timed(lambda: fwd(eager), reps), "eager_train_step_ms": timed(lambda: step(eager, eopt), reps),
         "layer_fwd_ms": timed(lambda: ops.gru_forward(x, w, None, True, False, save=False), reps),
         "layer_fwd_train_ms": timed(lambda: ops.gru_forward(x, w, None, True, False, save=True), reps),
         "layer_bwd_ms": timed(lambda: ops.gru_backward(dims, x, w, dout, None, ws), reps)}
    fwd_us = t["layer_fwd_ms"] * 1e3 / nodes
    tiles = (rows + 7) // 8
    res = {"nodes": nodes, "B": batch, "rows": rows, **{k: round(v, 4) for k, v in t.items()},
           "fwd_step_us": round(fwd_us, 3), "bwd_step_us_incl_wgrad": round(t["layer_bwd_ms"] * 1e3 / nodes, 3),
           "workgroups": tiles, "workspace_mb": round(ops.gru_sizes(dims)[0] * 4 / 1e6, 1),
           "fwd_step_cu_fp32_frac": round(2.0 * 8 * 768 * (256 + T) / (fwd_us * 1e-6) / CU_FP32, 3),
           "fwd_step_cu_l2_frac": round(768 * (256 + T) * 4 / (fwd_us * 1e-6) / CU_L2, 3),
           "fwd_faster_than_eager": t["fwd_ms"] < t["eager_fwd_ms"], "step_faster_than_eager": t["train_step_ms"] < t["eager_train_step_ms"]}
    return res


print(json.dumps({"shape": {"T": T, "O": O, "features": F, "hidden": 256},
                  "runs": [run(104, 1, 20), run(104, 64, 20), run(big, 1, 2)]}))
