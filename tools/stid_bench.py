#!/usr/bin/env python3
"""STID forward, backward and training-step times at the cfg-3 shape (L = 12, N = 100 000 nodes, C = 8, input_dim = 3, O = 1) for
B = 1 and B = 16, with the algorithmic bytes and flops of the forward and, in the same process, the times
of the fp32 restatement tests/stid_math.py run as torch-eager on the GPU with the same keep mask.  One JSON line.

    python tools/stid_bench.py [nodes]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import regtgcn_amd as R
from regtgcn_amd.nn import draw_stid_keep
from stid_math import stid

nodes = int(sys.argv[1]) if len(sys.argv) >= 2 else 100_000
L, C, D, O, NL = 12, 8, 3, 1, 3
HBM, FP32 = 8.0e12, 157.3e12          # MI355X peak HBM bandwidth, fp32 matrix (= vector) rate
dev = torch.device("cuda")
R.load_library()


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(batch):
    torch.manual_seed(42)
    model = R.STID(num_nodes=nodes, input_len=L, output_len=O, input_dim=D, num_layer=NL, if_time_in_day=False,
                   if_day_in_week=False).to(dev).train()
    x = torch.randn(batch, L, nodes, C, device=dev)
    y = torch.randn(batch, nodes, O, device=dev)
    keep = draw_stid_keep(NL, batch, nodes, 64, dev)
    keep_bool = ((keep.unsqueeze(-1) >> torch.arange(32, device=dev, dtype=torch.int32)) & 1).bool().reshape(NL, batch, nodes, 64)
    opt = torch.optim.RMSprop(model.parameters(), lr=1e-3, weight_decay=1e-4)
    params = [p.detach() for p in model.param_table()]
    dims = R.ops.stid_dims(nodes, batch, L, C, D, NL, O)
    eager = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    eopt = torch.optim.RMSprop(list(eager.values()), lr=1e-3, weight_decay=1e-4)

    def loss_of(out):
        return ((out - y.unsqueeze(1)) ** 2).mean(dim=(1, 2, 3)).sum()

    def step():
        loss_of(model(x, keep=keep)).backward()
        opt.step()
        opt.zero_grad()

    def eager_step():
        loss_of(stid(eager, x, D, keep=keep_bool, dtype=torch.float32)).backward()
        eopt.step()
        eopt.zero_grad()

    def eager_fwd():
        with torch.no_grad():
            stid(eager, x, D, dtype=torch.float32)

    out, ws = R.ops.stid_forward(dims, x, params, keep, save=True)
    dout = torch.randn_like(out)
    reps = 50 if batch == 1 else 10
    t = {"fwd_ms": timed(lambda: R.ops.stid_forward(dims, x, params, None, save=False), reps),
         "fwd_train_ms": timed(lambda: R.ops.stid_forward(dims, x, params, keep, save=True), reps),
         "bwd_ms": timed(lambda: R.ops.stid_backward(dims, x, params, keep, dout, ws), reps),
         "train_step_ms": timed(step, reps),
         "eager_fwd_ms": timed(eager_fwd, reps),
         "eager_train_step_ms": timed(eager_step, reps)}
    # forward, algorithmic, per node and snapshot: the L input rows, the node-embedding row, the output; flops: the embedding, the
    # 2 NL hidden x hidden products and the regression
    bn = batch * nodes
    fwd_bytes = bn * (L * C * 4 + 32 * 4 + O * 4)
    fwd_flops = 2.0 * bn * (L * D * 32 + NL * 2 * 64 * 64 + 64 * O)
    ws_bytes = bn * (2 * NL + 1) * 64 * 4
    res = {"B": batch, **{k: round(v, 4) for k, v in t.items()}, "fwd_alg_mb": round(fwd_bytes / 1e6, 1),
           "fwd_gflop": round(fwd_flops / 1e9, 2), "workspace_mb": round(ws_bytes / 1e6, 1),
           "fwd_hbm_frac": round(fwd_bytes / (t["fwd_ms"] * 1e-3) / HBM, 3),
           "fwd_fp32_frac": round(fwd_flops / (t["fwd_ms"] * 1e-3) / FP32, 3),
           "bwd_fp32_frac": round(2 * fwd_flops / (t["bwd_ms"] * 1e-3) / FP32, 3),
           "fwd_faster_than_eager": t["fwd_ms"] < t["eager_fwd_ms"], "step_faster_than_eager": t["train_step_ms"] < t["eager_train_step_ms"]}
    return res


print(json.dumps({"shape": {"nodes": nodes, "L": L, "C": C, "input_dim": D, "O": O, "num_layer": NL}, "runs": [run(1), run(16)]}))
