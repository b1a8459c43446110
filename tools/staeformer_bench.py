#!/usr/bin/env python3
"""STAEformer inference times at run.py's construction (model_dim 128, 4 heads, 3 + 3 layers, T = 12, O = 1, B = 1) for N = 104 and
N = 2048: the whole forward (device events around `reps` calls, three windows to show the spread), the library's per-stage times
from its own event brackets in a window of its own (the temporal and the spatial attention launches among them), and the attention
entry point alone on the layer's Q|K|V buffer next to torch-ROCm's own math for the same op on the same values:
scaled_dot_product_attention on (B S, H, L, 32) tensors, once on operands already laid out that way and once including the
permutes from and to the row layout that the library reads in place.  Recorded only: no pass bar.  One JSON line.

    python tools/staeformer_bench.py [big_nodes]
"""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import regtgcn_amd as R
from regtgcn_amd import _lib, ops

big = int(sys.argv[1]) if len(sys.argv) >= 2 else 2048
T, O, F, B, HEADS, D = 12, 1, 8, 1, 4, 128
dev = torch.device("cuda")
lib = R.load_library()


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


def stages(fn, reps):
    lib.regt_profile_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    lib.regt_profile_enable(0)
    buf = (ctypes.c_char * 16384)()
    _lib.check(lib.regt_profile_collect(buf, 16384), "regt_profile_collect")
    out = {}
    for line in buf.value.decode().splitlines():
        name, cnt, ms = line.split()
        out[name] = {"launch_groups": int(cnt) // reps, "ms_per_forward": round(float(ms) / reps, 4),
                     "ms_per_launch_group": round(float(ms) / int(cnt), 4)}
    return out


def torch_attention(qkv, n, axis, with_layout):
    """torch's math for the op: heads split, the sequence axis second to last."""
    def heads(z):
        z = z.reshape(B, T, n, HEADS, 32)
        z = z.permute(0, 2, 3, 1, 4) if axis == 1 else z.permute(0, 1, 3, 2, 4)                       # (B, S, H, L, 32)
        return z.reshape(-1, HEADS, z.shape[3], 32).contiguous()
    if with_layout:
        def run():
            q, k, v = (heads(qkv[:, i * D:(i + 1) * D]) for i in range(3))
            o = torch.nn.functional.scaled_dot_product_attention(q, k, v)
            o = o.reshape(B, -1, HEADS, o.shape[2], 32)
            return (o.permute(0, 3, 1, 2, 4) if axis == 1 else o.permute(0, 1, 3, 2, 4)).reshape(B * T * n, D)
        return run
    q, k, v = (heads(qkv[:, i * D:(i + 1) * D]) for i in range(3))
    return lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v)


def run(n, reps):
    torch.manual_seed(42)
    model = R.STAEformer(num_nodes=n, in_steps=T, out_steps=O, tod_embedding_dim=0).to(dev).eval()
    x = torch.randn(B, T, n, F, device=dev)
    x[..., 2] = torch.randint(0, 7, (B, T, n), device=dev).float()

    def fwd():
        with torch.no_grad():
            model(x)

    res = {"nodes": n, "rows": B * T * n, "reps": reps, "forward_ms": [round(timed(fwd, reps), 4) for _ in range(3)],
           "stages": stages(fwd, reps)}
    qkv = torch.randn(B * T * n, 3 * D, device=dev)
    q, k, v = (qkv[:, i * D:(i + 1) * D] for i in range(3))
    out = torch.empty(B * T * n, D, device=dev)
    for axis, name in ((1, "temporal"), (2, "spatial")):
        ours = lambda: ops.stae_attention(q, k, v, B, T, n, HEADS, axis, out=out)
        ref = torch_attention(qkv, n, axis, True)()
        res[f"attention_{name}"] = {
            "L": T if axis == 1 else n, "sequences": B * (n if axis == 1 else T),
            "hip_ms": round(timed(ours, reps), 4),
            "torch_sdpa_ms": round(timed(torch_attention(qkv, n, axis, False), reps), 4),
            "torch_sdpa_with_layout_ms": round(timed(torch_attention(qkv, n, axis, True), reps), 4),
            "max_abs_diff_vs_torch": float((ours() - ref).abs().max())}
    return res


print(json.dumps({"shape": {"T": T, "O": O, "B": B, "features": F, "model_dim": D, "heads": HEADS, "layers": "3 + 3", "feed_forward": 256},
                  "device": torch.cuda.get_device_name(0), "runs": [run(104, 200), run(big, 50)]}))
