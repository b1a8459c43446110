#!/usr/bin/env python3
"""Backward times of the STAEformer self-attention layer at run.py's widths (model_dim 128, 4 heads, feed_forward 256, T = 12,
B = 1) for N = 104 and N = 2048, the sibling of tools/staeformer_bench.py: the attention backward per axis (two launches: the query
pass and the key pass), the add+LayerNorm backward, and one nn.SelfAttentionLayer's forward + backward per axis, next to torch-ROCm's
own autograd for the same ops on the same values (scaled_dot_product_attention on (B S, H, L, 32) tensors, once on operands already
laid out that way and once including the permutes from and to the row layout; F.layer_norm on residual + y).  Device events around
`reps` calls, three windows each to show the spread.  Recorded only: no pass bar.  One JSON line.

    python tools/stae_backward_bench.py [big_nodes]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import regtgcn_amd as R
from regtgcn_amd import ops

big = int(sys.argv[1]) if len(sys.argv) >= 2 else 2048
T, B, HEADS, D, FF = 12, 1, 4, 128, 256
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


def three(fn, reps):
    return [round(timed(fn, reps), 4) for _ in range(3)]


def torch_attention_fb(qkv, dout, n, axis, with_layout):
    """torch's forward + backward of the op (its backward cannot run without its forward's graph)."""
    def heads(z):
        z = z.reshape(B, T, n, HEADS, 32)
        z = z.permute(0, 2, 3, 1, 4) if axis == 1 else z.permute(0, 1, 3, 2, 4)                       # (B, S, H, L, 32)
        return z.reshape(-1, HEADS, z.shape[3], 32)
    if with_layout:
        src = qkv.clone().requires_grad_(True)

        def run():
            src.grad = None
            q, k, v = (heads(src[:, i * D:(i + 1) * D]).contiguous() for i in range(3))
            o = torch.nn.functional.scaled_dot_product_attention(q, k, v)
            o = o.reshape(B, -1, HEADS, o.shape[2], 32)
            o = (o.permute(0, 3, 1, 2, 4) if axis == 1 else o.permute(0, 1, 3, 2, 4)).reshape(B * T * n, D)
            o.backward(dout)
        return run
    q, k, v = (heads(qkv[:, i * D:(i + 1) * D]).contiguous().requires_grad_(True) for i in range(3))
    do = heads(dout).contiguous()

    def run():
        q.grad = k.grad = v.grad = None
        torch.nn.functional.scaled_dot_product_attention(q, k, v).backward(do)
    return run


def run(n, reps):
    torch.manual_seed(42)
    m = B * T * n
    res = {"nodes": n, "rows": m, "reps": reps}
    qkv, dout = torch.randn(m, 3 * D, device=dev), torch.randn(m, D, device=dev)
    q, k, v = (qkv[:, i * D:(i + 1) * D] for i in range(3))
    grads = torch.empty(m, 3 * D, device=dev)
    for axis, name in ((1, "temporal"), (2, "spatial")):
        out, lse = ops.stae_attention_train(q, k, v, B, T, n, HEADS, axis)
        length, seqs = (T, B * n) if axis == 1 else (n, B * T)
        res[f"attention_{name}"] = {
            "L": length, "sequences": seqs,
            "hip_forward_train_ms": three(lambda: ops.stae_attention_train(q, k, v, B, T, n, HEADS, axis, out=out), reps),
            "hip_forward_inference_ms": three(lambda: ops.stae_attention(q, k, v, B, T, n, HEADS, axis, out=out), reps),
            "hip_backward_ms": three(lambda: ops.stae_attention_backward(q, k, v, out, dout, lse, B, T, n, HEADS, axis, grads=grads), reps),
            # dense 32 x 32 tiles on the matrix unit: five products per pass pair (S, dP, dQ | S, dP, dV, dK = 7) against the forward's 2
            "backward_mfma_flop": 7 * 2 * seqs * HEADS * (-(-length // 32) * 32) ** 2 * 32,
            "torch_sdpa_forward_backward_ms": three(torch_attention_fb(qkv, dout, n, axis, False), reps),
            "torch_sdpa_forward_backward_with_layout_ms": three(torch_attention_fb(qkv, dout, n, axis, True), reps)}
    res_t, y, gamma, beta = (torch.randn(m, D, device=dev), torch.randn(m, D, device=dev), torch.rand(D, device=dev) + 0.5,
                             torch.randn(D, device=dev))
    zr, gr, br = (res_t + y).requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)

    def torch_ln():
        zr.grad = gr.grad = br.grad = None
        torch.nn.functional.layer_norm(zr, (D,), gr, br, 1e-5).backward(dout)

    res["add_layernorm"] = {"hip_forward_ms": three(lambda: ops.stae_add_layernorm(res_t, y, gamma, beta), reps),
                            "hip_backward_ms": three(lambda: ops.stae_add_layernorm_backward(res_t, y, gamma, dout), reps),
                            "torch_layer_norm_forward_backward_ms": three(torch_ln, reps)}
    layer = R.SelfAttentionLayer(D, feed_forward_dim=FF, num_heads=HEADS, dropout=0).to(dev)
    x = torch.randn(B, T, n, D, device=dev, requires_grad=True)
    dx = dout.view(B, T, n, D)
    for axis, name in ((1, "temporal"), (2, "spatial")):
        def fb():
            layer.zero_grad(set_to_none=True)
            x.grad = None
            layer(x, dim=axis).backward(dx)

        def fwd():
            with torch.no_grad():
                layer(x, dim=axis)
        res[f"layer_{name}"] = {"forward_ms": three(fwd, reps), "forward_backward_ms": three(fb, reps)}
    return res


print(json.dumps({"shape": {"T": T, "B": B, "model_dim": D, "heads": HEADS, "feed_forward": FF}, "device": torch.cuda.get_device_name(0),
                  "runs": [run(104, 200), run(big, 50)]}))
