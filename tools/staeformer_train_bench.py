"""Whole-STAEformer training at run.py's construction (tod_embedding_dim=0: model_dim 128, 4 heads, dropout 0.1), T = 12:

    python tools/staeformer_train_bench.py [--step] [nodes batch]      (default: N = 104, B = 64 and N = 4096, B = 1)

Per shape: the keep-bit add+LayerNorm forward / backward next to the plain kernels in the same run (expected by bytes: forward about
1 + 1/32 of the plain one, backward about 5/4), the embedding and output-projection gradients with their achieved bytes/s against the
byte floors of DESIGN.md 3k, one layer's spatial attention backward as the yardstick of the two reductions, and one training step
(forward + backward, num_layers = 3) next to the inference forward.  Times are medians of 20 calls after 5 warm-up calls, each call
timed with device events around it; the four new pieces and the plain add+LayerNorm kernels are called through the raw C entries on
buffers allocated once, so no Python wrapper or allocation is inside a timed call.  ``--step nodes batch`` runs four training steps
and nothing else: the program for ``rocprofv3 --kernel-trace --stats`` (its table is per kernel over the four steps).  """
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import regtgcn_amd as R  # noqa: E402
from regtgcn_amd import ops  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts)


def shape(n, b, t=12, o=1, layers=3):
    torch.manual_seed(0)
    model = R.STAEformerTrainable(num_nodes=n, in_steps=t, out_steps=o, tod_embedding_dim=0, num_layers=layers).to(DEV)
    d, m = model.model_dim, b * t * n
    x = torch.rand(b, t, n, 8, device=DEV)
    x[..., 2] = torch.randint(0, 7, (b, t, n), device=DEV).float()
    dims = model.dims(b, 8)
    res, y, dout = (torch.randn(m, d, device=DEV) for _ in range(3))
    gamma, beta = torch.ones(d, device=DEV), torch.zeros(d, device=DEV)
    keep = R.nn.draw_stae_keep(1, m, d, DEV, 0.1)[0].contiguous()
    print(f"\nN = {n}, T = {t}, B = {b}: M = {m} rows of {d} floats")
    # the raw entries on buffers allocated once: no Python wrapper, no allocation inside the timed call
    lib, P, st = R.load_library(), R._lib.ptr, torch.cuda.current_stream().cuda_stream
    out, dz, dy = (torch.empty(m, d, device=DEV) for _ in range(3))
    dg, db = torch.empty(d, device=DEV), torch.empty(d, device=DEV)
    sc = torch.empty(lib.regt_stae_drop_add_layernorm_backward_scratch_floats(m, d), device=DEV)
    f0 = timed(lambda: lib.regt_stae_add_layernorm(P(res), P(y), P(gamma), P(beta), 1e-5, m, d, P(out), st))
    f1 = timed(lambda: lib.regt_stae_drop_add_layernorm(P(res), P(y), P(keep), 0.1, P(gamma), P(beta), 1e-5, m, d, P(out), st))
    b0 = timed(lambda: lib.regt_stae_add_layernorm_backward(P(res), P(y), P(gamma), P(dout), 1e-5, m, d, P(dz), P(dg), P(db), P(sc), st))
    b1 = timed(lambda: lib.regt_stae_drop_add_layernorm_backward(P(res), P(y), P(keep), 0.1, P(gamma), P(dout), 1e-5, m, d, P(dz), P(dy), P(dg),
                                                                 P(db), P(sc), st))
    fl = lambda k: 4.0 * k * m * d
    print(f"  add+LayerNorm forward   plain {f0 * 1e6:8.1f} us ({fl(3) / f0 / 1e12:.2f} TB/s)   keep-bit {f1 * 1e6:8.1f} us "
          f"({fl(3 + 1 / 32) / f1 / 1e12:.2f} TB/s)   ratio {f1 / f0:.3f} (by bytes 1.010; one array's 1/32: 1.031)")
    print(f"  add+LayerNorm backward  plain {b0 * 1e6:8.1f} us ({fl(4) / b0 / 1e12:.2f} TB/s)   keep-bit {b1 * 1e6:8.1f} us "
          f"({fl(5 + 1 / 32) / b1 / 1e12:.2f} TB/s)   ratio {b1 / b0:.3f} (by bytes 1.258)   [two launches each: rows, then the column sums]")
    rows = model.param_table()
    byref = __import__("ctypes").byref
    grads = [None if p_ is None else torch.empty_like(p_) for p_ in rows[:6]]
    gt = ops._ptr_table(grads)
    esc = torch.empty(lib.regt_stae_embed_backward_scratch_floats(byref(dims)), device=DEV)
    te = timed(lambda: lib.regt_stae_embed_backward(byref(dims), P(x), P(dout), gt, P(esc), st))
    h = torch.randn(m, d, device=DEV)
    go = torch.randn(b, o, n, 1, device=DEV)
    dw, dbo = torch.empty_like(rows[6]), torch.empty_like(rows[7])
    psc = torch.empty(lib.regt_stae_output_proj_backward_scratch_floats(byref(dims)), device=DEV)
    tp = timed(lambda: lib.regt_stae_output_proj_backward(byref(dims), P(h), P(rows[6]), P(go), *go.stride(), P(dz), P(dw), P(dbo), P(psc), st))
    print(f"  embedding backward      {te * 1e6:8.1f} us: floor {4.0 * m * (8 + d) / 1e6:.1f} MB -> {4.0 * m * (8 + d) / te / 1e12:.2f} TB/s   [three launches]")
    print(f"  output proj backward    {tp * 1e6:8.1f} us: floor {(fl(2) + 8.0 * o * t * d) / 1e6:.1f} MB -> {(fl(2) + 8.0 * o * t * d) / tp / 1e12:.2f} TB/s   [two launches]")
    qkv = torch.randn(m, 3 * d, device=DEV)
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    ao, lse = ops.stae_attention_train(q, k, v, b, t, n, 4, 2)
    ta = timed(lambda: ops.stae_attention_backward(q, k, v, ao, dout, lse, b, t, n, 4, 2))
    print(f"  spatial attention backward (one layer) {ta * 1e6:8.1f} us; the two reductions together {(te + tp) * 1e6:8.1f} us "
          f"({'within' if te + tp <= ta else 'ABOVE'} it)")
    model.eval()
    with torch.no_grad():
        ti = timed(lambda: model(x))
    model.train()

    def step():
        model.zero_grad(set_to_none=True)
        model(x).square().mean().backward()
    ts = timed(step)
    print(f"  inference forward {ti * 1e3:8.3f} ms   training step (forward + backward, dropout 0.1, fresh keep bits) {ts * 1e3:8.3f} ms")


def one_step(n, b, t=12, layers=3):
    """Three warm-up steps and ONE more training step: the program to put under ``rocprofv3 --kernel-trace --stats``."""
    torch.manual_seed(0)
    model = R.STAEformerTrainable(num_nodes=n, in_steps=t, out_steps=1, tod_embedding_dim=0, num_layers=layers).to(DEV).train()
    x = torch.rand(b, t, n, 8, device=DEV)
    for _ in range(4):
        model.zero_grad(set_to_none=True)
        model(x).square().mean().backward()
    torch.cuda.synchronize()
    print(f"4 training steps at N = {n}, B = {b}, T = {t}")


def main():
    args = [a for a in sys.argv[1:] if a != "--step"]
    shapes = [(int(args[0]), int(args[1]))] if len(args) > 1 else [(104, 64), (4096, 1)]
    if "--step" in sys.argv:
        return one_step(*shapes[0])
    print(torch.cuda.get_device_name(0))
    for n, b in shapes:
        shape(n, b)


if __name__ == "__main__":
    main()
