"""Golden vectors of the reference's StackedGRU (models/StackedGRU.py), run unmodified on the TPIMS fixture.

    python tools/make_gru_goldens.py

Needs the reference tree (oracle/make_goldens.py: REF); writes tests/golden/golden_gru_in6_out1.npz and golden_gru_in12_out3.npz.
The model is built as run.py:124 builds it (StackedGRU(in_channels=T, node_features=8, periods=T, output_dim=O)) and fed run.py's
input, ``batch.x`` (N, 8, T): the sequence runs over the 104 nodes.  Parameters plus gradients in full would be 2.5 MB, so each
file holds
  * ``seed``: the parameters are the seeded construction rounded to bf16 (tests/gru_math.py: build_params rebuilds them with
    torch.nn.GRU / torch.nn.Linear in the reference's order);
  * ``p__<name>``: the small tensors in full; for the three large matrices (both weight_hh, linear1.weight) ``p__<name>__s`` (every
    61st element, fp32), ``__rs`` / ``__cs`` (float64 row and column sums): enough to prove the rebuild;
  * ``x`` (N, 8, T), ``y`` (N, O): window ``window`` of tpims_fixture.npz;
  * ``train__out`` / ``train__loss`` / ``train__g__<name>`` (large ones sampled the same way): one training-mode forward / backward
    with run.py's loss mean((out[:, -1, :] - y)**2);
  * ``eval__out`` and run.py::test()'s and predict.py's metrics of an eval-mode forward;
  * ``traj__loss`` (3,), ``traj__dp__<name>``: windows window..window+2 accumulated as run.py::train() does, then one
    RMSprop(lr=1e-3, weight_decay=1e-4) step; the parameter steps stored like the gradients.
It prints, per tensor, the gap between tests/gru_math.py in float64 and the recorded fp32 values relative to the tensor's largest
magnitude, and the same gap of torch.nn.GRU in fp32 for the layer shape classes of tests/test_gpu_gru.py: the per-tensor constants
OUT_GAP, GRAD_GAP and LAYER_GAP of tests/gru_math.py.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

from oracle.make_goldens import OUT, REF, fixture  # noqa: E402
from gru_math import KEYS, LARGE, build_params, gru_layer, sample, stacked_gru  # noqa: E402


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_stacked_gru", os.path.join(REF, "models", "StackedGRU.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.StackedGRU


def window(fx, t_in, t_out, w):
    x = fx["node_data"][:, :, w:w + t_in].contiguous()                         # batch.x (N, 8, T)
    y = fx["node_data"][:, -1, w + t_in:w + t_in + t_out].contiguous()
    return x, y


def store(out, key, t):
    t = t.detach()
    if key.split("__")[-1] in LARGE:
        s, rs, cs = sample(t)
        out[key + "__s"], out[key + "__rs"], out[key + "__cs"] = s.numpy(), rs.numpy(), cs.numpy()
    else:
        out[key] = t.numpy().copy()


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def golden(SG, fx, t_in, t_out, seed, tag, w=0):
    n = fx["node_data"].shape[0]
    torch.manual_seed(seed)
    mod = SG(in_channels=t_in, node_features=8, periods=t_in, output_dim=t_out)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(p.to(torch.bfloat16).to(torch.float32))
    init = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    assert list(init) == KEYS
    rebuilt = build_params(seed, t_in, t_out)
    assert all(torch.equal(init[k], rebuilt[k]) for k in KEYS), "the rebuild does not reproduce the reference's construction"
    x, y = window(fx, t_in, t_out, w)
    out = {"t_in": t_in, "t_out": t_out, "seed": seed, "window": w, "nodes": n, "x": x.numpy(), "y": y.numpy()}
    for k in KEYS:
        store(out, f"p__{k}", init[k])

    mod.train()
    mod.zero_grad()
    o = mod(x, None)
    loss = torch.mean((o[:, -1, :] - y) ** 2)                        # run.py:176
    loss.backward()
    out["train__out"], out["train__loss"] = o.detach().numpy(), np.array([loss.item()])
    grads = {k: p.grad.clone() for k, p in mod.named_parameters()}
    for k in KEYS:
        store(out, f"train__g__{k}", grads[k])

    mod.eval()
    with torch.no_grad():
        o_e = mod(x, None)
    out["eval__out"] = o_e.numpy()
    last = o_e[:, -1, :]
    out["eval__test_mse"] = np.array([((last - y) ** 2).mean().item()])              # run.py:210-212
    err = (y - last).numpy()                                                         # predict.py:155-162
    out["eval__mae"], out["eval__mse"] = np.array([np.abs(err).mean()]), np.array([(err ** 2).mean()])
    out["eval__mape"] = np.array([(np.abs(err) / np.percentile(y.numpy(), q=95)).mean() * 100])

    mod.train()
    opt = torch.optim.RMSprop(mod.parameters(), lr=1e-3, weight_decay=1e-4)
    opt.zero_grad()
    losses = []
    for k in range(3):
        xk, yk = window(fx, t_in, t_out, w + k)
        lk = torch.mean((mod(xk, None)[:, -1, :] - yk) ** 2)
        lk.backward()
        losses.append(lk.item())
    opt.step()
    out["traj__loss"] = np.array(losses)
    steps = {k: p.detach() - init[k] for k, p in mod.named_parameters()}
    for k in KEYS:
        store(out, f"traj__dp__{k}", steps[k])
    path = os.path.join(OUT, f"golden_gru_{tag}.npz")
    np.savez_compressed(path, **out)

    # the float64 restatement against what was just recorded: the fp32-vs-float64 gap of the reference itself
    p64 = {k: v.double().requires_grad_(True) for k, v in init.items()}
    o64 = stacked_gru(p64, x)
    torch.mean((o64[:, -1, :] - y.double()) ** 2).backward()
    print(f"{tag}: {os.path.getsize(path)} bytes, loss {loss.item():.6g}, max |out| {float(o.abs().max()):.3g}")
    print(f"  out gap {rel(o.detach(), o64.detach()):.2e}")
    for k in KEYS:
        print(f"  grad {k:22s} max {float(grads[k].abs().max()):.3g} gap {rel(grads[k], p64[k].grad):.2e}")


def layer_gap(seq, rows, t, seed):
    """torch.nn.GRU in fp32 against the restatement in float64 for one layer with h0, dout on all rows and dh_last."""
    torch.manual_seed(seed)
    g = torch.nn.GRU(t, 256)
    x, h0 = torch.randn(seq, rows, t), (torch.randn(1, rows, 256) * 0.5).requires_grad_(True)
    dout, dlast = torch.randn(seq, rows, 256), torch.randn(1, rows, 256)
    o, l = g(x, h0)
    ((o * dout).sum() + (l * dlast).sum()).backward()
    w64 = [q.detach().double().requires_grad_(True) for q in g.parameters()]
    h64 = h0.detach().double().requires_grad_(True)
    o64, l64 = gru_layer(x.double(), *w64, h0=h64)
    ((o64 * dout.double()).sum() + (l64 * dlast[0].double()).sum()).backward()
    gaps = [rel(o.detach(), o64.detach()), rel(l.detach()[0], l64.detach())] + [rel(q.grad, q64.grad) for q, q64 in zip(g.parameters(), w64)] \
        + [rel(h0.grad[0], h64.grad)]
    print(f"layer seq={seq} rows={rows} T={t}: out, h_last, dW_ih, dW_hh, db_ih, db_hh, dh0 gaps " + " ".join(f"{v:.2e}" for v in gaps))


def main():
    torch.set_num_threads(1)            # one summation order: the files are reproducible bit for bit
    SG = load_reference()
    fx = fixture()
    for t_in, t_out, seed in ((6, 1, 41), (12, 3, 42)):
        golden(SG, fx, t_in, t_out, seed, f"in{t_in}_out{t_out}")
    layer_gap(104, 16, 12, 1)
    layer_gap(4096, 8, 12, 2)


if __name__ == "__main__":
    main()
