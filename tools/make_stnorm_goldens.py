"""Golden vectors of the reference's STNorm (models/STNorm.py), run unmodified on the TPIMS fixture.

    python tools/make_stnorm_goldens.py

Needs the reference tree (oracle/make_goldens.py: REF); writes tests/golden/golden_stnorm_in6_out1.npz and
golden_stnorm_in12_out3.npz.  The model is built as run.py:135 builds it (STNorm(num_nodes=N, in_dim=8, out_dim=O)) and fed
run.py's input, ``batch.x.permute(2, 0, 1).unsqueeze(0)`` (1, T, N, 8).  Each file holds
  * ``p__<name>``: the seeded state_dict (biases and SNorm's gamma / beta perturbed, so that every path is exercised) and its key list;
  * ``x`` (1, T, N, 8) and ``y`` (N, O): window ``window`` of tpims_fixture.npz, its first ``nodes`` nodes (STNorm has no graph);
  * ``train__out`` / ``train__loss`` / ``train__g__<name>`` / ``train__b__<name>``: one training-mode forward / backward with run.py's
    loss mean((out - y)**2) (broadcast as run.py broadcasts it), every parameter gradient in full and the running buffers after;
  * ``eval__out`` and run.py::test()'s and predict.py's metrics of an eval-mode forward that uses those buffers;
  * ``traj__loss`` (3,), ``traj__dp__<name>`` (the parameter step, fp16), ``traj__b__<name>``: windows window..window+2 accumulated
    as run.py::train() does, then one RMSprop(lr=1e-3, weight_decay=1e-4) step from the seeded state.
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
sys.dont_write_bytecode = True

from oracle.make_goldens import OUT, REF, fixture  # noqa: E402


def load_reference_stnorm():
    spec = importlib.util.spec_from_file_location("reference_stnorm", os.path.join(REF, "models", "STNorm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.STNorm


NODES = 72         # the first 72 of the fixture's 104 nodes: every per-node array (TNorm) shrinks, and each file stays near 500 KB


def window(fx, t_in, t_out, w):
    x = fx["node_data"][:NODES, :, w:w + t_in].permute(2, 0, 1).unsqueeze(0).contiguous()   # run.py:181
    y = fx["node_data"][:NODES, -1, w + t_in:w + t_in + t_out].contiguous()
    return x, y


def predict_metrics(out, y):
    """predict.py:176-180 for one batch: (mae, mse, mape) arrays before the mean."""
    err = y - out
    mape = np.abs(err.numpy()) / np.percentile(y.numpy(), q=95)
    return np.abs(err.numpy()).mean(), (err ** 2).mean().item(), mape.mean() * 100


def golden_stnorm(ST, fx, t_in, t_out, seed, tag, w=0):
    n = NODES
    torch.manual_seed(seed)
    mod = ST(num_nodes=n, in_dim=8, out_dim=t_out)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith("bias") or (name.endswith("beta") and p.dim() == 1):
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.4)
            elif name.endswith("gamma") and p.dim() == 1:     # SNorm; TNorm's per-node gamma / beta keep their 1 / 0 (file size)
                p.copy_(1 + (torch.rand(p.shape, generator=g) - 0.5) * 0.4)
        for p in mod.parameters():      # values with 8 significant bits (exact in fp32): the seeded state compresses
            p.copy_(p.to(torch.bfloat16).to(torch.float32))
    init = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    x, y = window(fx, t_in, t_out, w)
    out = {"t_in": t_in, "t_out": t_out, "seed": seed, "window": w, "nodes": n, "state_dict_keys": np.array(list(init.keys())),
           "x": x.numpy(), "y": y.numpy()}
    out.update({f"p__{k}": v.numpy().copy() for k, v in init.items()})

    mod.train()
    mod.zero_grad()
    o = mod(x)
    loss = torch.mean((o - y) ** 2)                              # run.py:184
    loss.backward()
    out["train__out"] = o.detach().numpy()
    out["train__loss"] = np.array([loss.item()])
    # (the last layer's residual conv feeds nothing: its gradient is None, listed in ``train__gnone``)
    out.update({f"train__g__{k}": p.grad.numpy().copy() for k, p in mod.named_parameters() if p.grad is not None})
    out["train__gnone"] = np.array([k for k, p in mod.named_parameters() if p.grad is None])
    out.update({f"train__b__{k}": b.numpy().copy() for k, b in mod.named_buffers()})

    mod.eval()
    with torch.no_grad():
        o = mod(x)
    out["eval__out"] = o.numpy()
    out["eval__test_mse"] = np.array([((o[0][0] - y) ** 2).mean().item()])     # run.py:217-221
    mae, mse, mape = predict_metrics(o, y)                                      # predict.py:176-180
    out["eval__mae"], out["eval__mse"], out["eval__mape"] = np.array([mae]), np.array([mse]), np.array([mape])

    mod.load_state_dict(init)
    mod.train()
    opt = torch.optim.RMSprop(mod.parameters(), lr=1e-3, weight_decay=1e-4)
    opt.zero_grad()
    losses = []
    for k in range(3):
        xk, yk = window(fx, t_in, t_out, w + k)
        lk = torch.mean((mod(xk) - yk) ** 2)
        lk.backward()
        losses.append(lk.item())
    opt.step()
    out["traj__loss"] = np.array(losses)
    # the step as an fp16 delta from the seeded parameters: RMSprop's first step is ~lr * sign(g), so the file stays small; a
    # comparison adds half an fp16 ulp of the delta to its bound
    out.update({f"traj__dp__{k}": (p.detach() - init[k]).numpy().astype(np.float16) for k, p in mod.named_parameters()})
    out.update({f"traj__b__{k}": b.numpy().copy() for k, b in mod.named_buffers()})
    path = os.path.join(OUT, f"golden_stnorm_{tag}.npz")
    np.savez_compressed(path, **out)
    return path, out["train__loss"][0]


def main():
    torch.set_num_threads(1)            # one summation order: the files are reproducible bit for bit
    ST = load_reference_stnorm()
    fx = fixture()
    for t_in, t_out, seed in ((6, 1, 21), (12, 3, 22)):
        path, loss = golden_stnorm(ST, fx, t_in, t_out, seed, f"in{t_in}_out{t_out}")
        print(path, os.path.getsize(path), "bytes, train loss", loss)


if __name__ == "__main__":
    main()
