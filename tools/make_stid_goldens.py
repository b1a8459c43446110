"""Golden vectors of the reference's STID (models/STID.py), run unmodified on the TPIMS fixture.

    python tools/make_stid_goldens.py

Needs the reference tree (oracle/make_goldens.py: REF); writes tests/golden/golden_stid_in6_out1.npz and golden_stid_in12_out3.npz.
The model is built as run.py:134 builds it (STID(num_nodes=N, input_len=T, output_len=O, if_time_in_day=False,
if_day_in_week=False), so input_dim = 3) on all 104 nodes and fed run.py's input, ``batch.x.permute(2, 0, 1).unsqueeze(0)``
(1, T, N, 8).  Each file holds
  * ``init__node_emb`` / ``init__time_series_emb_layer.weight``: those two tensors as the seeded construction drew them;
  * ``p__<name>``: the seeded state_dict with the biases perturbed (every path carries signal) and all values rounded to 8
    significant bits (exact in fp32; the file compresses), and its key list;
  * ``x`` (1, T, N, 8) and ``y`` (N, O): window ``window`` of tpims_fixture.npz;
  * ``train__out`` / ``train__loss`` / ``train__g__<name>`` / ``train__keep``: one training-mode forward / backward with run.py's
    loss mean((out - y)**2) (broadcast as run.py broadcasts it), every parameter gradient, and the keep mask the reference drew:
    a forward hook on each block's nn.Dropout records ``(out != 0) | (inp == 0)`` (where the ReLU output is 0 the bit changes
    neither the output nor a gradient), packed as the kernels read it: int32 (num_layer, 1, N, 2), bit j of word w = channel 32w + j;
  * ``eval__out`` and run.py::test()'s and predict.py's metrics of an eval-mode forward;
  * ``traj__loss`` (3,), ``traj__keep`` (3, num_layer, 1, N, 2), ``traj__dp__<name>`` (the parameter step, fp16): windows
    window..window+2 accumulated as run.py::train() does, then one RMSprop(lr=1e-3, weight_decay=1e-4) step from the seeded state.
It also prints the largest gap between tests/stid_math.py in float64 and the recorded fp32 results (tests/test_stid_cpu.py: GRAD_GAP).
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
from stid_math import pack_keep, stid, unpack_keep  # noqa: E402


def load_reference_stid():
    spec = importlib.util.spec_from_file_location("reference_stid", os.path.join(REF, "models", "STID.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.STID


def window(fx, t_in, t_out, w):
    x = fx["node_data"][:, :, w:w + t_in].permute(2, 0, 1).unsqueeze(0).contiguous()   # run.py:181
    y = fx["node_data"][:, -1, w + t_in:w + t_in + t_out].contiguous()
    return x, y


def predict_metrics(out, y):
    """predict.py:176-180 for one batch: (mae, mse, mape) before the mean over batches."""
    err = y - out
    mape = np.abs(err.numpy()) / np.percentile(y.numpy(), q=95)
    return np.abs(err.numpy()).mean(), (err ** 2).mean().item(), mape.mean() * 100


class KeepRecorder:
    """Forward hooks on the blocks' nn.Dropout modules: the keep mask of each call, in block order."""

    def __init__(self, mod):
        self.masks = []
        for block in mod.encoder:
            block.drop.register_forward_hook(self._hook)

    def _hook(self, module, inputs, output):
        if module.training:
            self.masks.append(((output != 0) | (inputs[0] == 0)).detach())

    def take(self):
        m = torch.stack([k[..., 0].permute(0, 2, 1) for k in self.masks])    # (1, H, N, 1) each -> (num_layer, 1, N, H)
        self.masks = []
        return pack_keep(m)


def golden_stid(ST, fx, t_in, t_out, seed, tag, w=0):
    n = fx["node_data"].shape[0]
    torch.manual_seed(seed)
    mod = ST(num_nodes=n, input_len=t_in, output_len=t_out, if_time_in_day=False, if_day_in_week=False)
    out = {"t_in": t_in, "t_out": t_out, "seed": seed, "window": w, "nodes": n,
           "init__node_emb": mod.node_emb.detach().numpy().copy(),
           "init__time_series_emb_layer.weight": mod.time_series_emb_layer.weight.detach().numpy().copy()}
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith("bias"):
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.4)
        for p in mod.parameters():
            p.copy_(p.to(torch.bfloat16).to(torch.float32))
    init = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    rec = KeepRecorder(mod)
    x, y = window(fx, t_in, t_out, w)
    out.update({"state_dict_keys": np.array(list(init.keys())), "x": x.numpy(), "y": y.numpy()})
    out.update({f"p__{k}": v.numpy().copy() for k, v in init.items()})

    mod.train()
    mod.zero_grad()
    o = mod(x)
    loss = torch.mean((o - y) ** 2)                              # run.py:186
    loss.backward()
    assert all(p.grad is not None for p in mod.parameters())
    out["train__out"] = o.detach().numpy()
    out["train__loss"] = np.array([loss.item()])
    out.update({f"train__g__{k}": p.grad.numpy().copy() for k, p in mod.named_parameters()})
    out["train__keep"] = rec.take().numpy()

    mod.eval()
    with torch.no_grad():
        o = mod(x)
    out["eval__out"] = o.numpy()
    out["eval__test_mse"] = np.array([((o[0][0] - y) ** 2).mean().item()])     # run.py:217-222
    mae, mse, mape = predict_metrics(o, y)                                      # predict.py:176-180
    out["eval__mae"], out["eval__mse"], out["eval__mape"] = np.array([mae]), np.array([mse]), np.array([mape])

    mod.load_state_dict(init)
    mod.train()
    opt = torch.optim.RMSprop(mod.parameters(), lr=1e-3, weight_decay=1e-4)
    opt.zero_grad()
    losses, keeps = [], []
    for k in range(3):
        xk, yk = window(fx, t_in, t_out, w + k)
        lk = torch.mean((mod(xk) - yk) ** 2)
        lk.backward()
        losses.append(lk.item())
        keeps.append(rec.take().numpy())
    opt.step()
    out["traj__loss"] = np.array(losses)
    out["traj__keep"] = np.stack(keeps)
    out.update({f"traj__dp__{k}": (p.detach() - init[k]).numpy().astype(np.float16) for k, p in mod.named_parameters()})
    path = os.path.join(OUT, f"golden_stid_{tag}.npz")
    np.savez_compressed(path, **out)

    # the float64 restatement against what was just recorded: the fp32-vs-float64 gap of the reference itself
    p64 = {k: v.double().requires_grad_(True) for k, v in init.items()}
    o64 = stid(p64, x, 3, keep=unpack_keep(torch.from_numpy(out["train__keep"])))
    torch.mean((o64 - y.double()) ** 2).backward()
    gap_out = float((o64.detach() - torch.from_numpy(out["train__out"]).double()).abs().max())
    gap_grad = max(float((p64[k].grad - torch.from_numpy(out[f"train__g__{k}"]).double()).abs().max()) for k in init)
    return path, out["train__loss"][0], gap_out, gap_grad


def main():
    torch.set_num_threads(1)            # one summation order: the files are reproducible bit for bit
    ST = load_reference_stid()
    fx = fixture()
    for t_in, t_out, seed in ((6, 1, 31), (12, 3, 32)):
        path, loss, gap_out, gap_grad = golden_stid(ST, fx, t_in, t_out, seed, f"in{t_in}_out{t_out}")
        print(path, os.path.getsize(path), "bytes, train loss", loss, "float64 restatement gap: out %.3g grad %.3g" % (gap_out, gap_grad))


if __name__ == "__main__":
    main()
