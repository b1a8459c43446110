"""Golden vectors of the reference's STAEformer (models/STAEformer.py), run unmodified in eval mode on the TPIMS fixture.

    python tools/make_staeformer_goldens.py

Needs the reference tree (oracle/make_goldens.py: REF); writes
  * tests/golden/golden_staeformer_in6_out1.npz: run.py:132's construction (STAEformer(num_nodes=N, in_steps=6, out_steps=1,
    tod_embedding_dim=0): model_dim 128, 4 heads, 3 + 3 layers) on all 104 nodes, one window, B = 1;
  * tests/golden/golden_staeformer_in12_out3_b2.npz: the same with num_layers=1, in_steps=12, out_steps=3 and two windows stacked to
    B = 2.
The input is run.py's, ``batch.x.permute(2, 0, 1).unsqueeze(0)`` (1, T, N, 8) per window.  Each file holds
  * ``p__<name>``: the seeded state_dict with every bias and the LayerNorm weights and biases perturbed (a dropped bias or a swapped
    gamma / beta shows) and all values rounded to 5 significant bits (exact in bf16 and fp32), stored as the two byte planes of
    their bf16 patterns (staeformer_math.encode_bf16 / decode_bf16; the file compresses to under 1 MiB), and its key list
    ``state_dict_keys``;
  * ``init__adaptive_embedding_t0`` / ``init__input_proj.weight``: adaptive_embedding[0] and input_proj.weight as the seeded
    construction drew them (one xavier-uniform and one default initialiser, at full precision);
  * ``x`` (B, T, N, 8), ``y`` (B, N, O) and ``windows``: the windows of tpims_fixture.npz, chosen so that x[..., 2].long() hits both
    rows 0 and 1 of dow_embedding (asserted);
  * ``eval__out`` (B, O, N, 1), run.py::test()'s ``eval__test_mse`` per window and predict.py's ``eval__mae`` / ``eval__mse`` /
    ``eval__mape`` over the windows.
It also prints the gap between tests/staeformer_math.py in float64 and the recorded fp32 output (tests/test_staeformer_cpu.py)."""
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
from staeformer_math import decode_bf16, encode_bf16, staeformer  # noqa: E402


def load_reference_staeformer():
    spec = importlib.util.spec_from_file_location("reference_staeformer", os.path.join(REF, "models", "STAEformer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.STAEformer


def window(fx, t_in, t_out, w):
    x = fx["node_data"][:, :, w:w + t_in].permute(2, 0, 1).unsqueeze(0).contiguous()   # run.py:218
    y = fx["node_data"][:, -1, w + t_in:w + t_in + t_out].contiguous()
    return x, y


def round5(t: torch.Tensor) -> torch.Tensor:
    """fp32 values rounded to 5 significant bits (4 stored mantissa bits): a subset of the bf16 values."""
    bits = t.contiguous().view(torch.int32)
    return ((bits + (1 << 18)) & ~((1 << 19) - 1)).view(torch.float32)


def pick_windows(fx, t_in, t_out, count, start=0):
    """The first ``count`` windows from ``start`` on whose day-of-week column hits both rows 0 and 1 of the table and nothing else
    outside it (the reference's embedding would raise)."""
    last = fx["node_data"].shape[2] - t_in - t_out
    picked = []
    for w in range(start, last + 1):
        rows = set(window(fx, t_in, t_out, w)[0][..., 2].long().unique().tolist())
        if {0, 1} <= rows and min(rows) >= 0 and max(rows) < 7:
            picked.append(w)
            if len(picked) == count:
                return picked
    raise SystemExit("no window of the fixture hits rows 0 and 1 of dow_embedding")


def golden(ST, fx, t_in, t_out, seed, tag, windows, **kw):
    n = fx["node_data"].shape[0]
    torch.manual_seed(seed)
    mod = ST(num_nodes=n, in_steps=t_in, out_steps=t_out, tod_embedding_dim=0, **kw)      # run.py:132
    out = {"t_in": t_in, "t_out": t_out, "seed": seed, "windows": np.array(windows), "nodes": n, "num_layers": mod.num_layers,
           "init__adaptive_embedding_t0": mod.adaptive_embedding[0].detach().numpy().copy(),
           "init__input_proj.weight": mod.input_proj.weight.detach().numpy().copy()}
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith("bias"):
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.4)
            elif ".ln" in name:                                    # LayerNorm gamma
                p.copy_(1.0 + (torch.rand(p.shape, generator=g) - 0.5) * 0.5)
        for p in mod.parameters():
            p.copy_(round5(p.detach()))
            assert torch.equal(p, decode_bf16(encode_bf16(p.detach())))
    sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    xs, ys = zip(*[window(fx, t_in, t_out, w) for w in windows])
    x, y = torch.cat(xs), torch.stack(ys)
    rows = set(x[..., 2].long().unique().tolist())
    assert {0, 1} <= rows, rows
    out.update({"state_dict_keys": np.array(list(sd.keys())), "x": x.numpy(), "y": y.numpy()})
    out.update({f"p__{k}": encode_bf16(v) for k, v in sd.items()})
    mod.eval()
    with torch.no_grad():
        o = mod(x)
    out["eval__out"] = o.numpy()
    out["eval__test_mse"] = np.array([((o[k:k + 1][0][0] - y[k]) ** 2).mean().item() for k in range(len(windows))])    # run.py:217-222
    ae, se, ape = [], [], []
    for k in range(len(windows)):                                                                                       # predict.py:176-181
        err = (y[k] - o[k:k + 1]).numpy()
        ae.append(np.abs(err)), se.append(err ** 2), ape.append(np.abs(err) / np.percentile(y[k].numpy(), q=95))
    out["eval__mae"] = np.array([np.concatenate(ae).mean()])
    out["eval__mse"] = np.array([np.concatenate(se).mean()])
    out["eval__mape"] = np.array([np.concatenate(ape).mean() * 100])
    path = os.path.join(OUT, f"golden_staeformer_{tag}.npz")
    np.savez_compressed(path, **out)
    o64 = staeformer(sd, x, t_out)
    return path, len(sd), float((o64 - o.double()).abs().max()), float(o.abs().max())


def main():
    torch.set_num_threads(1)            # one summation order: the files are reproducible bit for bit
    ST = load_reference_staeformer()
    fx = fixture()
    for t_in, t_out, seed, tag, count, kw in ((6, 1, 41, "in6_out1", 1, {}), (12, 3, 42, "in12_out3_b2", 2, {"num_layers": 1})):
        path, nkeys, gap, mag = golden(ST, fx, t_in, t_out, seed, tag, pick_windows(fx, t_in, t_out, count), **kw)
        print(path, os.path.getsize(path), "bytes,", nkeys, "keys, float64 restatement gap %.3g at output magnitude %.3g" % (gap, mag))


if __name__ == "__main__":
    main()
