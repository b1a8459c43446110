"""Golden vectors of the reference's SelfAttentionLayer (models/STAEformer.py:76-107), run unmodified on the CPU with its gradients.

    python tools/make_stae_layer_goldens.py

Needs the reference tree (oracle/make_goldens.py: REF); writes tests/golden/golden_stae_layer.npz:
  * ``p__<name>`` and ``state_dict_keys``: the seeded state_dict of SelfAttentionLayer(model_dim=64, feed_forward_dim=64, num_heads=2,
    dropout=0) with every bias and the LayerNorm weights and biases perturbed away from their 0 / 1 initial values and all values
    rounded to 5 significant bits, stored as bf16 byte planes (staeformer_math.encode_bf16);
  * ``x`` (2, 5, 7, 64) and ``dout`` (2, 5, 7, 64): the input and a fixed, non-uniform upstream gradient (a smooth pattern times
    seeded noise, so that no two rows or columns weigh alike);
  * for dim = 1 and dim = 2: ``dim<d>__out`` and ``dim<d>__grad__x`` / ``dim<d>__grad__<name>``, the gradients of sum(out * dout)
    with respect to the input and all 16 parameters, fp32 as the reference computes them.
It also prints the gap between tests/stae_layer_math.py in float64 and the recorded numbers (tests/test_stae_backward_cpu.py)."""
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

from oracle.make_goldens import OUT, REF  # noqa: E402
from make_staeformer_goldens import round5  # noqa: E402
from stae_layer_math import layer_grads  # noqa: E402
from staeformer_math import decode_bf16, encode_bf16  # noqa: E402

MODEL_DIM, HEADS, FF, SHAPE, SEED = 64, 2, 64, (2, 5, 7, 64), 51


def load_reference_layer():
    spec = importlib.util.spec_from_file_location("reference_staeformer", os.path.join(REF, "models", "STAEformer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SelfAttentionLayer


def main():
    torch.set_num_threads(1)            # one summation order: the file is reproducible bit for bit
    Layer = load_reference_layer()
    torch.manual_seed(SEED)
    mod = Layer(MODEL_DIM, feed_forward_dim=FF, num_heads=HEADS, dropout=0)
    g = torch.Generator().manual_seed(SEED)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith("bias"):
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.4)
            elif name.startswith("ln"):                                # LayerNorm gamma
                p.copy_(1.0 + (torch.rand(p.shape, generator=g) - 0.5) * 0.5)
        for p in mod.parameters():
            p.copy_(round5(p.detach()))
            assert torch.equal(p, decode_bf16(encode_bf16(p.detach())))
    sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    x = torch.randn(SHAPE, generator=g)
    b, t, n, d = SHAPE
    ramp = 1.0 + 0.5 * torch.sin(torch.arange(b * t * n * d, dtype=torch.float32) * 0.37).view(SHAPE)
    dout = ramp * torch.randn(SHAPE, generator=g)
    out = {"state_dict_keys": np.array(list(sd.keys())), "x": x.numpy(), "dout": dout.numpy(), "model_dim": MODEL_DIM, "num_heads": HEADS,
           "feed_forward_dim": FF, "seed": SEED}
    out.update({f"p__{k}": encode_bf16(v) for k, v in sd.items()})
    mod.train()                                                        # dropout 0: the identity, as in eval
    worst = 0.0
    for dim in (1, 2):
        xr = x.clone().requires_grad_(True)
        mod.zero_grad()
        o = mod(xr, dim=dim)
        o.backward(dout)
        out[f"dim{dim}__out"] = o.detach().numpy()
        grads = {"x": xr.grad}
        grads.update({k: p.grad for k, p in mod.named_parameters()})
        assert list(grads)[1:] == list(sd)
        for k, v in grads.items():
            out[f"dim{dim}__grad__{k}"] = v.detach().numpy().copy()
        o64, g64 = layer_grads(sd, x, dim, dout)
        worst = max(worst, float((o64 - o.detach().double()).abs().max()), *[float((g64[k] - grads[k].double()).abs().max()) for k in grads])
    path = os.path.join(OUT, "golden_stae_layer.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(sd), "keys, float64 restatement gap %.3g" % worst)


if __name__ == "__main__":
    main()
