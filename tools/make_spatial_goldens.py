"""Golden vectors of the reference's SpatialGCN (models/SpatialGCN.py), run unmodified on the TPIMS fixture.

    python tools/make_spatial_goldens.py

Needs the reference tree (oracle/make_goldens.py: REF) and its stand-in ChebConv; writes
tests/golden/golden_spatial_in6_out1.npz and golden_spatial_in12_out3.npz.  Each file holds
  * the seeded parameters (``p__<name>``) and the state_dict key list (``state_dict_keys``);
  * ``eval__*``: pred, hidden, loss and the gradient summary of oracle/make_goldens.grads_summary with the module in eval mode;
  * ``train__*``: the same in training mode, with F.dropout replaced by a seeded Bernoulli(0.5) keep mask (``g * keep * 2``),
    recorded as ``train__keep`` (N*T, 2) int32 in the layout of regt_spatial_embed_forward (row node*T + t, bit j of word w keeps
    channel 32w + j).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.make_goldens import OUT, REF, fixture, grads_summary, install_standins, param_checksum  # noqa: E402


def load_reference_spatial():
    install_standins()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from models.SpatialGCN import SpatialGCN  # noqa
    return SpatialGCN


def pack_keep(masks, channels: int = 64) -> np.ndarray:
    """masks: T boolean (N, 64) keep masks -> (N*T, 2) int32 bits, row node*T + t."""
    k = torch.stack(masks, dim=1).reshape(-1, channels).to(torch.int64)            # (N*T, 64)
    words = []
    for w in range(channels // 32):
        bits = k[:, 32 * w:32 * (w + 1)] << torch.arange(32, dtype=torch.int64)
        words.append(bits.sum(dim=1))
    u = torch.stack(words, dim=1).numpy().astype(np.uint32)
    return u.view(np.int32)


def run(mod, x, fx, y):
    mod.zero_grad()
    pred, hidden = mod(x=x, edge_index=fx["edge_index"], edge_attr=fx["edge_attr"])   # keyword call, run.py:188
    loss = torch.mean((pred - y) ** 2)
    loss.backward()
    return pred.detach().numpy(), hidden.detach().numpy(), float(loss.detach()), {n: p.grad for n, p in mod.named_parameters()}


def golden_spatial(SG, fx, t_in, t_out, seed, tag, window=0):
    x = fx["node_data"][:, :, window:window + t_in].contiguous()
    y = fx["node_data"][:, -1, window + t_in:window + t_in + t_out].contiguous()
    torch.manual_seed(seed)
    mod = SG(node_features=8, periods=t_in, output_dim=t_out)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                 # non-zero biases, so that every bias gradient and the ReLU pattern are exercised
        for name, p in mod.named_parameters():
            if name.endswith("bias"):
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.4)
    sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    out = {"t_in": t_in, "t_out": t_out, "seed": seed, "window": window, "param_checksum": param_checksum(sd),
           "state_dict_keys": np.array(list(sd.keys()))}
    out.update({f"p__{k}": v.numpy() for k, v in sd.items()})

    mod.eval()
    pred, hidden, loss, grads = run(mod, x, fx, y)
    out.update({"eval__pred": pred, "eval__hidden": hidden, "eval__loss": np.array([loss])})
    out.update({f"eval__{k}": v for k, v in grads_summary(grads).items()})

    mod.train()
    gen = torch.Generator().manual_seed(1000 + seed)
    masks = []
    orig = torch.nn.functional.dropout

    def dropout(inp, p=0.5, training=True, inplace=False):
        assert p == 0.5 and training and not inplace
        keep = torch.rand(inp.shape, generator=gen) < 0.5
        masks.append(keep)
        return inp * keep * 2

    torch.nn.functional.dropout = dropout
    try:
        pred, hidden, loss, grads = run(mod, x, fx, y)
    finally:
        torch.nn.functional.dropout = orig
    assert len(masks) == t_in
    out.update({"train__pred": pred, "train__hidden": hidden, "train__loss": np.array([loss]), "train__keep": pack_keep(masks)})
    out.update({f"train__{k}": v for k, v in grads_summary(grads).items()})
    np.savez_compressed(os.path.join(OUT, f"golden_spatial_{tag}.npz"), **out)
    return out["eval__loss"][0], loss


def main():
    SG = load_reference_spatial()
    fx = fixture()
    for t_in, t_out, seed in ((6, 1, 12), (12, 3, 13)):
        print("spatial", t_in, t_out, "loss eval / train", golden_spatial(SG, fx, t_in, t_out, seed, f"in{t_in}_out{t_out}"))
    print("goldens written to", OUT)


if __name__ == "__main__":
    main()
