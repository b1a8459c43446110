"""Golden vectors of the reference's STAEformer (models/STAEformer.py), run unmodified in TRAIN mode on the TPIMS fixture.

    python tools/make_staeformer_train_goldens.py

Needs the reference tree (oracle/make_goldens.py: REF); writes tests/golden/golden_staeformer_train.npz: STAEformer(num_nodes=33,
in_steps=6, out_steps=1, tod_embedding_dim=0, num_layers=1, feed_forward_dim=64) -- model_dim 128, 4 heads, one temporal and one
spatial layer -- on the first 33 nodes of two fixture windows stacked to B = 2.  The parameters are perturbed and rounded as
make_staeformer_goldens.py does (``p__<name>`` byte planes, ``state_dict_keys``).  Two records:
  * ``r0__*``: dropout = 0;
  * ``r1__*``: dropout = 0.1 with ``torch.nn.functional.dropout`` replaced for the duration by a seeded keep mask
    (``inp * keep / (1 - p)``, as make_spatial_goldens.py does it); ``r1__keep`` holds the four masks as the project's words, int32
    (4, B T N, model_dim / 32): site order dropout1, dropout2 of the temporal layer, then of the spatial layer, rows (b T + t) N + n
    (the temporal layer sees its tensor transposed to (B, N, T, D); the mask is transposed back), bit j of word w keeps column 32w + j.
Each record holds ``out`` (B, 1, N, 1), ``loss`` (B,): run.py:184-186's mean((out - y) ** 2) per snapshot, and ``g__<name>``: the
gradient of the sum of the two losses (run.py accumulates gradients over snapshots).  SIZE: the file must stay under 1 MiB, and the
two records' fp32 gradients of all 38 parameters alone are 1.4 MB, so record r0 leaves out the gradients of the twelve 2-D layer
weights (attn.FC_Q / FC_K / FC_V / out_proj and feed_forward.0 / .2 of both layers; 164 k of the 181 k parameters); it keeps
those of every embedding, the output projection, every bias and every LayerNorm parameter.  Record r1, the one with dropout, holds
all of them (``r0__grad_keys`` / ``r1__grad_keys`` list what is there).  The script prints the file's size."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

from oracle.make_goldens import OUT, fixture  # noqa: E402
from make_staeformer_goldens import load_reference_staeformer, pick_windows, round5, window  # noqa: E402
from staeformer_math import decode_bf16, encode_bf16  # noqa: E402
from staeformer_train_math import model_grads, pack_keep  # noqa: E402

NODES, T_IN, T_OUT, SEED, P, FF = 33, 6, 1, 43, 0.1, 64


def build(ST, dropout):
    torch.manual_seed(SEED)
    mod = ST(num_nodes=NODES, in_steps=T_IN, out_steps=T_OUT, tod_embedding_dim=0, num_layers=1, feed_forward_dim=FF, dropout=dropout)
    g = torch.Generator().manual_seed(SEED)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith("bias"):
                p.copy_((torch.rand(p.shape, generator=g) - 0.5) * 0.4)
            elif ".ln" in name:
                p.copy_(1.0 + (torch.rand(p.shape, generator=g) - 0.5) * 0.5)
        for p in mod.parameters():
            p.copy_(round5(p.detach()))
            assert torch.equal(p, decode_bf16(encode_bf16(p.detach())))
    return mod.train()


def run(mod, x, y):
    mod.zero_grad()
    out = mod(x)
    losses = torch.stack([((out[k:k + 1] - y[k]) ** 2).mean() for k in range(x.shape[0])])       # run.py:184-186 per snapshot
    losses.sum().backward()
    return out.detach(), losses.detach(), {k: p.grad.detach().clone() for k, p in mod.named_parameters()}


def main():
    torch.set_num_threads(1)
    ST = load_reference_staeformer()
    fx = {"node_data": fixture()["node_data"][:NODES].contiguous()}
    windows = pick_windows(fx, T_IN, T_OUT, 2)
    xs, ys = zip(*[window(fx, T_IN, T_OUT, w) for w in windows])
    x, y = torch.cat(xs), torch.stack(ys)
    b, m, d = x.shape[0], x.shape[0] * T_IN * NODES, 128
    out = {"windows": np.array(windows), "nodes": NODES, "t_in": T_IN, "t_out": T_OUT, "seed": SEED, "p": np.float32(P),
           "feed_forward_dim": FF, "x": x.numpy(), "y": y.numpy()}

    mod = build(ST, 0.0)
    sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    out["state_dict_keys"] = np.array(list(sd))
    out.update({f"p__{k}": encode_bf16(v) for k, v in sd.items()})
    records = {"r0": run(mod, x, y)}

    mod = build(ST, P)
    assert all(torch.equal(v, sd[k]) for k, v in mod.state_dict().items())
    gen = torch.Generator().manual_seed(1000 + SEED)
    masks = []
    orig = torch.nn.functional.dropout

    def dropout(inp, p=0.5, training=True, inplace=False):
        assert abs(p - P) < 1e-12 and training and not inplace
        keep = torch.rand(inp.shape, generator=gen) >= P
        masks.append(keep)
        return inp * keep / (1 - P)

    torch.nn.functional.dropout = dropout
    try:
        records["r1"] = run(mod, x, y)
    finally:
        torch.nn.functional.dropout = orig
    assert len(masks) == 4 and tuple(masks[0].shape) == (b, NODES, T_IN, d) and tuple(masks[2].shape) == (b, T_IN, NODES, d)
    rows = [k.transpose(1, 2) if i < 2 else k for i, k in enumerate(masks)]              # the temporal layer works on (B, N, T, D)
    keep = pack_keep(torch.stack([k.reshape(m, d) for k in rows]))
    out["r1__keep"] = keep.numpy()

    big = [k for k, v in sd.items() if v.dim() == 2 and k.startswith("attn_layers_")]
    assert len(big) == 12
    for tag, (o, losses, grads) in records.items():
        keys = [k for k in grads if not (tag == "r0" and k in big)]
        out[f"{tag}__out"], out[f"{tag}__loss"], out[f"{tag}__grad_keys"] = o.numpy(), losses.numpy(), np.array(keys)
        out.update({f"{tag}__g__{k}": grads[k].numpy() for k in keys})
    path = os.path.join(OUT, "golden_staeformer_train.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < (1 << 20), "the golden file must stay under 1 MiB"
    for tag, kp, p in (("r0", None, 0.0), ("r1", keep, P)):
        o64, l64, g64 = model_grads(sd, x, T_OUT, keep=kp, drop=p, y=y)
        o, losses, grads = records[tag]
        worst = max(float((g64[k] - grads[k].double()).abs().max() / max(float(g64[k].abs().max()), 1e-30)) for k in grads)
        print(f"{tag}: float64 restatement vs recorded fp32: out {float((o64 - o.double()).abs().max()):.3g}, loss "
              f"{float((l64 - losses.double()).abs().max()):.3g}, worst whole-tensor gradient ratio {worst:.3g}")


if __name__ == "__main__":
    main()
