"""STID (Shao et al., CIKM 2022, "Spatial-Temporal Identity") restated in plain torch, float64 by default, from the paper's
definition and the shapes of the module's parameters, with the temporal identities switched off (run.py's configuration):

    E_n   = We vec(X_n) + be                     vec(X_n)[l * input_dim + c] = x[b, l, n, c], c < input_dim
    H_0   = [E_n | node_emb_n]                   (only E_n without the spatial identity)
    H_l+1 = W2_l (keep_l * relu(W1_l H_l + b1_l) / (1 - p)) + b2_l + H_l
    out_n = Wr H_L + br

``keep`` is an explicit boolean mask (num_layer, B, N, hidden) or None (eval: no dropout).  ``pack_keep`` / ``unpack_keep`` convert
it to and from the kernels' bit layout: int32 (num_layer, B, N, hidden / 32), bit j of word w keeps channel 32 w + j."""
import numpy as np
import torch


def pack_keep(keep: torch.Tensor) -> torch.Tensor:
    k = keep.cpu().numpy().astype(np.uint8)
    words = np.packbits(k.reshape(k.shape[:-1] + (k.shape[-1] // 32, 32)), axis=-1, bitorder="little")
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).reshape(k.shape[:-1] + (k.shape[-1] // 32,)))


def unpack_keep(words: torch.Tensor) -> torch.Tensor:
    w = np.ascontiguousarray(words.cpu().numpy().astype(np.int32))
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape + (4,)), axis=-1, bitorder="little")
    return torch.from_numpy(bits.reshape(w.shape[:-1] + (w.shape[-1] * 32,)).astype(bool))


def stid(p, x, input_dim, keep=None, dropout_p=0.15, dtype=torch.float64):
    """out (B, output_len, N, 1) for x (B, L, N, C); ``p`` maps the state_dict names to tensors."""
    c = lambda t: t.to(dtype)
    b, l, n, _ = x.shape
    rows = c(x)[..., :input_dim].permute(0, 2, 1, 3).reshape(b, n, l * input_dim)
    we = c(p["time_series_emb_layer.weight"])
    h = rows @ we.reshape(we.shape[0], -1).T + c(p["time_series_emb_layer.bias"])
    if "node_emb" in p:
        h = torch.cat([h, c(p["node_emb"]).unsqueeze(0).expand(b, -1, -1)], dim=-1)
    i = 0
    while f"encoder.{i}.fc1.weight" in p:
        w1, w2 = c(p[f"encoder.{i}.fc1.weight"]), c(p[f"encoder.{i}.fc2.weight"])
        a = torch.relu(h @ w1.reshape(w1.shape[0], -1).T + c(p[f"encoder.{i}.fc1.bias"]))
        if keep is not None:
            a = a * keep[i].to(a.device).to(dtype) / (1.0 - dropout_p)
        h = a @ w2.reshape(w2.shape[0], -1).T + c(p[f"encoder.{i}.fc2.bias"]) + h
        i += 1
    wr = c(p["regression_layer.weight"])
    out = h @ wr.reshape(wr.shape[0], -1).T + c(p["regression_layer.bias"])
    return out.permute(0, 2, 1).unsqueeze(-1)
