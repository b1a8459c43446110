"""Float64 CPU restatement of the reference's SpatialGCN (models/SpatialGCN.py:30-49) in the reference's own order: per period
ChebConv (oracle.graph_ops.cheb_conv), ReLU, dropout as an explicit keep mask (x2), the second ChebConv, the sum over periods,
then linear1 -> ReLU -> linear2 on the sum (no ReLU before linear1: the reference's ``h = relu(H_accum)`` is dead)."""
import numpy as np
import torch

from oracle import graph_ops as G


def unpack_keep(keep, n: int, t: int, channels: int = 64) -> torch.Tensor:
    """(N*T, 2) int32 mask words (row node*T + t, bit j of word w keeps channel 32w + j) -> (N, T, 64) bool."""
    k = torch.as_tensor(np.asarray(keep)).to(torch.int64) & 0xFFFFFFFF
    bits = (k[:, :, None] >> torch.arange(32, dtype=torch.int64)) & 1            # (N*T, 2, 32)
    return bits.reshape(n * t, channels).bool().reshape(n, t, channels)


def spatial_embed(x, edge_index, edge_attr, w0, w1, b, keep=None):
    """S (N, 64) = sum_t keep_t * 2 * relu(cheb_conv(x_t)); x (N, F, T); keep (N*T, 2) int32 words or None (eval)."""
    n, _, t = x.shape
    km = None if keep is None else unpack_keep(keep, n, t)
    s = 0
    for p in range(t):
        g = torch.relu(G.cheb_conv(x[:, :, p], edge_index, edge_attr, w0, w1, b))
        if km is not None:
            g = g * km[:, p, :].to(g.dtype) * 2
        s = s + g
    return s


def spatial_gcn(params, x, edge_index, edge_attr, keep=None, dtype=torch.float64):
    """(pred (N, O), H (N, 256)) of the reference module; ``params`` keyed by its state_dict names (tensors may require grad)."""
    p = {k: v.to(dtype) if not v.requires_grad else v for k, v in params.items()}
    x = x.to(dtype)
    n, _, t = x.shape
    ew = None if edge_attr is None else edge_attr.to(dtype)
    km = None if keep is None else unpack_keep(keep, n, t)
    h = 0
    for period in range(t):
        g = G.cheb_conv(x[:, :, period], edge_index, ew, p["gcn.lins.0.weight"], p["gcn.lins.1.weight"], p["gcn.bias"])
        g = torch.relu(g)
        if km is not None:
            g = g * km[:, period, :].to(dtype) * 2
        g = G.cheb_conv(g, edge_index, ew, p["gcn2.lins.0.weight"], p["gcn2.lins.1.weight"], p["gcn2.bias"])
        h = h + g
    z = torch.relu(h @ p["linear1.weight"].t() + p["linear1.bias"])
    return z @ p["linear2.weight"].t() + p["linear2.bias"], h
