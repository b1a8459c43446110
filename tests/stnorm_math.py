"""Float64 restatement of the reference's STNorm (models/STNorm.py) for tests: the same layer sequence as the module, written
as functions of a parameter dict keyed by the state_dict names, with TNorm's statistics pooled over groups of ``tnorm_group``
consecutive batch elements (None = the whole batch, the reference's semantics).  Returns the output and the running buffers as
they stand afterwards (updated group by group, in order, in training mode)."""
import torch

EPS = 1e-5
MOMENTUM = 0.1


def receptive_field(blocks: int, layers: int) -> int:
    return 1 + blocks * ((1 << layers) - 1)


def conv1x1(x, w, b):
    """x (B, C, N, L), w (O, C, 1, 1)."""
    return torch.einsum("oc,bcnl->bonl", w[:, :, 0, 0], x) + b.view(1, -1, 1, 1)


def dilated_conv(x, w, b, d):
    """kernel (1, 2) with dilation d: out[t] = W[..., 0] x[t] + W[..., 1] x[t + d] + b."""
    n = x.shape[3] - d
    return (torch.einsum("oc,bcnl->bonl", w[:, :, 0, 0], x[..., :n]) + torch.einsum("oc,bcnl->bonl", w[:, :, 0, 1], x[..., d:d + n])
            + b.view(1, -1, 1, 1))


def tnorm(x, gamma, beta, rm, rv, training, group):
    if not training:
        return (x - rm) / (rv + EPS) ** 0.5 * gamma + beta, rm, rv
    outs = []
    for g0 in range(0, x.shape[0], group):
        xg = x[g0:g0 + group]
        mean = xg.mean((0, 3), keepdim=True)
        var = xg.var((0, 3), keepdim=True, unbiased=False)
        n = xg.shape[0] * xg.shape[3]
        with torch.no_grad():
            rm = MOMENTUM * mean + (1 - MOMENTUM) * rm
            rv = MOMENTUM * var * n / (n - 1) + (1 - MOMENTUM) * rv
        outs.append((xg - mean) / (var + EPS) ** 0.5 * gamma + beta)
    return torch.cat(outs, 0), rm, rv


def snorm(x, gamma, beta):
    """gamma, beta (C,); a (B, C) tensor gives every batch element its own copy (tests that take one element's share of a gradient)."""
    xn = (x - x.mean(2, keepdim=True)) / (x.var(2, keepdim=True, unbiased=True) + EPS) ** 0.5
    return xn * gamma.view(-1, gamma.shape[-1], 1, 1) + beta.view(-1, beta.shape[-1], 1, 1)


def stnorm(p, x, blocks=4, layers=2, tnorm_bool=True, snorm_bool=True, training=True, tnorm_group=None, dtype=torch.float64):
    """out (B, O, N, L_out) and {buffer name: tensor} for x (B, L, N, C_in); ``p``: state_dict names -> tensors (may require grad)."""
    p = {k: (v if v.requires_grad else v.to(dtype)) for k, v in p.items()}
    x = x.to(dtype).permute(0, 3, 2, 1)
    rf = receptive_field(blocks, layers)
    if x.shape[3] < rf:
        x = torch.nn.functional.pad(x, (rf - x.shape[3], 0, 0, 0))
    x = conv1x1(x, p["start_conv.weight"], p["start_conv.bias"])
    group = x.shape[0] if tnorm_group is None else tnorm_group
    bufs = {}
    skip = None
    for i in range(blocks * layers):
        d = 1 << (i % layers)
        parts = [x]
        if tnorm_bool:
            y, rm, rv = tnorm(x, p[f"tn.{i}.gamma"], p[f"tn.{i}.beta"], p[f"tn.{i}.running_mean"], p[f"tn.{i}.running_var"], training,
                              group)
            bufs[f"tn.{i}.running_mean"], bufs[f"tn.{i}.running_var"] = rm, rv
            parts.append(y)
        if snorm_bool:
            parts.append(snorm(x, p[f"sn.{i}.gamma"], p[f"sn.{i}.beta"]))
        z = torch.cat(parts, 1)
        h = torch.tanh(dilated_conv(z, p[f"filter_convs.{i}.weight"], p[f"filter_convs.{i}.bias"], d)) * \
            torch.sigmoid(dilated_conv(z, p[f"gate_convs.{i}.weight"], p[f"gate_convs.{i}.bias"], d))
        s = conv1x1(h, p[f"skip_convs.{i}.weight"], p[f"skip_convs.{i}.bias"])
        skip = s if skip is None else s + skip[..., -s.shape[3]:]
        x = conv1x1(h, p[f"residual_convs.{i}.weight"], p[f"residual_convs.{i}.bias"]) + x[..., -h.shape[3]:]
    r = torch.relu(conv1x1(torch.relu(skip), p["end_conv_1.weight"], p["end_conv_1.bias"]))
    return conv1x1(r, p["end_conv_2.weight"], p["end_conv_2.bias"]), bufs
