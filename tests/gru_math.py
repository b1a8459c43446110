"""StackedGRU (models/StackedGRU.py) and the GRU step it runs, restated in plain tensor operations -- no nn.GRU -- so that the
arithmetic is stated independently of both torch's recurrent code and the HIP kernels.  Runs in the dtype of the parameters
(float64 in the tests); differentiable by autograd.

    r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)      z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
    n = tanh(W_in x + b_in + r * (W_hn h + b_hn))   h' = (1 - z) * n + z * h            gates stacked r, z, n
"""
import torch

HIDDEN = 256
KEYS = ["gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0", "gru2.weight_ih_l0", "gru2.weight_hh_l0",
        "gru2.bias_ih_l0", "gru2.bias_hh_l0", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias"]


def gru_layer(x, w_ih, w_hh, b_ih, b_hh, h0=None):
    """x (S, rows, T), sequence first -> (out (S, rows, H), h_last (rows, H))."""
    hd = w_hh.shape[1]
    h = x.new_zeros(x.shape[1], hd) if h0 is None else h0.reshape(x.shape[1], hd)
    gi_all = x @ w_ih.t() + b_ih                                   # (S, rows, 3H)
    outs = []
    for s in range(x.shape[0]):
        gi, gh = gi_all[s], h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, :hd] + gh[:, :hd])
        z = torch.sigmoid(gi[:, hd:2 * hd] + gh[:, hd:2 * hd])
        n = torch.tanh(gi[:, 2 * hd:] + r * gh[:, 2 * hd:])
        h = (1 - z) * n + z * h
        outs.append(h)
    return torch.stack(outs), h


def stacked_gru(p, x):
    """models/StackedGRU.py:18-30: x (N, rows, T) -> (N, rows, O).  ``p``: the state_dict (12 entries, KEYS)."""
    x = x.to(p["gru.weight_ih_l0"].dtype)
    _, h = gru_layer(x, *[p[f"gru.{k}_l0"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")])
    out, _ = gru_layer(x, *[p[f"gru2.{k}_l0"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")], h0=h)
    return torch.relu(out @ p["linear1.weight"].t() + p["linear1.bias"]) @ p["linear2.weight"].t() + p["linear2.bias"]


def build_params(seed: int, t_in: int, t_out: int):
    """The seeded construction of the reference (nn.GRU, nn.GRU, nn.Linear, nn.Linear in that order after torch.manual_seed),
    rounded to bf16 and held in fp32: the parameters of the goldens."""
    torch.manual_seed(seed)
    mods = [torch.nn.GRU(input_size=t_in, hidden_size=HIDDEN), torch.nn.GRU(input_size=t_in, hidden_size=HIDDEN),
            torch.nn.Linear(HIDDEN, HIDDEN), torch.nn.Linear(HIDDEN, t_out)]
    vals = [q.detach() for m in mods for q in m.parameters()]
    return {k: v.to(torch.bfloat16).to(torch.float32) for k, v in zip(KEYS, vals)}


def sample(t: torch.Tensor):
    """What a golden keeps of a large matrix: every 61st element in fp32, and float64 row and column sums."""
    return t.flatten()[::61].clone(), t.double().sum(1), t.double().sum(0)


LARGE = ("gru.weight_hh_l0", "gru2.weight_hh_l0", "linear1.weight")


def bar(gap: float) -> float:
    """The tolerance of a comparison with a float64 reference, relative to the reference tensor's largest magnitude: 8 x the fp32
    reference's own gap to float64 (another summation order and other exp / tanh code, both carried through the recurrence), at
    least 32 x 2^-24 (two chained 256-term fp32 dot products under reordering), never above 1e-4."""
    return min(max(8.0 * gap, 32.0 * 2.0 ** -24), 1e-4)


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |got - ref| / max |ref|; an all-zero reference must be met exactly."""
    return float((got.detach().double().cpu() - ref.detach().double().cpu()).abs().max() / ref.detach().double().abs().max().clamp_min(1e-300))


def rmsprop_first_step(g: torch.Tensor, p: torch.Tensor, lr=1e-3, wd=1e-4, alpha=0.99, eps=1e-8):
    """The first RMSprop step from a zero square average, and the bound of its change under a gradient error of at most ``dg``
    per element: step = -lr g' / (sqrt(1 - alpha) |g'| + eps) with g' = g + wd p, so |d step / d g'| = lr eps / (...)^2."""
    gt = g.double() + wd * p.double()
    den = (1 - alpha) ** 0.5 * gt.abs() + eps
    return -lr * gt / den, lr * eps / den ** 2


# ---- the fp32 reference's own gaps to float64, as tools/make_gru_goldens.py printed them (one thread), each relative to the
# tensor's largest magnitude; bar() of a tensor's own gap is that tensor's tolerance ----
OUT_GAP = {"in6_out1": 3.23e-7, "in12_out3": 3.56e-7}
GRAD_GAP = {
    "in6_out1": {"gru.weight_ih_l0": 1.83e-7, "gru.weight_hh_l0": 3.24e-7, "gru.bias_ih_l0": 1.56e-7, "gru.bias_hh_l0": 2.14e-7,
                 "gru2.weight_ih_l0": 1.49e-7, "gru2.weight_hh_l0": 2.57e-7, "gru2.bias_ih_l0": 9.94e-8, "gru2.bias_hh_l0": 2.88e-7,
                 "linear1.weight": 1.75e-7, "linear1.bias": 1.36e-7, "linear2.weight": 3.21e-7, "linear2.bias": 1.06e-7},
    "in12_out3": {"gru.weight_ih_l0": 3.09e-7, "gru.weight_hh_l0": 3.26e-7, "gru.bias_ih_l0": 2.80e-7, "gru.bias_hh_l0": 4.09e-7,
                  "gru2.weight_ih_l0": 1.30e-7, "gru2.weight_hh_l0": 3.00e-7, "gru2.bias_ih_l0": 8.40e-8, "gru2.bias_hh_l0": 2.97e-7,
                  "linear1.weight": 1.38e-7, "linear1.bias": 9.44e-8, "linear2.weight": 1.96e-7, "linear2.bias": 5.89e-8}}
# shapes that are not a golden's (other N, rows, O): the smaller of the two recorded gaps of each tensor
OUT_GAP_ANY = min(OUT_GAP.values())
GRAD_GAP_ANY = {k: min(GRAD_GAP[t][k] for t in GRAD_GAP) for k in KEYS}
# torch.nn.GRU in fp32 against gru_layer in float64, one layer with h0, dout on all rows and dh_last (same tool), per tensor:
#   short: seq 104, rows 16, T 12; long: seq 4096, rows 8, T 12
LAYER_GAP = {
    "short": {"out": 1.73e-7, "h_last": 1.66e-7, "dW_ih": 4.45e-7, "dW_hh": 3.40e-7, "db_ih": 1.05e-7, "db_hh": 3.25e-7, "dh0": 2.21e-7},
    "long": {"out": 1.27e-7, "h_last": 1.10e-7, "dW_ih": 4.28e-7, "dW_hh": 2.36e-6, "db_ih": 1.14e-7, "db_hh": 2.15e-6, "dh0": 1.69e-7}}


def check_stored(g, prefix, tensors, tol, what):
    """Every tensor against what the golden keeps of it: in full, or a sample of every 61st element with float64 row and column
    sums.  ``tol(k)``: the relative bar of tensor k (a share of the tensor's largest magnitude, so an absolute bound per element),
    or a per-element absolute bound as a tensor of its shape.  A row or column sum moves by at most the sum of what its elements
    may move by: its bound is the sum of their bounds."""
    import numpy as np
    for k in KEYS:
        t = tensors[k].detach().double().cpu()
        b = tol(k)
        if k in LARGE:
            if not isinstance(b, torch.Tensor):
                # the golden holds no full copy: the sample's largest magnitude stands for the tensor's (it is no larger)
                b = torch.full_like(t, b * float(np.abs(g[f"{prefix}{k}__s"]).max()))
            s, rs, cs = sample(t)
            triples = [(s, g[f"{prefix}{k}__s"], sample(b)[0]), (rs, g[f"{prefix}{k}__rs"], b.double().sum(1)),
                       (cs, g[f"{prefix}{k}__cs"], b.double().sum(0))]
        else:
            ref = np.asarray(g[f"{prefix}{k}"])
            triples = [(t, ref, b if isinstance(b, torch.Tensor) else b * float(np.abs(ref).max()))]
        for part, (got, ref, bound) in enumerate(triples):
            err = (got - torch.from_numpy(np.asarray(ref)).double()).abs()
            assert bool((err <= bound).all()), (what, k, part, float(err.max()))


def trajectory(tpims, g, forward):
    """Three windows accumulated as run.py::train() does: ``forward(x, y)`` gives a window's loss, whose gradients are left to
    add up on the leaves; returns the losses."""
    t_in, t_out, w = int(g["t_in"]), int(g["t_out"]), int(g["window"])
    losses = []
    for k in range(3):
        x = tpims["node_data"][:, :, w + k:w + k + t_in].contiguous()
        y = tpims["node_data"][:, -1, w + k + t_in:w + k + t_in + t_out].contiguous()
        loss = forward(x, y)
        loss.backward()
        losses.append(loss.item())
    return losses
