"""Cases, block maps and GPU runners of the whole-STAEformer training tests (test helper only).

Bars are those of grad_bars.py (REL, CAP, ill_conditioned) through stae_layer_bars.assert_blocks' rule; no bar value is introduced
here.  Classes: ``default`` -- output_proj.* and the op-level output-projection gradients; ``attention`` -- everything upstream of an
attention: the embedding parameters, attn.FC_Q / FC_K / FC_V, row gradients; ``norm`` -- the rest of a layer
(stae_layer_bars.grad_class).  Blocks: weights per 32 x 32 quadrant, adaptive_embedding / node_emb per 64-node tile, tables per table
row, output_proj.weight per time step (D columns), vectors whole.  Each layer's attn.FC_K.bias takes its scale from
staeformer_train_math.key_bias_scales.  A block that is exactly zero in float64 must be exactly zero.

Seeds: model cases draw x features from seed 900 + B + T + N (feature 1 in [0, 1), feature 2 in {0..4}), dout standard normal, the
parameters from ``model_state`` (seed 11: default-style initialisers, biases and LayerNorm parameters perturbed), keep words from
seed 77 + sites."""
import functools

import torch

import stae_layer_bars as LB
from grad_bars import CAP, REL, ill_conditioned
from staeformer_train_math import key_bias_scales, model_grads, pack_keep

K_GAP = LB.K_GAP
QUAD, TILE = 32, 64
DEV = "cuda:0"
SENTINEL = -777.0


def grad_class(name: str) -> str:
    if name.startswith("output_proj.") or name in ("dw", "db", "dx_proj"):
        return "default"
    if name.startswith(("attn_layers_t.", "attn_layers_s.")):
        return LB.grad_class(name.split(".", 2)[2])
    if name in ("dz", "dy", "dgamma", "dbeta"):
        return "norm"
    return "attention"          # input_proj.*, tod / dow tables, node_emb, adaptive_embedding, row gradients


def blocks(name: str, t: torch.Tensor, model_dim: int):
    if t.dim() == 1:
        return [(name, t)]
    if name in ("output_proj.weight", "dw"):
        return [(f"{name}[step {s}]", t[:, s * model_dim:(s + 1) * model_dim].reshape(-1)) for s in range(t.shape[1] // model_dim)]
    if name == "adaptive_embedding":
        return [(f"{name}[nodes {a}:{a + TILE}]", t[:, a:a + TILE].reshape(-1)) for a in range(0, t.shape[1], TILE)]
    if name == "node_emb":
        return [(f"{name}[nodes {a}:{a + TILE}]", t[a:a + TILE].reshape(-1)) for a in range(0, t.shape[0], TILE)]
    if name in ("tod_embedding.weight", "dow_embedding.weight"):
        return [(f"{name}[row {r}]", t[r]) for r in range(t.shape[0])]
    if name in ("dx_proj", "dz", "dy"):
        r = t.reshape(-1, t.shape[-1])
        return [(f"{name}[rows {a}:{a + TILE}]", r[a:a + TILE].reshape(-1)) for a in range(0, r.shape[0], TILE)]
    assert t.dim() == 2, (name, tuple(t.shape))
    return [(f"{name}[{a}:{a + QUAD}, {c}:{c + QUAD}]", t[a:a + QUAD, c:c + QUAD].reshape(-1)) for a in range(0, t.shape[0], QUAD)
            for c in range(0, t.shape[1], QUAD)]


def assert_blocks(got, want64, ref32, what, model_dim, scales=None, rel=REL, max_ill=0.05):
    """stae_layer_bars.assert_blocks' rule on this model's names, and at most ``max_ill`` of the blocks may be ill-conditioned (held to
    the K_GAP bar instead of their class's).  Returns (ill-conditioned labels, number of blocks)."""
    bad, ill, n, worst = [], [], 0, {}
    for name, want in want64.items():
        w = want.detach().cpu().double()
        g, r = got[name].detach().cpu().double(), ref32[name].detach().cpu().double()
        assert g.shape == w.shape == r.shape, (name, tuple(g.shape), tuple(w.shape), tuple(r.shape))
        cls = grad_class(name)
        for (label, eb), (_, wb), (_, gb) in zip(blocks(name, (g - w).abs(), model_dim), blocks(name, w.abs(), model_dim),
                                                 blocks(name, (r - w).abs(), model_dim)):
            n += 1
            err, gap = float(eb.max()), float(gb.max())
            scale = scales[name] if scales and name in scales else float(wb.max())
            if ill_conditioned(cls, scale, gap):
                ill.append(label)
                if not err <= K_GAP * gap:
                    bad.append(f"{label} [{cls}, ill-conditioned]: max|err| {err:.3e} > {K_GAP} x {gap:.3e}")
            else:
                if scale > 0:
                    worst[cls] = max(worst.get(cls, 0.0), err / scale)
                if not err <= rel[cls] * scale:             # (NaN fails; scale 0 demands err 0)
                    bad.append(f"{label} [{cls}]: max|err| {err:.3e} vs scale {scale:.3e} > {rel[cls]:.3e}")
    print(f"{what}: {n} blocks, {len(ill)} ill-conditioned, worst ratio " + ", ".join(f"{c} {v:.3e} (bar {rel[c]:.3e})" for c, v in sorted(worst.items())))
    assert not bad, f"{what}: {len(bad)} gradient block(s) off their own scale:\n  " + "\n  ".join(bad[:40])
    assert len(ill) <= max_ill * n, f"{what}: {len(ill)} of {n} blocks are ill-conditioned (at most {max_ill:.0%} may be): {ill[:10]}"
    return ill, n


forward_bar = LB.forward_bar


# ---- cases ----------------------------------------------------------------------------------------------------------------------

LN_M, LN_D, LN_P = (1, 15, 16, 17, 65), (32, 128, 256), 0.1
EMBED_SHAPES = [(1, 1, 1), (3, 4, 7), (2, 2, 65)]
EMBED_WIDTHS = [(24, 0, 24, 0, 80), (32, 32, 16, 16, 32), (32, 0, 0, 0, 0)]      # (E, tod, dow, S, A)
EMBED_F, EMBED_CIN, EMBED_SPD, EMBED_DPW = 8, 3, 12, 7
PROJ_CASES = [(1, 1, 1, 32, 1, 1), (2, 4, 7, 128, 3, 1), (1, 6, 65, 128, 1, 1), (2, 3, 33, 256, 4, 2), (1, 2, 5, 32, 64, 1)]   # B T N D O C
# (B, T, N, num_layers, dropout, constructor keywords)
MODEL_CASES = {"small": (2, 4, 7, 1, 0.0, dict(input_embedding_dim=32, tod_embedding_dim=32, dow_embedding_dim=16, spatial_embedding_dim=16,
                                                adaptive_embedding_dim=32, feed_forward_dim=64, num_heads=4, steps_per_day=12)),
               "drop": (1, 6, 33, 2, 0.1, dict(tod_embedding_dim=0, feed_forward_dim=64))}


def model_kwargs(name):
    b, t, n, layers, p, kw = MODEL_CASES[name]
    return dict(num_nodes=n, in_steps=t, out_steps=2, num_layers=layers, dropout=p, **kw)


def model_state(shapes, seed=11):
    """{key: tensor} for the (key, shape) list of a state_dict: uniform(-1, 1) / sqrt(fan_in) matrices, perturbed biases and LayerNorm."""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in shapes:
        if ".ln" in key:
            sd[key] = (1.0 if key.endswith("weight") else 0.0) + 0.5 * (torch.rand(shape, generator=gen) - 0.5)
        elif key.endswith("bias"):
            sd[key] = 0.4 * (torch.rand(shape, generator=gen) - 0.5)
        else:
            sd[key] = (torch.rand(shape, generator=gen) * 2 - 1) / shape[-1] ** 0.5
    return sd


def features(b, t, n, f, gen, spd, wild=False, nan=False):
    """x (B, T, N, F): feature 1 a time of day in [0, 1), feature 2 a day in {0 .. 4} (row 5 is never hit).  ``wild``: a few negative and
    too-large entries in both index columns; ``nan``: NaN ones too (they would poison an input projection that reads the column)."""
    x = torch.randn(b, t, n, f, generator=gen)
    x[..., 1] = torch.randint(0, max(1, spd - 1), (b, t, n), generator=gen) / spd + 0.25 / spd
    x[..., 2] = torch.randint(0, 5, (b, t, n), generator=gen).float()
    if wild and b * t * n < 8:
        x.view(-1, f)[0, 1], x.view(-1, f)[0, 2] = (float("nan") if nan else -0.5), 99.0
    if wild and b * t * n >= 8:
        flat = x.view(-1, f)
        flat[0, 1], flat[1, 1], flat[3, 2], flat[4, 2] = -0.5, 3.0, -2.0, 99.0
        if nan:
            flat[2, 1] = flat[5, 2] = float("nan")
    return x


def state_shapes(kw):
    """(key, shape) in state_dict order for STAEformer(**kw), from the reference's parameter creation order."""
    d = kw.get("input_embedding_dim", 24) + kw.get("tod_embedding_dim", 24) + kw.get("dow_embedding_dim", 24) + \
        kw.get("spatial_embedding_dim", 0) + kw.get("adaptive_embedding_dim", 80)
    n, t, ff = kw["num_nodes"], kw["in_steps"], kw.get("feed_forward_dim", 256)
    out = []
    if kw.get("spatial_embedding_dim", 0):
        out.append(("node_emb", (n, kw["spatial_embedding_dim"])))
    if kw.get("adaptive_embedding_dim", 80):
        out.append(("adaptive_embedding", (t, n, kw.get("adaptive_embedding_dim", 80))))
    out += [("input_proj.weight", (kw.get("input_embedding_dim", 24), kw.get("input_dim", 3))), ("input_proj.bias", (kw.get("input_embedding_dim", 24),))]
    if kw.get("tod_embedding_dim", 24):
        out.append(("tod_embedding.weight", (kw.get("steps_per_day", 288), kw["tod_embedding_dim"])))
    if kw.get("dow_embedding_dim", 24):
        out.append(("dow_embedding.weight", (kw.get("days_per_week", 7), kw.get("dow_embedding_dim", 24))))
    out += [("output_proj.weight", (kw["out_steps"] * kw.get("output_dim", 1), t * d)), ("output_proj.bias", (kw["out_steps"] * kw.get("output_dim", 1),))]
    for kind in "ts":
        for i in range(kw["num_layers"]):
            pre = f"attn_layers_{kind}.{i}."
            for m in ("FC_Q", "FC_K", "FC_V", "out_proj"):
                out += [(pre + f"attn.{m}.weight", (d, d)), (pre + f"attn.{m}.bias", (d,))]
            out += [(pre + "feed_forward.0.weight", (ff, d)), (pre + "feed_forward.0.bias", (ff,)), (pre + "feed_forward.2.weight", (d, ff)),
                    (pre + "feed_forward.2.bias", (d,))]
            out += [(pre + f"ln{j}.{w}", (d,)) for j in (1, 2) for w in ("weight", "bias")]
    return out, d


@functools.lru_cache(maxsize=None)
def model_case(name):
    """x, dout, state_dict, keep words (or None) with the float64 and fp32 restatements (out, gradients) and the key-bias scales."""
    b, t, n, layers, p, _ = MODEL_CASES[name]
    kw = model_kwargs(name)
    shapes, d = state_shapes(kw)
    sd = model_state(shapes)
    gen = torch.Generator().manual_seed(900 + b + t + n)
    x = features(b, t, n, 8, gen, kw.get("steps_per_day", 288))
    dout = torch.randn(b, kw["out_steps"], n, 1, generator=gen)
    keep = None
    if p > 0:
        kg = torch.Generator().manual_seed(77 + 4 * layers)
        keep = pack_keep(torch.rand(4 * layers, b * t * n, d, generator=kg) >= p)
    o64, _, g64 = model_grads(sd, x, kw["out_steps"], keep=keep, drop=p, dout=dout)
    o32, _, g32 = model_grads(sd, x, kw["out_steps"], keep=keep, drop=p, dout=dout, dtype=torch.float32)
    scales = key_bias_scales(sd, x, kw["out_steps"], keep=keep, drop=p, dout=dout)
    return {"x": x, "dout": dout, "sd": sd, "keep": keep, "kw": kw, "dim": d, "scales": scales}, (o64, g64), (o32, g32)


def ill_fraction(got, want64, ref32, model_dim, scales=None):
    """(ill-conditioned blocks, blocks) decided by the references alone."""
    ill = n = 0
    for name, want in want64.items():
        w, r = want.detach().double(), ref32[name].detach().double()
        cls = grad_class(name)
        for (_, wb), (_, gb) in zip(blocks(name, w.abs(), model_dim), blocks(name, (r - w).abs(), model_dim)):
            n += 1
            scale = scales[name] if scales and name in scales else float(wb.max())
            ill += bool(ill_conditioned(cls, scale, float(gb.max())))
    return ill, n


# ---- runners on the GPU -----------------------------------------------------------------------------------------------------------

def make_model(case, cls=None):
    import regtgcn_amd as R
    mod = (cls or R.STAEformerTrainable)(**case["kw"])
    mod.load_state_dict(case["sd"], strict=True)
    return mod.to(DEV).train()


def run_model_backward(mod, x, dout, keep=None):
    mod.zero_grad(set_to_none=True)
    out = mod(x.to(DEV), keep=None if keep is None else keep.to(DEV))
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), {k: p.grad for k, p in mod.named_parameters()}


# ---- the reference's train-mode records (tools/make_staeformer_train_goldens.py) ----------------------------------------------------

GOLDEN_RECORDS = ("r0", "r1")


@functools.lru_cache(maxsize=None)
def golden_case(tag):
    """One record of tests/golden/golden_staeformer_train.npz with the float64 and fp32 restatements on its inputs: (case, (out, losses,
    gradients) recorded by the reference, the same in float64, in fp32).  Gradient dictionaries hold the record's ``grad_keys`` only
    (r0 leaves out the twelve 2-D layer weights, for the file's size)."""
    import os

    import numpy as np

    from staeformer_math import golden_state_dict
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_staeformer_train.npz"))
    sd = golden_state_dict(g)
    x, y, p = torch.from_numpy(g["x"]), torch.from_numpy(g["y"]), float(g["p"]) if tag == "r1" else 0.0
    keep = torch.from_numpy(g["r1__keep"]) if tag == "r1" else None
    keys = [str(k) for k in g[f"{tag}__grad_keys"]]
    kw = dict(num_nodes=int(g["nodes"]), in_steps=int(g["t_in"]), out_steps=int(g["t_out"]), tod_embedding_dim=0, num_layers=1,
              feed_forward_dim=int(g["feed_forward_dim"]), dropout=p)
    rec = (torch.from_numpy(g[f"{tag}__out"]), torch.from_numpy(g[f"{tag}__loss"]), {k: torch.from_numpy(g[f"{tag}__g__{k}"]) for k in keys})
    pick = lambda r: (r[0], r[1], {k: r[2][k] for k in keys})
    r64 = pick(model_grads(sd, x, kw["out_steps"], keep=keep, drop=p, y=y))
    r32 = pick(model_grads(sd, x, kw["out_steps"], keep=keep, drop=p, y=y, dtype=torch.float32))
    scales = key_bias_scales(sd, x, kw["out_steps"], keep=keep, drop=p, y=y)
    return {"x": x, "y": y, "sd": sd, "keep": keep, "kw": kw, "dim": 128, "scales": scales, "p": p}, rec, r64, r32
