"""Measure the ratios that tests/stae_layer_bars.py holds the STAEformer self-attention layer's gradients to: for every gradient
comparison of tests/test_gpu_stae_backward.py (the attention backward and the add+LayerNorm backward at op level, the layer on the
golden and on the restatement cases, with the runners of tests/stae_layer_bars.py) and every block, max|hip - want64| / scale next
to the same ratio of the fp32 restatement -- want64 is the float64 restatement, scale the block's own float64 maximum (attn.FC_K.bias: the magnitude of what it sums,
stae_layer_math.key_bias_scale).  Run on the GPU box from the repo root:

    python tools/stae_backward_bars.py > profiles/stae_backward_bars.txt

One line per case and class with its worst well-conditioned block; '!' counts the blocks that the fp32 restatement makes
ill-conditioned (grad_bars.ill_conditioned), which are held to their fp32 gap and stay out of the worst ratios.  The last lines give
the worst block per class over all cases, that ratio x 4 and the class's REL and CAP from tests/grad_bars.py: a worst ratio x 4 over
REL is a finding about the kernel's summation order, never a reason to widen a bar."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grad_bars as B                       # noqa: E402
import stae_layer_bars as S                 # noqa: E402
from conftest import load_npz               # noqa: E402
from stae_layer_math import key_bias_scale, layer_grads  # noqa: E402
from staeformer_math import golden_state_dict  # noqa: E402

worst = {}                                  # class -> (hip ratio, fp32 ratio, where)


def report(case, got, g64, g32, axis=None, scales=None):
    rows = S.block_rows(got, g64, g32, axis, scales)
    per = {}
    for label, cls, err, scale, gap in rows:
        cur = per.setdefault(cls, [0, 0, (-1.0, 0.0, "")])
        cur[0] += 1
        if B.ill_conditioned(cls, scale, gap):
            cur[1] += 1
        elif scale > 0:
            cur[2] = max(cur[2], (err / scale, gap / scale, label))
            if err / scale > worst.get(cls, (-1.0,))[0]:
                worst[cls] = (err / scale, gap / scale, f"{case} {label}")
    for cls, (count, ill, (ratio, r32, label)) in sorted(per.items()):
        print(f"{case:44s} {cls:9s} {count:5d} {ill:3d}! {ratio:9.2e} {r32:9.2e}  {label}")


def main():
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"{'case':44s} {'class':9s} {'blocks':>5s} {'ill':>4s} {'hip':>9s} {'fp32':>9s}  worst well-conditioned block")
    for length, axis, heads, batch, scale in [c + (1.0,) for c in S.ATTN_CASES] + [c + (30.0,) for c in S.LARGE_SCORE_CASES]:
        case, r64, r32 = S.attention_case(length, axis, heads, batch, scale)
        _, _, _, (gbuf,) = S.run_attention(case, heads, axis)
        report(f"attention L {length} axis {axis} heads {heads} B {batch}" + (" q x 30" if scale != 1.0 else ""), S.attention_grads_of(gbuf, case, heads),
               S.attention_grad_dicts(r64), S.attention_grad_dicts(r32), axis=axis)
    for m, d, kind in [(m, d, "normal") for m, d in S.LN_CASES] + [(65, 32, "constant_row"), (65, 256, "constant_row"), (65, 128, "gamma_zeros")]:
        case, r64, r32 = S.layernorm_case(m, d, kind)
        _, grads = S.run_layernorm(case)
        report(f"add_layernorm M {m} D {d} {kind}", grads, S.layernorm_grad_dicts(r64), S.layernorm_grad_dicts(r32))
    g = load_npz("golden_stae_layer.npz")
    sd = golden_state_dict(g)
    x, dout = torch.from_numpy(g["x"]), torch.from_numpy(g["dout"])
    for dim in (1, 2):
        mod = S.make_layer(sd, int(g["model_dim"]), int(g["num_heads"]), int(g["feed_forward_dim"]))
        _, grads = S.run_layer_backward(mod, x, dim, dout)
        _, g64 = layer_grads(sd, x, dim, dout)
        report(f"golden layer dim {dim} (fp32: the reference)", grads, g64, {k: torch.from_numpy(g[f"dim{dim}__grad__{k}"]) for k in g64},
               scales={"attn.FC_K.bias": key_bias_scale(sd, x, dim, dout)})
    for b, t, n in S.LAYER_SHAPES:
        for axis in (1, 2):
            case, r64, r32 = S.layer_case(b, t, n, axis)
            mod = S.make_layer(case["sd"])
            _, grads = S.run_layer_backward(mod, case["x"], axis, case["dout"])
            report(f"layer B {b} T {t} N {n} axis {axis}", grads, r64[1], r32[1], scales=case["scales"])
    print()
    for cls, (ratio, r32, where) in sorted(worst.items()):
        print(f"{cls:9s} worst {ratio:.3e} (fp32 restatement there {r32:.3e}) at {where}: x 4 = {4 * ratio:.3e}; REL {B.REL[cls]:.3e}, CAP {B.CAP[cls]:.0e}"
              f" -> {'within REL' if 4 * ratio <= B.REL[cls] else 'OVER REL: a finding about the summation order'}")


if __name__ == "__main__":
    main()
