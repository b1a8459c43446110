"""Measure the bars that tests/grad_bars.py holds the STNorm, STID and SpatialGCN gradients to: for every gradient comparison of
tests/test_gpu_stnorm.py, test_gpu_stid.py and test_gpu_spatial.py (goldens, restatement cases, cfg-3 shapes, the kernel pair's
shapes) and every gradient block, max|hip - want64| / max|want64_block| next to the same ratio of the fp32 restatement --
want64 is the float64 restatement.  Run on the GPU box from the repo root:

    python tools/baseline_grad_bars.py > profiles/baseline_grad_bars.txt

One line per tensor, showing its worst block (a cfg-3 case alone has 25 000 blocks); '!' marks a block that the fp32 restatement
makes ill-conditioned (grad_bars.ill_conditioned), which is held to its fp32 gap and stays out of the worst ratios.  The last
lines give the two worst well-conditioned blocks per model and class and the constant that follows (x 4, rounded up to a power of
two)."""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grad_bars as B                       # noqa: E402
import test_gpu_spatial as SP               # noqa: E402
import test_gpu_stid as SI                  # noqa: E402
import test_gpu_stnorm as SN                # noqa: E402
from conftest import load_npz               # noqa: E402

DEV = "cuda:0"
worst = {}                                  # (model, class) -> [(hip ratio, fp32 ratio, where)]


def report(model, case, got, g64, g32, **kw):
    rows = B.conditioned_rows(got, g64, g32, **kw)
    print(f"\n== {model} {case}: {len(rows)} blocks")
    print(f"{'tensor: worst block':78s} {'class':7s} {'blocks':>6s} {'max|want64|':>11s} {'hip':>9s} {'fp32':>9s}")
    per_tensor = {}
    for label, cls, err, scale, gap, excess in rows:
        name = label.split("[")[0]
        if scale == 0.0:
            ratio, r32 = (0.0 if err == 0.0 else math.inf), (0.0 if gap == 0.0 else math.inf)
        else:
            ratio, r32 = max(excess, 0.0) / scale, gap / scale
        ill = B.ill_conditioned(cls, scale, gap)
        if not ill:
            worst.setdefault((model, cls), []).append((ratio, r32, f"{case} {label}"))
        cur = per_tensor.get(name)
        per_tensor[name] = (cur[0] + 1, max(cur[1], (ratio, label, cls, scale, r32, ill))) if cur else (1, (ratio, label, cls, scale, r32, ill))
    for name, (count, (ratio, label, cls, scale, r32, ill)) in per_tensor.items():
        print(f"{label:78s} {cls:7s} {count:6d} {scale:11.2e} {ratio:9.2e} {r32:9.2e}{' !' if ill else ''}")


def hip_grads(mod):
    torch.cuda.synchronize()
    return {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in mod.named_parameters()}


def stnorm():
    for tag in SN.TAGS:
        g, keys = SN._golden(tag)
        mod = SN._module(g, keys).train()
        x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
        torch.mean((mod(x) - y) ** 2).backward()
        report("stnorm", f"golden-{tag}", hip_grads(mod), *SN.golden_case(tag))
    for kw in SN.RESTATEMENT_CASES + [SN.CFG3_CASE]:
        c = SN.restatement_case(**kw)
        mod = c["mod"].to(DEV).train(c["training"])
        out = mod(c["x"].to(DEV), tnorm_group=c["tnorm_group"])
        (out * c["w"].to(DEV)).sum().backward()
        report("stnorm", " ".join(f"{k}={v}" for k, v in kw.items()), hip_grads(mod), c["g64"], c["g32"])


def stid():
    for tag in SI.TAGS:
        g, keys = SI._golden(tag)
        mod = SI._module(g, keys).train()
        x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
        torch.mean((mod(x, keep=torch.from_numpy(g["train__keep"]).to(DEV)) - y) ** 2).backward()
        report("stid", f"golden-{tag}", hip_grads(mod), *SI.golden_case(tag), input_dim=3)
    for kw in SI.RESTATEMENT_CASES + [SI.CFG3_CASE]:
        c = SI.restatement_case(**kw)
        mod = c["mod"].to(DEV).train(c["keep"] is not None)
        out = mod(c["x"].to(DEV), keep=None if c["keep"] is None else SI.pack_keep(c["keep"]).to(DEV))
        (out * c["w"].to(DEV)).sum().backward()
        report("stid", " ".join(f"{k}={v}" for k, v in kw.items()), hip_grads(mod), c["g64"], c["g32"], input_dim=c["input_dim"])


def spatial():
    import regtgcn_amd as R
    tpims = {k: torch.from_numpy(v) for k, v in load_npz("tpims_fixture.npz").items() if v.ndim > 0}
    for tag in ("in6_out1", "in12_out3"):
        for mode in ("eval", "train"):
            g, params = SP._golden(tag)
            t_in, t_out, w0 = int(g["t_in"]), int(g["t_out"]), int(g["window"])
            x = tpims["node_data"][:, :, w0:w0 + t_in].contiguous().cuda()
            y = tpims["node_data"][:, -1, w0 + t_in:w0 + t_in + t_out].contiguous().cuda()
            mod = R.SpatialGCN(8, t_in, t_out)
            mod.load_state_dict(params, strict=True)
            mod = mod.cuda().train(mode == "train")
            op = mod.prepare_graph(tpims["edge_index"].cuda(), tpims["edge_attr"].cuda(), x.shape[0])
            keep = torch.from_numpy(g["train__keep"]).cuda() if mode == "train" else None
            pred, _hidden = mod.forward_prepared(x, op, keep=keep)
            torch.mean((pred - y) ** 2).backward()
            report("spatial", f"golden-{tag}-{mode}", hip_grads(mod), *SP.golden_case(tpims, tag, mode))
    shapes = [(n, t, f, SP.kernel_pair_inputs(R, n, t, f)) for n, t, f in SP.KERNEL_PAIR_SHAPES]
    n, e, t, f = 100_000, 1_000_000, 12, 32
    g = R.data.synthetic_regional_graph(n, e, 5, seed=31)
    shapes.append((n, t, f, (g.edge_index, g.edge_attr) + SP._inputs(n, t, f, seed=32)))
    for n, t, f, (ei, ea, x, w0, w1, b, ds) in shapes:
        for masked in (False, True):
            if n == 100_000 and not masked:
                continue
            keep = R.nn.draw_keep_mask(n * t, "cuda") if masked else None
            _s, grads = SP._embed_gpu(R, x, ei, ea, w0, w1, b, keep, ds)
            _ref, g64, g32, allow = SP.embed_case(x, ei, ea, w0, w1, b, keep, ds)
            report("spatial", f"kernel pair n={n} t={t} f={f} {'train' if masked else 'eval'}", dict(zip(SP.EMBED_NAMES, (v.cpu() for v in grads))),
                   g64, g32, allow=allow)


def main():
    import regtgcn_amd as R
    R.load_library()
    torch.manual_seed(1234)
    print("# ratio = max|got - want64| / max|want64| per gradient block; want64 = float64 restatement; hip = the kernels, fp32 = the fp32 restatement")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    stnorm()
    stid()
    spatial()
    print("\n== the two worst well-conditioned blocks per model and class")
    by_class = {}
    for (model, cls), entries in sorted(worst.items()):
        entries.sort(reverse=True)
        for ratio, r32, where in entries[:2]:
            print(f"{model:8s} {cls:8s} hip {ratio:.3e}  fp32 {r32:.3e}  at {where}")
        by_class[cls] = max(by_class.get(cls, 0.0), entries[0][0])
    for cls, ratio in sorted(by_class.items()):
        if 0.0 < ratio < math.inf:
            e = math.ceil(math.log2(4.0 * ratio))
            print(f"{cls:8s} worst {ratio:.3e}   -> x4, next power of two: 2^{e} = {2.0 ** e:.3e}   (cap {B.CAP[cls]:.0e})")
    print("REL in tests/grad_bars.py: " + ", ".join(f"{k} = {v:.3e}" for k, v in B.REL.items()))


if __name__ == "__main__":
    main()
