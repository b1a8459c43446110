"""Measure the bars of tests/grad_bars.py: for every case of tests/test_gpu_grad_scale.py and every gradient block,
max|hip - want64| / max|want64| under both fp32-storage arithmetics and every switch setting of the case, next to the same
ratio of the fp32 oracle -- want64 is the float64 oracle.  Run on the GPU box from the repo root:

    python tools/grad_scale_bars.py > profiles/grad_scale_bars.txt

The last lines give the worst ratio per class and the constant that follows from it (x 4, rounded up to a power of two)."""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import grad_bars as B                       # noqa: E402
import test_gpu_grad_scale as T             # noqa: E402


def main():
    import regtgcn_amd as R
    R.load_library()
    torch.manual_seed(1234)
    worst = {}                              # (class, column) -> (ratio, where)
    print("# ratio = max|got - want64| / max|want64| per gradient block; want64 = float64 oracle; loss = mse(pred, y) + mean(hidden^2)")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    for name, (_build, settings) in T.CASES.items():
        case, want64 = T.case_and_want64(name)
        cols = [("oracle_fp32", case.oracle_grads(torch.float32))]
        for sw in settings:
            tag = "".join(f",{o.decode()}={v}" for o, v in sw)
            for arith, aname in ((0, "fp32mfma"), (1, "bf16x3")):
                cols.append((f"hip_{aname}{tag}", T.hip_grads_under(R, case, arith, sw)))
        rows = [B.block_ratios(g, want64, case.num_regions) for _c, g in cols]
        print(f"\n== {name}")
        print(f"{'block':64s} {'class':9s} {'max|want64|':>11s} " + " ".join(f"{c:>24s}" for c, _g in cols))
        for i, (_n, label, cls, _err, scale) in enumerate(rows[0]):
            cells = []
            for (cname, _g), r in zip(cols, rows):
                err = r[i][3]
                if scale == 0.0:
                    cells.append(f"{'exact 0' if err == 0.0 else 'NONZERO %.2e' % err:>24s}")
                    ratio = 0.0 if err == 0.0 else math.inf
                else:
                    ratio = err / scale
                    cells.append(f"{ratio:24.2e}")
                key = (cls, "oracle_fp32" if cname == "oracle_fp32" else "hip")
                if ratio > worst.get(key, (-1.0, ""))[0]:
                    worst[key] = (ratio, f"{name} {label} {cname}")
            print(f"{label:64s} {cls:9s} {scale:11.2e} " + " ".join(cells))
    print("\n== worst ratio per class")
    for (cls, col), (ratio, where) in sorted(worst.items()):
        line = f"{cls:9s} {col:11s} {ratio:.3e}  at {where}"
        if col == "hip" and 0.0 < ratio < math.inf:
            line += f"   -> x4, next power of two: 2^{math.ceil(math.log2(4.0 * ratio))} = {2.0 ** math.ceil(math.log2(4.0 * ratio)):.3e}"
        print(line)
    print(f"REL in tests/grad_bars.py: " + ", ".join(f"{k} = {v:.3e}" for k, v in B.REL.items()))


if __name__ == "__main__":
    main()
