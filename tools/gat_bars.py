#!/usr/bin/env python3
"""Measure the per-row ratios of tests/gat_math.py on the GPU and write profiles/gat_bars.txt.

For every case of gat_math.CASES (the cases of tests/test_gpu_gat_bars.py) and every class (d, m, l, out, D, dd, ds): the kernel
instantiation the pick_group restatement expects, the worst r of the HIP kernels against the sparse float64 reference, the same r
of the fp32 restatement evaluated on the host, the class's bar and the row where the HIP kernels are worst.  The bars (4 x the
worst restatement ratio of a class, rounded up to a power of two) are stated in tests/gat_math.py.

    python tools/gat_bars.py [--out profiles/gat_bars.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import gat_math as G  # noqa: E402
import regtgcn_amd as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gat_bars.txt"))
    args = ap.parse_args()
    R.load_library()
    rows = []
    for c in G.CASES:
        inp = G.inputs(c)
        sel = G.case_rows(c, G.cpu_pattern(inp.ei, c.n))
        pat, got, _ = G.run_hip(R, c, inp, *sel)
        ref = G.reference(inp, pat, *sel)
        restated = G.ratios(ref, G.restate(inp, pat, *sel))
        for cls, label, kernel, r, where in G.measure(c, inp, pat, ref, got):
            rows.append((cls, label, kernel, r, restated[cls][0], where))
    lines = [f"# per-row ratios of the kernels of csrc/gat.hip on {torch.cuda.get_device_name(0)}",
             "# (tools/gat_bars.py; classes, statistic and bars: tests/gat_math.py)",
             f"# {'class':<4} {'HIP r':>10} {'fp32 restatement r':>19} {'bar':>10}  case [kernels], worst row of the HIP kernels"]
    for cls, label, kernel, r, r32, where in rows:
        lines.append(f"{cls:<6} {r:>10.3e} {r32:>19.3e} {G.BAR[cls]:>10.3e}  {label} [{kernel}], {where}")
    lines.append("#")
    for cls in G.CLASSES:
        sel = [r for r in rows if r[0] == cls]
        hip = max(sel, key=lambda r: r[3])
        ref = max(sel, key=lambda r: r[4])
        lines.append(f"# {cls}: worst HIP r {hip[3]:.3e} ({hip[1]} [{hip[2]}]); worst restatement r {ref[4]:.3e} ({ref[1]}); "
                     f"bar {G.BAR[cls]:.3e}; over the bar: {sum(1 for r in sel if not r[3] <= G.BAR[cls])}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-len(G.CLASSES) - 1:]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
