#!/usr/bin/env python3
"""Measure the bf16 arithmetic's per-row and per-node ratios on the GPU and write profiles/bf16_bars.txt.

For every case of tests/bf16_probe.py under every option set that changes its form (the runs of tests/test_gpu_bf16_bars.py): the forms
the dispatch restatement names, the worst per-node ratio of hidden and pred, and for every probe node and the dense probe the ratio
max |got - want64| / max |want64| of every parameter gradient, next to the bars (bf16_probe.BAR, derived on the host from the emulation).

    python tools/bf16_bars.py [--out profiles/bf16_bars.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bf16_probe as P  # noqa: E402
import regtgcn_amd as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_bars.txt"))
    args = ap.parse_args()
    R.load_library()
    table = P.bar_table()
    lines = ["# tools/bf16_bars.py: RegionalTemporalGCN / TemporalGCN under regt_set_gemm_mode(2), ratios of tests/bf16_probe.py against float64",
             "# bars (4 x the emulation's worst ratio, rounded up to a power of two): " +
             ", ".join(f"{k} {P.BAR[k]:.3e} (emulation {table[k][0]:.3e}, {table[k][1]})" for k in P.CLASSES),
             "# case | option set | forms | two runs | named | over the bar, then one line per row class / probe node and tensor: ratio [class]"]
    worst = {k: (0.0, "") for k in P.CLASSES}
    over = 0
    t0 = time.time()
    for name in P.CASES:
        for key in P.runs(name):
            m = P.measure(R, name, key)
            over += len(m["bad"])
            lines.append(f"{name} | {key} | {P.form_label(m['forms'])} | {'identical' if m['identical'] else 'DIFFER'} | {len(m['named'])} | {len(m['bad'])}")
            print(lines[-1], flush=True)
            for what, cls, r, ill in m["ratios"]:
                lines.append(f"    {what}: {r:.3e} [{cls}]{' ill-conditioned' if ill else ''}")
            for line in m["named"]:
                lines.append(f"    named: {line}")
            for b in m["bad"]:
                lines.append(f"    OVER: {b}")
            for cls, (r, where) in m["worst"].items():
                if r > worst[cls][0]:
                    worst[cls] = (r, where)
    for k in P.CLASSES:
        lines.append(f"# worst {k}: {worst[k][0]:.3e} ({worst[k][1]}), bar {P.BAR[k]:.3e}, emulation {table[k][0]:.3e}")
    lines.append(f"# rows and tensors over their bar: {over}; {time.time() - t0:.1f} s")
    print("\n".join(lines[-7:]))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
