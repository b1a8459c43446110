#!/usr/bin/env python3
"""Measure the cell's per-row ratios on the GPU and write profiles/cell_bars.txt.

For every case and probe of tests/cell_probe.py, in both fp32-storage arithmetics and under each data-gradient form that the
"dgrad1_gen" switch selects (the runs of tests/test_gpu_cell_bars.py): the forms the dispatch restatement names, the worst ratio
max_c |got - want64| / max_c |want64| over the well-conditioned rows of pred, hidden and dh_in next to the same ratio of the fp32
restatement (cell_probe.cell32), the per-element ratio of the blend probe, and the bars (cell_probe.BAR, derived on the host).

    python tools/cell_bars.py [--out profiles/cell_bars.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cell_probe as P  # noqa: E402
import regtgcn_amd as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_bars.txt"))
    args = ap.parse_args()
    R.load_library()
    lines = ["# tools/cell_bars.py: regt_cell_forward / regt_cell_backward through functional.CellFunction, per-row ratios of tests/cell_probe.py",
             "# bars: " + ", ".join(f"{k} {v:.3e}" for k, v in P.BAR.items()),
             "# case | probe | mode | dgrad1_gen | forms | tensor: HIP ratio / restatement ratio ... | blend per element | two runs | named rows | over the bar"]
    worst = {k: (0.0, "") for k in P.CLASSES}
    over = 0
    t0 = time.time()
    for name in P.CASES:
        for probe in P.PROBES:
            for mode, gen in P.runs(name):
                m = P.measure(R, name, probe, mode, gen)
                rest = P.restatement_ratios(name, probe)
                cells = []
                for tensor in ("pred", "hidden", "dh_in"):
                    r = m["ratios"][tensor]
                    cells.append(f"{tensor} {r:.3e} / {rest[tensor]:.3e}")
                    k = P.klass(tensor, probe)
                    if r > worst[k][0]:
                        worst[k] = (r, f"{name} {probe} mode {mode} dgrad1_gen {gen}")
                over += len(m["bad"])
                lines.append(f"{name} | {probe} | {mode} | {gen} | {P.form_label(m['forms'])} | {' | '.join(cells)} | "
                             f"{'-' if m['blend'] is None else format(m['blend'], '.3e')} | "
                             f"{'-' if m['identical'] is None else ('identical' if m['identical'] else 'DIFFER')} | {len(m['named'])} | {len(m['bad'])}")
                print(lines[-1], flush=True)
    for k in P.CLASSES:
        lines.append(f"# worst {k}: {worst[k][0]:.3e} ({worst[k][1]}), bar {P.BAR[k]:.3e}")
    lines.append(f"# rows over their bar: {over}; {time.time() - t0:.1f} s")
    print("\n".join(lines[-5:]))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
