#!/usr/bin/env python3
"""Measure the regional embedding's per-element ratios on the GPU and write profiles/embed_bars.txt.

For every form and layout of tests/embed_probe.py (the cases of tests/test_gpu_embed_bars.py): the kernel the dispatch restatement
selects, whether the ``exact`` family's h equals the expected bits, the worst ratio of the ``full`` family against float64 next to the
same ratio of the host restatement (op_bars.linear_restatement in the form's arithmetic), and the bar (op_bars.BAR, unchanged).

    python tools/embed_bars.py [--out profiles/embed_bars.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import embed_probe as E  # noqa: E402
import op_bars as B  # noqa: E402
import regtgcn_amd as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embed_bars.txt"))
    args = ap.parse_args()
    R.load_library()
    lines = ["# tools/embed_bars.py: h = leaky_relu(x A0^T + (L~ x) A_region^T + b') read through the probe of tests/embed_probe.py",
             "# form | layout (N, T, regions) | kernel selected | exact family | full family: worst HIP r | restatement r | bar"]
    for form, (mode, _opts, f, c, lays) in E.FORMS.items():
        for lay in lays:
            m = E.measure(R, form, lay)
            p = E.probe(lay, f, c)
            h = p.restatement("full", mode)
            r_ref = p.full_ratio(B.bf16_round(h) if mode == 2 else h, rounded=mode == 2, stored_bf16=mode == 2)
            lines.append(f"{form} | {lay} ({p.n}, {p.t}, {p.R}) | {m['stage']} | {'equal' if m['exact'] else 'DIFFERS'} | "
                         f"{m['full']:.3e} | {r_ref:.3e} | {m['bar']:.3e}")
            print(lines[-1], flush=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
