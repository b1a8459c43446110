#!/usr/bin/env python3
"""The window sum's bar table (tests/window_bars.py): the fp32 restatement's worst ratio per case on the CPU and, where a GPU is
present, the HIP kernel's own.  python tools/window_bars.py > profiles/window_bars.txt"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import window_bars as W  # noqa: E402

rows, bar = W.bar_table()
hip = {}
if torch.cuda.is_available():
    import regtgcn_amd as R
    for case in W.CASES:
        ring, att = W.inputs(case)
        want, den = W.reference64(ring, att, case)
        head = [t.cuda() for t in W.head_inputs(case[1])]
        _, hidden = R.ops.window_forward(ring.cuda(), case[4], case[5], att.cuda(), *head)
        hip[case] = W.ratio(hidden.cpu(), want, den)
print("window sum (csrc/window.hip): |got - want64| / sum_p |prob_p ring term|, worst over every output element")
print(f"{'case (N, C, T, ring_len, first_slot, windows)':<50} {'restatement':<12}" + ("HIP kernel (MI355X)" if hip else ""))
for case, r in rows:
    print(f"{str(case):<50} {r:.2e}" + (f"     {hip[case]:.2e}" if hip else ""))
worst = max(r for _, r in rows)
print(f"worst restatement {worst:.2e}  x 4, rounded up: 2 ** {int(math.log2(bar))} ({bar:.2e}) = BAR_WINDOW" + (
    f"; worst HIP {max(hip.values()):.2e}" if hip else ""))
