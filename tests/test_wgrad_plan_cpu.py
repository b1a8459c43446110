"""Which kernel a weight gradient runs on (csrc/wgrad_dispatch.hip wgrad_pick and the launchers of wgrad_fp32.hip / wgrad_bf16.hip),
pinned without a GPU.

tests/wgrad_plan/wgrad_plan.hip links the three units compiled host-only with tests/wgrad_plan/launch_log.h forced in: every
hipLaunchKernelGGL becomes one line of text -- the kernel's full name as the compiler spells it, grid, dynamic LDS bytes, whether
the kernel's LDS limit was asked for, all_csum -- and every refusal its error text.  tests/golden/wgrad_plan.txt was recorded with
the same recorder and shim from csrc/wgrad.hip as it was BEFORE it was cut into units and its launch ladder restated as wgrad_pick
(the build line is in the recorder's header), so the golden is not taken from the code under test.

The cases (all_cases() in wgrad_plan.hip) are the smallest arguments that reach each choice: the three arithmetics with and without
the wide fp32 core at Nin <= 32, 33-64 (wgrad_bnw64 on / off), > 64 and rows that are no multiple of 4; operands stored as bf16; the
two-part right-hand side with the split inside a 64-column tile, on and off a 128-column boundary, and with q_relu; wgrad_ring
0 / 4 / 6 / 8, wgrad_tile 128 / 256 with Nout % 256 zero and not, wgrad_ring256 2 / 4; a chunk whose rows x row bytes reach 2^31;
one case per refusal."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "regt-gcn_amd", "csrc")
PLAN = os.path.join(ROOT, "tests", "wgrad_plan")
GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_plan.txt")
UNITS = ["wgrad_dispatch.hip", "wgrad_fp32.hip", "wgrad_bf16.hip"]
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found: the recorder cannot be built")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wgrad_plan") / "wgrad_plan")
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-I", CSRC, "-include", os.path.join(PLAN, "launch_log.h"),
           os.path.join(PLAN, "wgrad_plan.hip")] + [os.path.join(CSRC, u) for u in UNITS] + ["-Wl,--unresolved-symbols=ignore-all", "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return res.stdout.splitlines()


def test_kernel_choice_is_what_it_was(plan):
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    for k, (a, b) in enumerate(zip(plan, want)):
        if a != b:
            print("first difference at line %d\nrecorded: %s\nnow:      %s" % (k + 1, b, a))
            break
    assert plan == want


def test_every_kernel_and_every_refusal_is_reached(plan):
    """The 17 GEMM kernels of the two kernel units (the 19 of the digest minus the two reduce kernels) all occur, and every
    REGT_CHECK_ARG text of wgrad_pick is the error of some case."""
    kernels = set(k.strip() for k in plan[-1][len("kernels"):].split(";") if k.strip())
    assert plan[-1].startswith("kernels ")
    expected = {"regt::wgrad3_kernel"}
    expected |= {"void regt::wgrad_kernel<%s>(regt::WgradArgs)" % t for t in ("32, false", "32, true", "64, false", "128, false")}
    expected |= {"void regt::wgrad_kernel_generic<%d>(regt::WgradArgs)" % t for t in (32, 128)}
    expected |= {"void regt::wgrad_split_kernel<%s>(regt::WgradArgs)" % t
                 for t in ("3, false, false", "1, false, false", "1, false, true", "1, true, false", "1, true, true")}
    expected |= {"void regt::wgrad_bf16_ring_kernel<%s>(regt::WgradArgs)" % t for t in ("4, 2", "6, 2", "8, 2", "2, 4", "4, 4")}
    assert len(expected) == 17
    assert kernels == expected, (sorted(expected - kernels), sorted(kernels - expected))
    with open(os.path.join(CSRC, "wgrad_dispatch.hip")) as f:
        src = f.read()
    pick = src[src.index("int wgrad_pick("):]
    texts = [t.replace("%%", "%") for t in re.findall(r'REGT_CHECK_ARG\(.*?"(wgrad: [^"]*)"\);', pick, flags=re.S)]
    assert len(texts) == 8, texts
    errors = [line.split(" error: ", 1)[1] for line in plan if " error: " in line]
    assert set(texts) == set(errors), (sorted(set(texts) - set(errors)), sorted(set(errors) - set(texts)))
    assert all(" rc=1 " in line for line in plan if " error: " in line)
