"""The launch plan of the training step (csrc/api_step.hip), pinned without a GPU.

tests/step_plan/step_plan.hip links api_step.hip and api_layout.hip compiled host-only and stands in for every launcher, predicate
and side-stream call: each launch becomes one line of text -- its name, the PROF stage it runs under, its stream and every field
the kernel would read, pointers as arena+offset.  tests/golden/step_plan.txt holds, per case and launch, the name and a 64-bit hash
of that text.  It was recorded from api_step.hip as it was BEFORE the step was restated as named stages, and did not change
with that refactor: the sequence of launches, their arguments and streams, the side_fork / side_join / side_resync positions, the
slab offsets (order and sizes of ReduceQueue::take), the order of the reduce and composition tasks and the stage names are the same.

The twenty cases (all_cases() in step_plan.hip, named after what they vary) run forward and backward each at N = 40 nodes: fp32
regional at F = 32 / 8, R = 1, overlapping regions, a region shard, a wide head, no attention gradient, each data-gradient form,
bf16x3, TemporalGCN collapsed / uncollapsed, the bf16 forms, the cell path, a forward-only call, a minimal slab region.  Notes:
  * 18 (cell path) sets regional = 0, R = 1 and no region tables: regt_cell_forward / _backward accept nothing else.
  * 20 (slab region = the largest single request) flushes mid-pass at three takes, so no batch of it reaches WR_MAX_TASKS; the batch
    that passes WR_MAX_TASKS (13 reductions) is case 4, the same step on the full slab region.
  * Profiling is ON in the recorder (hipEventCreate / hipEventRecord are its own stand-ins): that is how a launch knows its stage.
The recorder's predicates and chunk rules are stand-ins, so this pins the step's host logic given their answers, not the kernels'
own limits.  On a mismatch the full text of the first differing launch is printed; compare it with the same launch of the
recorder built against the other version of the file (`step_plan --full`)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "regt-gcn_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "step_plan.txt")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found: the recorder cannot be built")


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_plan") / "step_plan")
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-I", CSRC,
           os.path.join(ROOT, "tests", "step_plan", "step_plan.hip"), os.path.join(CSRC, "api_step.hip"),
           os.path.join(CSRC, "api_layout.hip"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    return exe


def _run(exe, *args):
    res = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return res.stdout.splitlines()


def test_launch_plan_is_what_it_was(recorder):
    got = _run(recorder)
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        case = next((line for line in reversed(got[:k + 1]) if line.startswith("case ")), "(no case)")
        full = _run(recorder, "--full")
        print("first difference at line %d, in %s" % (k + 1, case))
        print("recorded: %s" % (want[k] if k < len(want) else "(end of file)"))
        print("now:      %s" % (got[k] if k < len(got) else "(end of output)"))
        print("now, in full: %s" % (full[k] if k < len(full) else "(end of output)"))
    assert got == want


def test_every_stage_of_the_step_is_reached(recorder):
    """Every PROF name of api_step.hip (and the queue's wgrad_reduce) occurs in at least one case, every case ran both passes without an
    error, and there are twenty of them."""
    out = _run(recorder)
    cases = [line.split() for line in out if line.startswith("case ")]
    assert len(cases) == 20
    assert all(c[2:5] == ["rc", "0", "0"] for c in cases), cases
    assert not any(" set_error " in line for line in out)
    reached = set(out[-1].split()[1:])
    assert out[-1].startswith("stages ")
    with open(os.path.join(CSRC, "api_step.hip")) as f:
        src = f.read()
    # (the weight-gradient stages reach PROF through a helper's `name` parameter; comments quote option names the same way)
    named = set(re.findall(r'PROF\("(\w+)"', src)) | set(re.findall(r'(?<!set_option\()"(wgrad_\w+)"', src)) | {"wgrad_reduce"}
    assert len(named) >= 29, sorted(named)
    assert named <= reached, sorted(named - reached)
