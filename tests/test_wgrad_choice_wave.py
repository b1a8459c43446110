"""When a weight gradient runs on the wave-owned fp32 kernel (csrc/wgrad_dispatch.hip wgrad_pick -> wgrad_wave_kernel) and how its
row chunks are sized, pinned without a GPU.  tests/wgrad_wave_plan/wave_plan.hip links the three weight-gradient units compiled
host-only with tests/wgrad_plan/launch_log.h forced in, as tests/test_wgrad_plan_cpu.py does, on a stand-in device of 256 CUs."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "regt-gcn_amd", "csrc")
UNITS = ["wgrad_dispatch.hip", "wgrad_fp32.hip", "wgrad_bf16.hip"]
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CUS, MIN_CHUNK_ROWS, SLAB = 256, 128 * 32, 32          # the row gate: every CU a chunk of 128 slabs
M_CFG3, M_MIN = 1_200_000, CUS * MIN_CHUNK_ROWS

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found: the recorder cannot be built")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wave_plan") / "wave_plan")
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-I", CSRC, "-include",
           os.path.join(ROOT, "tests", "wgrad_plan", "launch_log.h"), os.path.join(ROOT, "tests", "wgrad_wave_plan", "wave_plan.hip")]
    cmd += [os.path.join(CSRC, u) for u in UNITS] + ["-Wl,--unresolved-symbols=ignore-all", "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    picks, chunks = {}, {}
    for line in res.stdout.splitlines():
        m = re.match(r"pick (\w+): .*?regt::(\w+).*? grid=(\d+) lds=(\d+)$", line)
        if m:
            picks[m.group(1)] = (m.group(2), int(m.group(3)), int(m.group(4)))
            continue
        m = re.match(r"chunks (\d+) (\d+): ok=(\d) kchunk=(-?\d+) nchunks=(-?\d+) pool=(\d+) min_rows=(\d+)$", line)
        assert m, line
        chunks[(int(m.group(1)), int(m.group(2)))] = tuple(int(v) for v in m.groups()[2:])
    return picks, chunks


def test_chosen_for_the_wide_gradients_at_large_m(plan):
    picks, _ = plan
    lds = 2 * 2 * 32 * (256 + 4) * 4                   # two stages of a 32-row slab of both operands, rows of 260 floats
    assert picks["dUh_cfg3"] == ("wgrad_wave_kernel", CUS, lds)
    assert picks["dUzr_cfg3"] == ("wgrad_wave_kernel", 2 * CUS, lds)
    assert picks["dUh_min"] == ("wgrad_wave_kernel", CUS, lds)
    assert picks["dUzr_min"] == ("wgrad_wave_kernel", 2 * CUS, lds)
    assert picks["dUzr_window"] == ("wgrad_wave_kernel", 2 * CUS, lds)      # an operand inside wider rows, 16-byte aligned


@pytest.mark.parametrize("case,kernel", [
    ("small_m", "wgrad3_kernel"), ("tpims_m", "wgrad3_kernel"), ("f_wide_rhs", "wgrad_kernel"), ("f64_rhs", "wgrad3_kernel"),
    ("nin128", "wgrad3_kernel"), ("nout384", "wgrad3_kernel"), ("misaligned_p", "wgrad_kernel_generic"),
    ("misaligned_q", "wgrad_kernel_generic"), ("layout_chunks", "wgrad3_kernel"), ("option_off", "wgrad3_kernel"),
    ("option_off_dUzr", "wgrad3_kernel"), ("wide_core", "wgrad_kernel"), ("bf16x3", "wgrad_split_kernel"),
    ("bf16_operands", "wgrad_bf16_ring_kernel")])
def test_everything_else_keeps_its_kernel(plan, case, kernel):
    assert plan[0][case][0] == kernel, plan[0][case]


def test_option_off_restores_the_parents_chunks(plan):
    """wgrad3_kernel on one wave of three workgroups per CU: 768 / 4 and 768 / 8 chunks of 128 x 128 tiles."""
    picks, _ = plan
    assert picks["option_off"][1] == 768 and picks["option_off_dUzr"][1] == 768


@pytest.mark.parametrize("nout", [256, 512])
@pytest.mark.parametrize("M", [M_CFG3, M_MIN, M_MIN + 1, 3 * M_MIN + 12345, 40_000_000])
def test_chunks_tile_m_and_fit_the_slab_budget(plan, nout, M):
    ok, kc, nc, pool, min_rows = plan[1][(nout, M)]
    assert ok == 1 and min_rows == M_MIN
    assert kc % SLAB == 0 and kc >= MIN_CHUNK_ROWS and kc <= 32768
    assert (nc - 1) * kc < M <= nc * kc                                   # the chunks tile M exactly, none empty
    # the launch's slabs (one per chunk, with their column sums) fit what make_layout reserves for the regions of dUh and dUzr -- one
    # pool (ReduceQueue::take refuses a launch that does not fit it and reduces what is queued before it hands out a region again)
    assert nc * (nout * 256 + nout) <= pool
    assert nc * (nout // 256) * 64 >= CUS * 63                            # workgroups for all but one CU in 64 at least
    if M <= 32768 * CUS:
        assert nc <= CUS


@pytest.mark.parametrize("nout", [256, 512])
def test_below_the_smallest_m_the_chunker_refuses(plan, nout):
    assert plan[1][(nout, M_MIN - 1)][0] == 0
