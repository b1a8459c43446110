"""Which kernel an aggregation, a snapshot pack or a row conversion runs on (csrc/spmm_dispatch.hip spmm_pick, the launch entries of
spmm_csr.hip / spmm_panel.hip, the launchers of pack.hip), pinned without a GPU.

tests/spmm_plan/spmm_plan.hip links the four units compiled host-only with tests/spmm_plan/launch_log.h forced in: every
hipLaunchKernelGGL becomes one line of text -- the kernel's full name as the compiler spells it, grid, block, dynamic LDS bytes and
every argument of the launch -- and every refusal its return code and error text.  tests/golden/spmm_plan.txt was recorded with the
same recorder and shim from csrc/spmm.hip as it was BEFORE it was cut into units and its three statements of the kernel choice
became spmm_pick (the build line is in the recorder's header), so the golden is not taken from the code under test.

The cases (all_cases() in spmm_plan.hip) are the smallest arguments that reach each choice: the pack launchers on each side of
F % 4, F * T = 4096, pointer alignment and their block caps; every rung of both lane-group ladders at its upper edge and one
float4 past it, column passes with a short last pass; the panel gate on each side of each condition; nstack 1 and 2; 128- and
256-byte panels by W4 % 16, by the slice bound and by spmm_pl; spmm_rows 0 / 1 with each clause of the row-block eligibility
failing in turn; the halo form; the bf16 form's own bounds; every refusal."""
import os
import re
import shutil
import subprocess

import pytest

import op_bars as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "regt-gcn_amd", "csrc")
PLAN = os.path.join(ROOT, "tests", "spmm_plan")
GOLDEN = os.path.join(ROOT, "tests", "golden", "spmm_plan.txt")
UNITS = ["pack.hip", "spmm_dispatch.hip", "spmm_csr.hip", "spmm_panel.hip"]
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found: the recorder cannot be built")


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spmm_plan") / "spmm_plan")
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-I", CSRC, "-include", os.path.join(PLAN, "launch_log.h"),
           os.path.join(PLAN, "spmm_plan.hip")] + [os.path.join(CSRC, u) for u in UNITS] + ["-Wl,--unresolved-symbols=ignore-all", "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    return exe


def _run(exe, *args):
    res = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return res.stdout.splitlines()


@pytest.fixture(scope="module")
def plan(recorder):
    return _run(recorder)


def test_kernel_choice_is_what_it_was(plan):
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    for k, (a, b) in enumerate(zip(plan, want)):
        if a != b:
            print("first difference at line %d\nrecorded: %s\nnow:      %s" % (k + 1, b, a))
            break
    assert plan == want


def _short(name):
    """'void regt::spmm_rows_kernel<16, true, false>(int const*, ...)' -> 'spmm_rows_kernel<16,true,false>'"""
    name = re.sub(r"\(.*\)$", "", name.strip())
    return name.replace("void ", "").replace("regt::", "").replace(" ", "")


def test_every_kernel_and_every_refusal_is_reached(plan):
    """The 33 kernels of the digest of the units (profiles/spmm_units_isa.txt) all occur, and every REGT_CHECK_ARG text of spmm_pick
    and of the pack / convert launchers is the error of some case."""
    assert plan[-1].startswith("kernels ")
    kernels = set(_short(k) for k in plan[-1][len("kernels"):].split(";") if k.strip())
    expected = {"pack_x_kernel", "pack_x_lds_kernel", "pack_x_bf16_kernel", "pack_x_bf16_lds_kernel", "cvt_rows_bf16_kernel"}
    expected |= {"spmm_csr_kernel<%d,%d>" % t for t in ((8, 1), (16, 1), (32, 1), (64, 1), (32, 3), (64, 2), (64, 3), (64, 4), (64, 8))}
    expected |= {"spmm_dual_csr_kernel<%d,%d>" % t for t in ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 8))}
    expected |= {"spmm_panel_kernel<%d>" % pl for pl in (8, 16)}
    expected |= {"spmm_dual_panel_kernel<%d,%d>" % (pl, pl) for pl in (8, 16)}
    expected |= {"spmm_dual_panel_bf16_kernel<%d,%d>" % (pl, pl) for pl in (8, 16)}
    expected |= {"spmm_rows_kernel<%d,%s>" % (pl, f) for pl in (8, 16) for f in ("false,false", "true,false", "true,true")}
    assert len(expected) == 33
    assert kernels == expected, (sorted(expected - kernels), sorted(kernels - expected))
    texts = []
    with open(os.path.join(CSRC, "spmm_dispatch.hip")) as f:
        src = f.read()
    pick = src[src.index("int spmm_pick("):src.index("static int pick_and_launch(")]
    assert "set_error(" not in pick
    texts += re.findall(r'REGT_CHECK_ARG\(.*?, "([^"]*)"', pick, flags=re.S)
    assert len(texts) == 11, texts
    with open(os.path.join(CSRC, "pack.hip")) as f:
        pack = re.findall(r'REGT_CHECK_ARG\(.*?, "([^"]*)"', f.read(), flags=re.S)
    assert len(pack) == 2, pack
    errors = [line.split(" error: ", 1)[1] for line in plan if " error: " in line]
    # a text with conversions is matched as a pattern: each %d stands for an integer
    for t in texts + pack:
        pat = re.compile("^" + re.escape(t).replace("%d", "-?[0-9]+") + "$")
        assert any(pat.match(e) for e in errors), t
    for e in errors:
        assert any(re.match("^" + re.escape(t).replace("%d", "-?[0-9]+") + "$", e) for t in texts + pack), e
    assert all(" rc=1 " in line for line in plan if " error: " in line)


def test_python_restatement_agrees(recorder, tmp_path):
    """tests/op_bars.py::expected_kernel names, for every spmm case its tables enumerate, the kernel the launchers pick."""
    cases = []
    for w in B.SPMM_WIDTHS:
        cases.append(("spmm_csr", (B.SPMM_N, B.SPMM_N, w), 0))
    for w in B.DUAL_WIDTHS:
        cases.append(("spmm_dual", (B.SPMM_N, w), 0))
    for rows in (0, 1):
        for w in B.LARGE_WIDTHS:
            cases.append(("spmm_csr", (B.LARGE_N, B.LARGE_N, w), rows))
            cases.append(("spmm_csr", (2 * B.LARGE_N, B.LARGE_N, w), rows))
            cases.append(("spmm_dual", (B.LARGE_N, w), rows))
        for w in B.LARGE_BF16_WIDTHS:
            cases.append(("spmm_dual_bf16", (B.LARGE_N, B.LARGE_N, w), rows))
    lines = []
    for i, (op, shape, rows) in enumerate(cases):
        if op == "spmm_csr":              # regt_spmm_csr (api_ops.hip) passes nstack = 1
            lines.append("c%d csr %d %d %d 1 %d 0" % ((i,) + shape + (rows,)))
        elif op == "spmm_dual":           # regt_spmm_dual: x_rows = n
            lines.append("c%d dual %d %d %d %d 0" % (i, shape[0], shape[0], shape[1], rows))
        else:
            lines.append("c%d bf16 %d %d %d %d 0" % ((i,) + shape + (rows,)))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    out = _run(recorder, "--cases", str(path))
    assert len(out) == len(cases)
    seen = set()
    for (op, shape, rows), line in zip(cases, out):
        assert " error: " not in line, line
        launches = line.split(": ", 1)[1].split(" | ")
        names = set(_short(l.split(" grid=")[0]) for l in launches)
        assert len(names) == 1, line
        got = names.pop() + ("/column-pass" if len(launches) > 1 else "")
        want = B.expected_kernel(op, 0, shape, {"spmm_rows": rows})
        assert got == want, (op, shape, rows, got, want)
        seen.add(got)
    # the enumeration is the one table_kernels() makes: together the cases reach every spmm name of KERNELS
    assert seen == set(B.KERNELS["spmm_csr"]) | set(B.KERNELS["spmm_dual"]) | set(B.KERNELS["spmm_dual_bf16"])
