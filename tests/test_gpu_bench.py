"""bench.py's result line: a plain run measures the headline only and writes the outputs of its timed steps with --dump-outputs;
--full adds the per-stage table, the roofline and the other GEMM arithmetics."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*args):
    res = subprocess.run([sys.executable, "bench.py", "--workload", "small", "--warmup", "1"] + list(args), cwd=ROOT,
                         capture_output=True, text=True, timeout=500)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_its_outputs(tmp_path):
    out = _bench("--steps", "3", "--dump-outputs", str(tmp_path))
    for k in HEADLINE:
        assert k in out, k
    assert out["steps"] == 3 and out["dtype"] == "fp32" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and out["value"] * out["ms_per_step"] == pytest.approx(1000.0)
    for k in ("stages", "roofline", "opt_in_bf16x3_split", "opt_in_bf16", "cpu_baseline"):
        assert k not in out, k
    files = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    for name, a in files.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
    assert files["pred"].shape == (20_000, 1)
    assert files["hidden"].ndim == 1 and 0 < files["hidden"].size <= 1 << 20      # (20 000, 256) written as a fixed sample
    assert float(files["loss"]) == pytest.approx(out["config"]["final_loss"], rel=1e-6)
    grads = [n for n in files if n.startswith("grad.")]
    assert len(grads) > 10 and all("param." + n[len("grad."):] in files for n in grads)
    assert any(float(np.abs(files[n]).max()) > 0 for n in grads)


def test_full_run_adds_stages_roofline_and_other_arithmetics():
    out = _bench("--steps", "2", "--full", "--no-cpu-baseline")
    for k in HEADLINE + ("stages", "roofline", "opt_in_bf16x3_split", "opt_in_bf16"):
        assert k in out, k
    assert out["config"]["ms_per_step_with_stage_events"] > 0
