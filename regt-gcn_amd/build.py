"""Build libregtgcn_hip.so (gfx950 only) in-tree with hipcc.

    python regt-gcn_amd/build.py [--force]

The library has no torch dependency: plain HIP + the C ABI of include/regtgcn.h.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.environ.get("REGT_LIB_DIR") or os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libregtgcn_hip.so")
SOURCES = ["api_runtime.hip", "api_layout.hip", "api_step.hip", "api_model.hip", "api_cell0.hip", "api_ops.hip", "api_baselines.hip", "options.hip", "gemm_fwd.hip", "gemm_cell.hip", "gemm_dispatch.hip", "gemm_small.hip", "wgrad_dispatch.hip", "wgrad_fp32.hip", "wgrad_bf16.hip", "wgrad_reduce.hip", "pack.hip", "spmm_dispatch.hip", "spmm_csr.hip", "spmm_panel.hip", "graph.hip", "cell.hip", "cell_dx.hip", "model_dx.hip", "spmm_dual_t.hip", "window.hip", "window_bwd.hip", "gat.hip", "fused.hip", "fused_rows.hip", "embed.hip", "spatial.hip", "stnorm.hip", "stid.hip", "gru.hip", "staeformer.hip", "staeformer_bwd.hip", "staeformer_train.hip"]
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join("..", "..", "include", "regtgcn.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
# developer switches, e.g. REGT_HIPCC_FLAGS=-DREGT_WG_TRACE (workgroup phase trace, tools/wg_trace.py)
FLAGS += os.environ.get("REGT_HIPCC_FLAGS", "").split()


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(LIBDIR, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs = []
    procs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(LIBDIR, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            cmd = [hipcc] + FLAGS + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((src, subprocess.Popen(cmd)))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")
    if force or procs or _stale(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
