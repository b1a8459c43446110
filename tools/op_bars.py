#!/usr/bin/env python3
"""Measure the per-element ratios of tests/op_bars.py on the GPU and write profiles/op_bars.txt.

For every case of the tables of tests/op_bars.py (the cases of tests/test_gpu_op_bars.py): the kernel name the dispatch restatement
expects, r = max |got - want64| / sum|terms| of the HIP kernel, the same r of the fp32 restatement evaluated on the host, and the
class's bar.  The bars (4 x the worst restatement ratio of a class, rounded up to a power of two) are stated in tests/op_bars.py.

    python tools/op_bars.py [--out profiles/op_bars.txt]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import op_bars as B  # noqa: E402
import regtgcn_amd as R  # noqa: E402


def rows_of_gemm(lib):
    rows = []
    for mode in B.MODES:
        lib.regt_set_gemm_mode(mode)
        for shape, acts in B.LINEAR_CASES:
            rows += B.linear_case(shape, acts, mode, hip=lambda a, w, b, act: R.ops.linear(a.cuda(), w.cuda(), b.cuda(), act))
        for k, n in B.IDENTITY_CASES:
            rows += B.identity_case(k, n, mode, hip=lambda a, w: R.ops.linear(a.cuda(), w.cuda()))[0]
        for shape in B.WGRAD_CASES:
            for wb in (True, False):
                rows += B.wgrad_case(shape, mode, wb, hip=lambda d, a, wb: R.ops.wgrad(d.cuda(), a.cuda(), wb))
        if mode == 1:
            for shape in B.SENSITIVE_LINEAR:
                rows += B.linear_case(shape, (0,), 1, hip=lambda a, w, b, act: R.ops.linear(a.cuda(), w.cuda(), b.cuda(), act),
                                      inputs=B.split_sensitive_inputs)
            for shape in B.SENSITIVE_WGRAD:
                rows += B.wgrad_case(shape, 1, False, hip=lambda d, a, wb: R.ops.wgrad(d.cuda(), a.cuda(), wb), inputs=B.wgrad_sensitive_inputs)
    lib.regt_set_gemm_mode(0)
    return rows


def child_rows(modes, opt):
    """The shapes of the environment-only switches, in this process (started by main with the variable set)."""
    lib = R.load_library()
    rows = []
    for mode in modes:
        lib.regt_set_gemm_mode(mode)
        for shape in B.CHILD_SHAPES:
            rows += B.linear_case(shape, (0, 3), mode, hip=lambda a, w, b, act: R.ops.linear(a.cuda(), w.cuda(), b.cuda(), act), options=opt)
        if opt.get("fp32_core_wide"):
            for shape in B.CHILD_WGRAD_SHAPES:
                rows += B.wgrad_case(shape, mode, True, hip=lambda d, a, wb: R.ops.wgrad(d.cuda(), a.cuda(), wb), options=opt)
    return rows


def rows_of_children():
    rows = []
    for env, modes, opt in (({"REGT_FP32_CORE": "wide"}, "0", "fp32_core_wide"), ({"REGT_GEMM_DESC": "table"}, "0,1,2", "desc_table")):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", modes, opt], env=dict(os.environ, **env),
                             capture_output=True, text=True, check=True)
        for ln in res.stdout.splitlines():
            if ln.startswith("ROW "):
                cls, label, name, r_hip, r_ref = ln[4:].split("|")
                rows.append((cls, f"{label} ({'='.join(*env.items())})", name, float(r_hip), float(r_ref)))
    return rows


def rows_of_spmm(lib):
    rows = []

    def both(label, name, cls, got, val, x, cpu, ratio=B.spmm_ratio, store=False):
        rp, col = cpu[0], cpu[1]
        ref = B.csr_reference(rp, col, val.cpu(), x.cpu())
        s32 = B.spmm_restatement(rp, col, val.cpu(), x.cpu())
        rows.append((cls, label, name, ratio(got.cpu(), ref), ratio(s32.to(torch.bfloat16) if store else s32, ref)))

    cpu = B.graph(B.SPMM_N)
    rp, col, va, vl = (t.cuda() for t in cpu)
    for w in B.SPMM_WIDTHS:
        x = B.spmm_x(B.SPMM_N, w).cuda()
        name = B.expected_kernel("spmm_csr", 0, (B.SPMM_N, B.SPMM_N, w))
        for tag, val in (("A", va), ("L", vl)):
            both(f"spmm_csr n {B.SPMM_N} width {w} {tag}", name, "spmm", R.ops.spmm_csr(rp, col, val, x), val, x, cpu)
    for w in B.DUAL_WIDTHS:
        x = B.spmm_x(B.SPMM_N, w).cuda()
        name = B.expected_kernel("spmm_dual", 0, (B.SPMM_N, w))
        ya, yl = R.ops.spmm_dual(rp, col, va, vl, x)
        for tag, y, val in (("A", ya, va), ("L", yl, vl)):
            both(f"spmm_dual n {B.SPMM_N} width {w} {tag}", name, "spmm", y, val, x, cpu)
    n = B.LARGE_N
    cpu = B.graph(n, B.HUB)
    rp, col, va, vl = (t.cuda() for t in cpu)
    srp, scol, sval = B.stacked(rp, col, va, vl)
    for on in (0, 1):
        opt = {"spmm_rows": on}
        prev = lib.regt_set_option(b"spmm_rows", on)
        try:
            for w in B.LARGE_WIDTHS:
                x = B.spmm_x(n, w).cuda()
                both(f"spmm_csr n {n} width {w} L", B.expected_kernel("spmm_csr", 0, (n, n, w), opt), "spmm", R.ops.spmm_csr(rp, col, vl, x), vl, x, cpu)
                st = R.ops.spmm_csr(srp, scol, sval, x)
                k2 = B.expected_kernel("spmm_csr", 0, (2 * n, n, w), opt)
                both(f"spmm_csr stacked 2 x {n} width {w} A", k2, "spmm", st[:n], va, x, cpu)
                both(f"spmm_csr stacked 2 x {n} width {w} L", k2, "spmm", st[n:], vl, x, cpu)
                ya, yl = R.ops.spmm_dual(rp, col, va, vl, x)
                kd = B.expected_kernel("spmm_dual", 0, (n, w), opt)
                both(f"spmm_dual n {n} width {w} A", kd, "spmm", ya, va, x, cpu)
                both(f"spmm_dual n {n} width {w} L", kd, "spmm", yl, vl, x, cpu)
            for w in B.LARGE_BF16_WIDTHS:
                x = B.spmm_x(n, w, bf16=True).cuda()
                if not on:      # the fp32 dual kernel on the same bf16 values: what the stored rows are compared with bit for bit
                    fa, fl = R.ops.spmm_dual(rp, col, va, vl, x.float().contiguous())
                    kf = B.expected_kernel("spmm_dual", 0, (n, w))
                    both(f"spmm_dual n {n} width {w} (bf16 values) A", kf, "spmm", fa, va, x, cpu)
                    both(f"spmm_dual n {n} width {w} (bf16 values) L", kf, "spmm", fl, vl, x, cpu)
                ya, yl = R.ops.spmm_dual_bf16(rp, col, va, vl, x)
                kb = B.expected_kernel("spmm_dual_bf16", 0, (n, n, w), opt)
                both(f"spmm_dual_bf16 n {n} width {w} A", kb, "bf16_store", ya, va, x, cpu, B.bf16_store_ratio, True)
                both(f"spmm_dual_bf16 n {n} width {w} L", kb, "bf16_store", yl, vl, x, cpu, B.bf16_store_ratio, True)
        finally:
            lib.regt_set_option(b"spmm_rows", prev)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "op_bars.txt"))
    ap.add_argument("--child", nargs=2, metavar=("MODES", "OPTION"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        for row in child_rows([int(m) for m in args.child[0].split(",")], {args.child[1]: 1}):
            print("ROW " + "|".join(str(v) for v in row))
        return
    lib = R.load_library()
    rows = rows_of_gemm(lib) + rows_of_children() + rows_of_spmm(lib)
    lines = [f"# per-element ratios r = max |got - want64| / sum|terms| of the op-site kernels on {torch.cuda.get_device_name(0)}",
             "# (tools/op_bars.py; classes, statistic and bars: tests/op_bars.py)",
             f"# {'class':<11} {'HIP r':>10} {'fp32 restatement r':>19} {'bar':>10}  case [kernel]"]
    for cls, label, name, r_hip, r_ref in rows:
        lines.append(f"{cls:<13} {r_hip:>10.3e} {r_ref:>19.3e} {B.BAR[cls]:>10.3e}  {label} [{name}]")
    lines.append("#")
    for cls in B.BAR:
        sel = [r for r in rows if r[0] == cls]
        hip = max(sel, key=lambda r: r[3])
        ref = max(sel, key=lambda r: r[4])
        lines.append(f"# {cls}: worst HIP r {hip[3]:.3e} ({hip[1]} [{hip[2]}]); worst restatement r {ref[4]:.3e} ({ref[1]}); "
                     f"bar {B.BAR[cls]:.3e}; over the bar: {sum(1 for r in sel if not r[3] <= B.BAR[cls])}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-len(B.BAR) - 1:]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
