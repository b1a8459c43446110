#!/usr/bin/env python3
"""Micro-benchmark of the fp32-MFMA GEMM entry points (regt_linear / regt_wgrad) at pipeline shapes.

    python tools/gemm_bench.py [MxKxN ...]
    python tools/gemm_bench.py slabs [M]      in-process A/B of the two wide fp32 weight gradients of the cell (dUh 256 x 256,
                                              dUz2|dUr2 512 x 256 with P in 512-wide rows) through regt_wgrad_slabs: option
                                              "wgrad_wave" 0 (wgrad3_kernel, one wave of three workgroups per CU) against 1 (the
                                              wave-owned kernel, one chunk per CU), alternating, five rounds of ten launches each
"""
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import regtgcn_amd as R


def timeit(fn, n=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / n


def _chunks(m, nch):
    kc = ((m + nch - 1) // nch + 31) // 32 * 32
    return kc, (m + kc - 1) // kc


def slabs_ab(m):
    import ctypes
    lib = R.load_library()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    q = torch.randn(m, 256, device="cuda")
    for name, nout in (("dUh", 256), ("dUzr", 512)):
        p = torch.randn(m, 512, device="cuda")[:, :nout]
        plans = {0: _chunks(m, cus * 3 // (nout // 128 * 2)), 1: _chunks(m, cus)}
        slab = torch.empty(max(nc for _, nc in plans.values()) * (nout * 256 + nout), device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        ms = {0: [], 1: []}
        for _ in range(5):
            for opt in (0, 1):
                kc, nc = plans[opt]
                ran = ctypes.c_char_p()
                prev = lib.regt_set_option(b"wgrad_wave", opt)
                fn = lambda: lib.regt_wgrad_slabs(p.data_ptr(), p.stride(0), nout, q.data_ptr(), 256, 256, m, kc, nc, 1, slab.data_ptr(), 1,
                                                  ctypes.byref(ran), st)
                ms[opt].append(timeit(fn))
                lib.regt_set_option(b"wgrad_wave", prev)
                ms[opt][-1] = (ms[opt][-1], ran.value.decode())
        for opt in (0, 1):
            t = sorted(v for v, _ in ms[opt])
            kc, nc = plans[opt]
            print(f"slabs {name} M={m} wgrad_wave={opt} kernel={ms[opt][0][1]} chunks={nc}x{kc}: min {t[0]:.3f} median {t[2]:.3f} max {t[-1]:.3f} ms  "
                  f"{2.0 * m * nout * 256 / t[2] / 1e9:6.1f} TFLOP/s (median)")
        del p


def main():
    R.load_library()
    if len(sys.argv) > 1 and sys.argv[1] == "slabs":
        return slabs_ab(int(sys.argv[2]) if len(sys.argv) > 2 else 1_200_000)
    shapes = [(1_200_000, 256, 512), (1_200_000, 256, 256), (150_000, 2048, 512), (75_000, 4096, 512), (1_200_000, 64, 256), (100_000, 256, 128)]
    if len(sys.argv) > 1:
        shapes = [tuple(int(v) for v in a.split('x')) for a in sys.argv[1:]]
    for m, k, n in shapes:
        a = torch.randn(m, k, device="cuda")
        w = torch.randn(n, k, device="cuda") / 16
        b = torch.randn(n, device="cuda")
        ms = timeit(lambda: R.ops.linear(a, w, b, 1))
        print(f"linear  M={m:8d} K={k:4d} N={n:4d}: {ms:8.3f} ms  {2.0*m*k*n/ms/1e9:7.1f} TFLOP/s")
        if n <= 512 and k <= 256:
            d = torch.randn(m, n, device="cuda")
            ms = timeit(lambda: R.ops.wgrad(d, a))
            print(f"wgrad   M={m:8d} N={n:4d} K={k:4d}: {ms:8.3f} ms  {2.0*m*k*n/ms/1e9:7.1f} TFLOP/s")
        del a, w, b


if __name__ == "__main__":
    main()
