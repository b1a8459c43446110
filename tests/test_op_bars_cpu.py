"""Host proof of tests/op_bars.py: the fp32 restatement of every op passes its own bar against float64 on every case of the GPU
tables, the bars are 4 x the worst restatement ratio rounded up to a power of two, planted corruptions exceed their class's bar by at
least 2 x (the ones the former absolute bars accepted are listed in OLD_BARS_ACCEPT), and the tables reach every kernel name."""
import pytest
import torch

import op_bars as B

SMALL = 600


@pytest.fixture(scope="module")
def restated():
    """{class: [(label, kernel name, r)]} of the restatements over every case of the GPU tables: with and without the bias gradient,
    the identity cases, the non-cancelling inputs, the shapes of the environment-switch children (under their switches) and both
    operators at every width."""
    out = {c: [] for c in B.BAR}

    def add(rows):
        for cls, label, name, _, r in rows:
            out[cls].append((label, name, r))

    for mode in B.MODES:
        for shape, acts in B.LINEAR_CASES:
            add(B.linear_case(shape, acts, mode))
        for k, n in B.IDENTITY_CASES:
            add(B.identity_case(k, n, mode)[0])
        for shape in B.CHILD_SHAPES:
            add(B.linear_case(shape, (0, 3), mode, options={"desc_table": 1}))
        for shape in B.WGRAD_CASES:
            for wb in (True, False):
                add(B.wgrad_case(shape, mode, wb))
    for shape in B.SENSITIVE_LINEAR:
        add(B.linear_case(shape, (0,), 1, inputs=B.split_sensitive_inputs))
    for shape in B.SENSITIVE_WGRAD:
        add(B.wgrad_case(shape, 1, False, inputs=B.wgrad_sensitive_inputs))
    for shape in B.CHILD_SHAPES:
        add(B.linear_case(shape, (0, 3), 0, options={"fp32_core_wide": 1}))
    for shape in B.CHILD_WGRAD_SHAPES:
        add(B.wgrad_case(shape, 0, True, options={"fp32_core_wide": 1}))
    for n, hub, widths, bf_widths in ((B.SPMM_N, 0, sorted(set(B.SPMM_WIDTHS) | set(B.DUAL_WIDTHS)), ()),
                                      (B.LARGE_N, B.HUB, B.LARGE_WIDTHS, B.LARGE_BF16_WIDTHS)):
        rp, col, va, vl = B.graph(n, hub)
        for w in widths:
            x = B.spmm_x(n, w)
            for tag, val in (("A", va), ("L", vl)):
                r = B.spmm_ratio(B.spmm_restatement(rp, col, val, x), B.csr_reference(rp, col, val, x))
                out["spmm"].append((f"spmm n {n} width {w} {tag}", "", r))
        for w in bf_widths:
            x = B.spmm_x(n, w, bf16=True)
            for tag, val in (("A", va), ("L", vl)):
                s32 = B.spmm_restatement(rp, col, val, x)
                ref = B.csr_reference(rp, col, val, x)
                out["spmm"].append((f"spmm n {n} bf16 rows width {w} {tag}", "", B.spmm_ratio(s32, ref)))
                out["bf16_store"].append((f"bf16 rows n {n} width {w} {tag}", "", B.bf16_store_ratio(s32.to(torch.bfloat16), ref)))
    return out


def test_every_restatement_is_inside_its_bar_and_the_bars_follow_the_rule(restated):
    for cls, rows in restated.items():
        assert rows, cls
        label, name, worst = max(rows, key=lambda t: t[2])
        print(f"{cls}: worst restatement r {worst:.3e} ({label} {name}) -> bar {B.BAR[cls]:.3e}")
        assert worst <= B.BAR[cls], (cls, label, worst)
    # the rule: 4 x the worst restatement ratio, rounded up to a power of two; the stored bf16 rows take the bar of the fp32 sum
    for cls in ("linear", "wgrad", "wgrad_bias", "spmm"):
        assert B.BAR[cls] == B.bar_from(max(r for _, _, r in restated[cls])), cls
    assert B.BAR["bf16_store"] == B.BAR["spmm"]
    # arithmetics 0 and 1 (and 2, against the rounded operands) share the bar: the worst of each is inside it
    assert max(r for _, _, r in restated["bf16_store"]) <= max(r for _, _, r in restated["spmm"])


def test_the_tables_reach_every_kernel_name():
    got = B.table_kernels()
    for op in ("linear", "wgrad"):
        for mode in B.MODES:
            names = got[op][mode]
            for want in B.KERNELS[op][mode]:
                assert any(n.startswith(want) for n in names), (op, mode, want, sorted(names))
    for suffix in B.KERNELS["wgrad_reduce"]:
        for mode in B.MODES:
            assert any(n.endswith(suffix) for n in got["wgrad"][mode]), (mode, suffix)
    for op in ("spmm_csr", "spmm_dual", "spmm_dual_bf16"):
        assert set(B.KERNELS[op]) <= got[op][None], (op, sorted(set(B.KERNELS[op]) - got[op][None]))
    # the environment-only switches (children of the GPU file)
    for shape in B.CHILD_SHAPES:
        assert B.expected_kernel("linear", 0, shape, {"fp32_core_wide": 1}) == "gemm_flat_fast_kernel<FastCore>"
        assert B.expected_kernel("linear", 0, shape) == "gemm_flat_split_kernel<0>/scalar"
        for mode in B.MODES:
            assert B.expected_kernel("linear", mode, shape, {"desc_table": 1}).endswith("/table")
    for shape in B.CHILD_WGRAD_SHAPES:
        assert B.expected_kernel("wgrad", 0, shape, {"fp32_core_wide": 1}).startswith("wgrad_kernel<128>")
    for mode, kernel in ((0, "gemm_flat_split_kernel<0>"), (1, "gemm_flat_split_kernel<3>"), (2, "gemm_flat_split_kernel<1>")):
        assert B.expected_kernel("linear", mode, B.SENSITIVE_LINEAR[0]) == ("gemm_flat_small_kernel" if mode == 0 else kernel + "/scalar")
        assert B.expected_kernel("linear", mode, B.SENSITIVE_LINEAR[1]) == ("gemm_flat_small_kernel" if mode == 0 else kernel + "/table")
    # the hub row does not fit the row-block kernel's LDS
    assert B.HUB > B.rows_cap(False) and B.HUB > B.rows_cap(True)
    assert B.wgrad_chunks(70000) == (576, 122) and B.wgrad_chunks(513) == (512, 2)


# what the former absolute bars say to each planted corruption (True: accepted)
OLD_BARS_ACCEPT = {"a2w2 dropped": True, "k-slab tail missing": False, "chunk slab twice": False, "dbias last chunk": False,
                   "degree G + 1 last entry": False, "odd tail weight": False, "val_a / val_l swapped": False, "hub entry": False}


def _old_linear(got, a, w, b):
    return float((got.double() - (a.double() @ w.double().t() + b.double())).abs().max()) < 2e-5


def test_planted_corruptions_exceed_their_bar_twice():
    seen = {}
    # bf16x3 with one kept product lost, on the non-cancelling inputs of the GPU cases that run the split kernels: every one of
    # the three smallest kept products (a2 * w2, a1 * w3, a3 * w1; the larger ones all the more) is >= 2 x over the bar, in
    # gemm_flat_split_kernel<3> (scalar descriptors, LDS table) and in wgrad_split_kernel<3>
    for shape in B.SENSITIVE_LINEAR:
        assert B.expected_kernel("linear", 1, shape).startswith("gemm_flat_split_kernel<3>")
        a, w, b = B.split_sensitive_inputs(*shape)
        assert B.linear_ratio(B.contract_split3(a, w), a, w, b) <= B.BAR["linear"]
        for drop in B.SPLIT_PRODUCTS:
            r = B.linear_ratio(B.contract_split3(a, w, drop=drop), a, w, b)
            print(f"linear {shape} non-cancelling, product {drop} lost: r = {r:.3e}")
            assert r >= 2 * B.BAR["linear"], (shape, drop, r)
    for shape in B.SENSITIVE_WGRAD:
        assert B.expected_kernel("wgrad", 1, shape).startswith("wgrad_split_kernel<3>")
        d, a = B.wgrad_sensitive_inputs(*shape)
        assert B.wgrad_ratio(B.wgrad_restatement(d, a, 1)[0], d, a) <= B.BAR["wgrad"]
        for drop in B.SPLIT_PRODUCTS:
            r = B.wgrad_ratio(B.wgrad_restatement(d, a, 1, drop=drop)[0], d, a)
            print(f"wgrad {shape} non-cancelling, product {drop} lost: r = {r:.3e}")
            assert r >= 2 * B.BAR["wgrad"], (shape, drop, r)
    # (the former 2e-5 on the ordinary inputs of that shape and of a K = 64 shape: the dropped product is ~2^-18 of an output of size ~1)
    for shape in ((7, 5, 3), (300, 64, 192)):
        a, w, b = B.linear_inputs(*shape)
        bad = B.contract_split3(a, w, drop=(1, 1)) + b
        print(f"a2w2 dropped, ordinary inputs {shape}: r = {B.linear_ratio(bad, a, w, b):.3e}")
        seen["a2w2 dropped"] = seen.get("a2w2 dropped", True) and _old_linear(bad, a, w, b)
    # the K % 32 tail missing from one output row
    a, w, b = B.linear_inputs(131, 36, 4)
    bad = B.linear_restatement(a, w, b, 0, drop_tail_row=130)
    assert B.linear_ratio(bad, a, w, b) >= 2 * B.BAR["linear"]
    seen["k-slab tail missing"] = _old_linear(bad, a, w, b)
    # wgrad: one chunk's slab twice; dbias without its last chunk (one row)
    d, a = B.wgrad_inputs(513, 128, 64)
    dw, db = B.wgrad_restatement(d, a, 0, twice=1)
    assert B.wgrad_ratio(dw, d, a) >= 2 * B.BAR["wgrad"]
    seen["chunk slab twice"] = float((dw.double() - d.double().t() @ a.double()).abs().max()) < 3e-5 * 513 ** 0.5
    dw, db = B.wgrad_restatement(d, a, 0, bias_skip_last=True)
    assert B.wgrad_ratio(dw, d, a) <= B.BAR["wgrad"] and B.dbias_ratio(db, d) >= 2 * B.BAR["wgrad_bias"]
    seen["dbias last chunk"] = float((db.double() - d.double().sum(0)).abs().max()) < 3e-5 * 513 ** 0.5
    # SpMM on the structured graph: rows 0 .. 19 have the forced degrees
    rp, col, va, vl = B.graph(SMALL)
    x = B.spmm_x(SMALL, 32)
    ref_a, ref_l = B.csr_reference(rp, col, va, x), B.csr_reference(rp, col, vl, x)
    good = B.spmm_restatement(rp, col, va, x)
    deg = (rp[1:] - rp[:-1]).tolist()

    def old_spmm(y, ref):
        return float((y.double() - ref[0]).abs().max()) < 5e-6

    row = deg.index(9)                      # G + 1 for the 8-lane groups of width 32: the last entry dropped
    e = int(rp[row + 1]) - 1
    bad = good.clone()
    bad[row] -= va[e] * x[col[e].long()]
    assert B.spmm_ratio(bad, ref_a) >= 2 * B.BAR["spmm"]
    seen["degree G + 1 last entry"] = old_spmm(bad, ref_a)
    row = deg.index(7)                      # odd degree: the tail entry weighted with its neighbour's value
    e = int(rp[row + 1]) - 1
    bad = good.clone()
    bad[row] += (va[e - 1] - va[e]) * x[col[e].long()]
    assert B.spmm_ratio(bad, ref_a) >= 2 * B.BAR["spmm"]
    seen["odd tail weight"] = old_spmm(bad, ref_a)
    row = deg.index(3)                      # dual form: val_a and val_l swapped on one entry
    e = int(rp[row])
    bad_a, bad_l = good.clone(), B.spmm_restatement(rp, col, vl, x)
    bad_a[row] += (vl[e] - va[e]) * x[col[e].long()]
    bad_l[row] += (va[e] - vl[e]) * x[col[e].long()]
    assert B.spmm_ratio(bad_a, ref_a) >= 2 * B.BAR["spmm"] and B.spmm_ratio(bad_l, ref_l) >= 2 * B.BAR["spmm"]
    seen["val_a / val_l swapped"] = old_spmm(bad_a, ref_a) and old_spmm(bad_l, ref_l)
    # hub: the star of test_spmm_empty_rows_and_hub with its smallest entry dropped, against that test's 1e-4
    n = 300
    wt = torch.rand(n - 1, generator=torch.Generator().manual_seed(3)) + 0.5
    hx = torch.randn(n, 96, generator=torch.Generator().manual_seed(4))
    hrp = torch.zeros(n + 1, dtype=torch.int32)
    hrp[1:] = n - 1
    hcol = torch.arange(1, n, dtype=torch.int32)
    href = B.csr_reference(hrp, hcol, wt, hx)
    hgood = B.spmm_restatement(hrp, hcol, wt, hx)
    assert B.spmm_ratio(hgood, href) <= B.BAR["spmm"]
    e = int((wt[:, None] * hx[1:]).abs().max(1).values.argmin())
    bad = hgood.clone()
    bad[0] -= wt[e] * hx[e + 1]
    assert B.spmm_ratio(bad, href) >= 2 * B.BAR["spmm"]
    seen["hub entry"] = float((bad.double() - href[0]).abs().max()) < 1e-4
    print("accepted by the former absolute bars:", seen)
    assert seen == OLD_BARS_ACCEPT


def test_bf16_store_statistic_and_the_tie():
    """One rounding too many (a second rounding through a wider grid), a neighbour value and truncation are outside the bar; a wrong
    direction on an exact tie is not visible to a per-element tolerance, only to bit-equality with the RNE of the fp32 sum."""
    rp, col, va, vl = B.graph(SMALL)
    x = B.spmm_x(SMALL, 64, bf16=True)
    ref = B.csr_reference(rp, col, vl, x)
    s32 = B.spmm_restatement(rp, col, vl, x)
    good = s32.to(torch.bfloat16)
    assert B.bf16_store_ratio(good, ref) <= B.BAR["bf16_store"]
    trunc = (s32.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)            # round toward zero
    assert B.bf16_store_ratio(trunc, ref) >= 2 * B.BAR["bf16_store"]
    nxt = (good.view(torch.int16) + 1).view(torch.bfloat16)                                    # the next bf16 value
    assert B.bf16_store_ratio(nxt, ref) >= 2 * B.BAR["bf16_store"]
    # an exact tie: one entry, weight 1 + 2^-8, x = 1 -> 1.00390625, halfway between bf16 1.0 (even) and 1.0078125
    trp = torch.tensor([0, 1], dtype=torch.int32)
    tcol = torch.tensor([0], dtype=torch.int32)
    tval = torch.tensor([1.0 + 2.0 ** -8])
    tx = torch.ones(1, 4).to(torch.bfloat16)
    tref = B.csr_reference(trp, tcol, tval, tx)
    t32 = B.spmm_restatement(trp, tcol, tval, tx)
    rne = t32.to(torch.bfloat16)
    away = torch.full_like(rne, 1.0078125)
    assert float(rne[0, 0]) == 1.0 and B.bf16_store_ratio(rne, tref) == 0.0
    assert B.bf16_store_ratio(away, tref) == 0.0            # the statistic cannot tell
    assert not torch.equal(away, t32.to(torch.bfloat16))    # bit-equality does (the GPU tests keep it)


def test_statistic_rules():
    z = torch.zeros(2, 2, dtype=torch.float64)
    assert B._ratio(z, z) == 0.0
    e = z.clone()
    e[0, 1] = 1e-30
    assert B._ratio(e, z) == float("inf")                   # a denominator of 0 demands an exact 0
    # relu: a float64 pre-activation below 0 demands an exact 0 unless it is within the bar of 0
    a = torch.tensor([[1.0, -1.0 - 2.0 ** -10]])
    w = torch.tensor([[1.0, 1.0]])
    assert B.linear_ratio(torch.tensor([[1e-9]]), a, w, None, 2) == float("inf")
    a = torch.tensor([[1.0, -1.0 - 2.0 ** -23]])
    assert B.linear_ratio(torch.tensor([[2.0 ** -24]]), a, w, None, 2) <= B.BAR["linear"]
