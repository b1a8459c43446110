"""Per-row bars for the three kernels of csrc/gat.hip: gat_fwd_kernel, gat_bwd_dst_kernel, gat_bwd_src_kernel.

Test helper only (like op_bars.py and window_math.py), numpy, no GPU.  A row is one (node i, period t) pair, m = i * T + t.  What the
kernels owe per row, from the header of gat.hip, with s_j = <u_src, x_j>, d_i = <u_dst, x_i> and the row's LISTED entries j (the
pattern of graph.prepare_attention_pattern: in-edges in edge order, duplicates as listed, listed self loops dropped, the pattern's
own self loop last):

    raw_ij = s_j + d_i,  e_ij = lrelu(raw_ij),  m_i = max_j e_ij,  l_i = sum_j exp(e_ij - m_i),  alpha_ij = exp(e_ij - m_i) / l_i
    out_i = sum_j alpha_ij x_j                         stats[m] = (m_i, l_i, d_i, D_i)
    g_ij = <dout_i, x_j>,  D_i = sum_j alpha_ij g_ij,  de_ij = alpha_ij (g_ij - D_i) (raw_ij > 0 ? 1 : slope)
    dd_i = sum_j de_ij,  ds_j = sum_{i : j -> i} de_ij                                            dsd[m] = (ds, dd)

``reference`` evaluates this in float64 from the same fp32 inputs, sparsely (segment sums over the CSR, never a dense N x N), on
all rows or on a stated subset of them.  The slope is the fp32 value the kernel receives.

The statistic.  Every class is an error over a denominator of absolute terms, the maximum over EVERY row (element for ``out``); a
denominator of 0 demands an exact 0 and a NaN counts as infinite (the rules of op_bars._ratio).  The softmax carries a relative
error proportional to the ABSOLUTE error of the scores, which is an fp32 rounding of S_i = sum_k |u_dst,k x_ik| + max_j sum_k
|u_src,k x_jk|, so (1 + S_i) multiplies the denominators of everything behind the exponential:

    d     |d - d64|     / sum_k |u_dst,k x_ik|
    m     |m - m64|     / S_i
    l     |l - l64|     / (l64 (1 + S_i))
    out   |out - out64| / ((1 + S_i) sum_j alpha64_ij |x_jc|)                    per element c
    D     |D - D64|     / ((1 + S_i) Dabs_i),   Dabs_i = sum_j alpha64_ij G_ij,  G_ij = sum_c |dout_ic x_jc|
    dd    |dd - dd64|   / ((1 + S_i) sum_j alpha64_ij (G_ij + Dabs_i) lr'_ij)
    ds    |ds - ds64|   / sum_{i : j -> i} (1 + S_i) alpha64_ij (G_ij + Dabs_i) lr'_ij

The leaky-relu kink: an fp32 score may fall on the other side of 0 from the float64 one.  An entry is AMBIGUOUS when S_i > 0 and
|raw64_ij| <= BAR["d"] * S_i (S_i = 0 means u_src = u_dst = 0 on the row's entries: raw is 0 in every arithmetic and nothing is
ambiguous).  A row of dd (a source of ds) with ambiguous entries keeps its bar and gets sum_ambiguous (1 - slope) alpha64 |g64 -
D64| taken off its error; it is not dropped.  As a condition on the inputs, from float64 alone: at most 1 % of a case's rows have
an ambiguous entry, and the small cases (everything but the grid-stride case, the hub cases included: one allowance would
cover the whole end-to-end check of a case) are seeded so that they have none (tests/test_gat_bars_cpu.py).

End to end (du_src, du_dst through GatAggregateFunction = ops.wgrad(dsd, x)): per element k against sum_m dsd64_m x_mk, with the
denominator sum_m den_m |x_mk| (den_m: the row's own ds / dd denominator above, which already carries the row's own 1 + S_i) and
the bar BAR[ds or dd] + op_bars.BAR["wgrad"].  This is tighter than one factor 1 + S_max for the whole case: |dsd64_m| <= den_m, so
the weight gradient's own error BAR["wgrad"] sum_m |dsd_m x_mk| is inside BAR["wgrad"] sum_m den_m |x_mk| as well.

Bars.  BAR[class] = 4 x the worst r of the fp32 RESTATEMENT (``restate``) over every case of CASES, rounded up to a power of two
(op_bars.bar_from, ORDER_FACTOR = 4).  The restatement follows the kernels: dot4's fma nesting per lane and the xor-shuffle tree
over the G lanes of a group (the padded lanes hold 0), ev = lrelu(s + d_i), the running-maximum recurrence l = l * sc + w, acc =
fma(w, x_j, acc * sc) with the library exp in fp32, inv = 1 / l, both passes of gat_bwd_dst (D = fma(a, g, D), then dd += a (g -
D) lr') and the gat_bwd_src sum over the transposed CSR.  fma(a, b, c) is float32(float64(a) float64(b) + float64(c)).  Whether
the compiler contracts l * sc + w and the += of the backward sums is its own business: the restatement does not, and __expf in
place of the library exp is likewise part of what the x 4 has to absorb.  tests/test_gat_bars_cpu.py recomputes the table:

    class  worst restatement r                              x 4, rounded up       worst HIP r (MI355X)
    d      1.24e-07  grid stride, F 4 (G = 2, padded)        2 ** -20  (9.54e-07)  1.24e-07  the same case
    m      2.01e-07  scores ascending, F 20 (G = 8, padded)  2 ** -20  (9.54e-07)  2.01e-07  the same case
    l      1.29e-07  scores gap                              2 ** -20  (9.54e-07)  1.03e-07  the same case
    out    6.35e-07  scores zero (201 equal weights in turn) 2 ** -18  (3.81e-06)  6.35e-07  the same case
    D      1.38e-07  scores zero                             2 ** -20  (9.54e-07)  1.38e-07  the same case
    dd     6.77e-08  scores zero                             2 ** -21  (4.77e-07)  6.75e-08  the same case
    ds     9.03e-08  scores ascending                        2 ** -21  (4.77e-07)  1.11e-07  the same case

Planted corruptions of the restatement (CORRUPTIONS, tests/test_gat_bars_cpu.py) exceed the bar of the class they are aimed at by at
least 2 x.  One entry lost from a row of 5 201 is 1 / 5 201 of the row: under the bar of out, 23 x the bar of l.  The end-to-end bar
is the sum of the per-row bars with every row at its worst and one sign, so it is loose by construction (the restatement sits at
1e-11 of its denominator; a wrong slope on every entry is barely over the bar): the per-row bars are what sees the arithmetic, the
end-to-end comparison sees the way from dsd to (du_src, du_dst), e.g. the two columns exchanged.

No kernel was over its bar, so gat.hip did not change: with __expf in place of the library exp the worst HIP r of every
class is within 1.25 x of the restatement's worst (ds: 1.11e-07 against 9.03e-08), at arguments down to -60 (every edge rescaling)
and -119 (underflow to an exact 0); case by case the ratio reaches 1.9 x (D, general F 132 T 1: 1.68e-09 against 8.76e-10).

The HIP kernels' own r per case is in profiles/gat_bars.txt (tools/gat_bars.py writes it).

``expected_group`` restates pick_group of gat.hip; the cases are labelled with it and tests/test_gat_bars_cpu.py asserts that CASES
reaches every G with a full and with a padded group.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from op_bars import bar_from  # noqa: F401  (the rule of the bars; used by tests/test_gat_bars_cpu.py)

BAR = {"d": 2.0 ** -20, "m": 2.0 ** -20, "l": 2.0 ** -20, "out": 2.0 ** -18, "D": 2.0 ** -20, "dd": 2.0 ** -21, "ds": 2.0 ** -21}
CLASSES = ("d", "m", "l", "out", "D", "dd", "ds")
SLOPE = 0.2
SLOPE32 = np.float32(SLOPE)
GRID_CAP = 65536                       # gat.hip: the grid is capped at this many workgroups
AMBIGUOUS_ROWS_CAP = 0.01
F32, F64 = np.float32, np.float64


def expected_group(f: int) -> int:
    """gat.hip pick_group: lanes per (node, period) row, F / 4 float4 pieces padded to a power of two."""
    f4 = f // 4
    return 2 if f4 <= 2 else 4 if f4 <= 4 else 8 if f4 <= 8 else 16 if f4 <= 16 else 32 if f4 <= 32 else 64


def group_form(f: int) -> str:
    return "full" if f // 4 == expected_group(f) else "padded"


def kernel_name(f: int) -> str:
    return f"gat_*_kernel<{expected_group(f)}>/{group_form(f)}"


# ---- the pattern ------------------------------------------------------------------------------------------------------------------

def cpu_pattern(ei: np.ndarray, n: int):
    """(rowptr, col, t_rowptr, t_col) of graph.prepare_attention_pattern, on the host: a row holds its kept in-edges in edge order,
    then the node's own self loop (graph.hip); the transpose is ordered by (source, destination), stable (graph.transpose_csr)."""
    src, dst = np.asarray(ei[0], dtype=np.int64), np.asarray(ei[1], dtype=np.int64)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    order = np.argsort(dst, kind="stable")
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(dst, minlength=n) + 1)
    col = np.empty(int(rowptr[-1]), dtype=np.int64)
    ds = dst[order]
    col[np.arange(ds.size) + ds] = src[order]                   # sorted edge k of destination d sits behind d self loops
    col[rowptr[1:] - 1] = np.arange(n)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    t_order = np.argsort(col * n + rows, kind="stable")
    t_rowptr = np.zeros(n + 1, dtype=np.int64)
    t_rowptr[1:] = np.cumsum(np.bincount(col, minlength=n))
    return rowptr.astype(np.int32), col.astype(np.int32), t_rowptr.astype(np.int32), rows[t_order].astype(np.int32)


def expand(ptr, idx, t_len: int, rows):
    """Entries of the rows m = node * T + t over a CSR: (seg: index into rows, other: row node' * T + t of every entry, start)."""
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    node, t = rows // t_len, rows % t_len
    beg = ptr[node]
    deg = ptr[node + 1] - beg
    start = np.zeros(rows.size + 1, dtype=np.int64)
    start[1:] = np.cumsum(deg)
    seg = np.repeat(np.arange(rows.size), deg)
    e = beg[seg] + (np.arange(int(start[-1])) - start[seg])
    return seg, idx[e] * t_len + t[seg], start


def _segsum(v, start):
    return np.add.reduceat(v, start[:-1], axis=0) if v.shape[0] else np.zeros((start.size - 1,) + v.shape[1:], v.dtype)


def _chunks(start, width: int, budget: int = 1 << 22):
    """Row ranges [a, b) whose entries times the width stay around the budget (a single row may exceed it)."""
    per = max(1, budget // max(1, width))
    a, n = 0, start.size - 1
    while a < n:
        b = int(np.searchsorted(start, start[a] + per, side="right")) - 1
        b = min(n, max(b, a + 1))
        yield a, b
        a = b


# ---- float64 ----------------------------------------------------------------------------------------------------------------------

def reference(c, pat, rows=None, src_rows=None) -> Dict[str, np.ndarray]:
    """Float64 on ``rows`` (default: all); ds, its denominator and allowance on ``src_rows`` (default: all), every out-edge of
    which must end in ``rows``.  Per entry (in CSR order of the rows): alpha, raw, g, seg, src."""
    rowptr, col = pat[0], pat[1]
    t_len, f = c.t, c.f
    x = c.x.reshape(-1, f)
    go = c.dout.reshape(-1, f)
    if rows is None:
        rows = np.arange(x.shape[0], dtype=np.int64)
        src_rows = rows
    seg, src, start = expand(rowptr, col, t_len, rows)
    us, ud = c.us.astype(F64), c.ud.astype(F64)
    slope = float(SLOPE32)
    xi = x[rows].astype(F64)
    d = xi @ ud
    dabs = np.abs(xi) @ np.abs(ud)
    ne = seg.size
    s, sabs, g, gabs = (np.empty(ne) for _ in range(4))
    for a, b in _chunks(start, f):
        e0, e1 = int(start[a]), int(start[b])
        xj = x[src[e0:e1]].astype(F64)
        gi = go[rows[seg[e0:e1]]].astype(F64)
        s[e0:e1] = xj @ us
        sabs[e0:e1] = np.abs(xj) @ np.abs(us)
        g[e0:e1] = (gi * xj).sum(1)
        gabs[e0:e1] = (np.abs(gi) * np.abs(xj)).sum(1)
    raw = s + d[seg]
    lr = np.where(raw > 0, 1.0, slope)
    ev = raw * lr
    m = np.maximum.reduceat(ev, start[:-1])
    p = np.exp(ev - m[seg])
    l = _segsum(p, start)
    alpha = p / l[seg]
    big_s = dabs + np.maximum.reduceat(sabs, start[:-1])
    big_d = _segsum(alpha * g, start)
    big_dabs = _segsum(alpha * gabs, start)
    de = alpha * (g - big_d[seg]) * lr
    den_e = (1.0 + big_s[seg]) * alpha * (gabs + big_dabs[seg]) * lr
    amb = (big_s[seg] > 0) & (np.abs(raw) <= BAR["d"] * big_s[seg])
    allow_e = np.where(amb, (1.0 - slope) * alpha * np.abs(g - big_d[seg]), 0.0)
    out = np.empty((rows.size, f))
    out_abs = np.empty((rows.size, f))
    for a, b in _chunks(start, f):
        e0, e1 = int(start[a]), int(start[b])
        xj = x[src[e0:e1]].astype(F64) * alpha[e0:e1, None]
        st = start[a:b + 1] - e0
        out[a:b] = _segsum(xj, st)
        out_abs[a:b] = _segsum(np.abs(xj), st)
    pos = np.minimum(np.searchsorted(src_rows, src), src_rows.size - 1)
    hit = src_rows[pos] == src
    sums = [np.bincount(pos[hit], weights=v[hit], minlength=src_rows.size) for v in (de, den_e, allow_e)]
    return {"rows": rows, "src_rows": src_rows, "start": start, "seg": seg, "src": src, "alpha": alpha, "raw": raw, "g": g,
            "ambiguous": amb, "S": big_s, "d": d, "d_den": dabs, "m": m, "l": l, "out": out, "out_abs": out_abs, "D": big_d,
            "Dabs": big_dabs, "dd": _segsum(de, start), "dd_den": _segsum(den_e, start), "dd_allow": _segsum(allow_e, start),
            "ds": sums[0], "ds_den": sums[1], "ds_allow": sums[2]}


def _worst(err, den):
    """(max of err / den, flat index of it); a denominator of 0 demands an exact 0, a NaN counts as infinite."""
    assert err.shape == den.shape, (err.shape, den.shape)
    if err.size == 0:
        return 0.0, 0
    bad = np.isnan(err) | ((den == 0) & (err != 0))
    if bad.any():
        return float("inf"), int(np.argmax(bad))
    r = err / np.where(den == 0, 1.0, den)
    k = int(np.argmax(r))
    return float(r.flat[k]), k


def ratios(ref, got) -> Dict[str, tuple]:
    """{class: (r, index of the worst row -- into ref["rows"], for ds into ref["src_rows"])}; ``got`` holds out (R, F), m, l, d, D, dd
    (R) on ref["rows"] and ds on ref["src_rows"]."""
    one_s = 1.0 + ref["S"]
    g = {k: np.asarray(v, dtype=F64) for k, v in got.items()}
    res = {"d": _worst(np.abs(g["d"] - ref["d"]), ref["d_den"]),
           "m": _worst(np.abs(g["m"] - ref["m"]), ref["S"]),
           "l": _worst(np.abs(g["l"] - ref["l"]), ref["l"] * one_s),
           "D": _worst(np.abs(g["D"] - ref["D"]), one_s * ref["Dabs"]),
           "dd": _worst(np.maximum(np.abs(g["dd"] - ref["dd"]) - ref["dd_allow"], 0.0), ref["dd_den"]),
           "ds": _worst(np.maximum(np.abs(g["ds"] - ref["ds"]) - ref["ds_allow"], 0.0), ref["ds_den"])}
    r, k = _worst(np.abs(g["out"] - ref["out"]), one_s[:, None] * ref["out_abs"])
    res["out"] = (r, k // ref["out"].shape[1])
    return res


def ambiguous_rows(ref) -> int:
    """Rows with an ambiguous entry."""
    return int(np.unique(ref["seg"][ref["ambiguous"]]).size)


def du_ratios(ref, c, du_src, du_dst) -> Dict[str, float]:
    """End to end: du = dsd^T x per element against float64, over sum_m den_m |x_mk| (module docstring); needs a full reference."""
    x = c.x.reshape(-1, c.f).astype(F64)
    ax = np.abs(x)
    res = {}
    for key, got, col in (("ds", du_src, "ds"), ("dd", du_dst, "dd")):
        want = ref[col] @ x
        err = np.maximum(np.abs(np.asarray(got, dtype=F64) - want) - ref[col + "_allow"] @ ax, 0.0)
        res[key] = _worst(err, ref[col + "_den"] @ ax)[0]
    return res


# ---- the fp32 restatement ---------------------------------------------------------------------------------------------------------

def _fma(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _dot4(a, b):
    """dot4 of gat.hip per lane: a, b (..., F4, 4) -> (..., F4)."""
    return _fma(a[..., 0], b[..., 0], _fma(a[..., 1], b[..., 1], _fma(a[..., 2], b[..., 2], a[..., 3] * b[..., 3])))


def _group_sum(v, g: int, drop: Optional[int] = None):
    """Lane 0 of the xor-shuffle tree over G lanes (every lane ends with the same bits; lanes >= F4 hold 0).  ``drop``: planted
    corruption -- that lane's contribution is lost."""
    if drop is not None:
        v = v.copy()
        v[..., drop] = 0
    if v.shape[-1] < g:
        v = np.concatenate([v, np.zeros(v.shape[:-1] + (g - v.shape[-1],), F32)], axis=-1)
    off = g // 2
    while off:
        v = v[..., :off] + v[..., off:2 * off]
        off //= 2
    return v[..., 0]


def _lrelu32(v):
    return np.where(v > 0, v, v * SLOPE32)


def _seq_sum(term, start, fused_with=None):
    """Sum of every row's entries one after the other, in fp32; ``fused_with``: acc = fma(term, fused_with, acc)."""
    deg = np.diff(start)
    order = np.argsort(-deg, kind="stable")
    sdeg, sst = deg[order], start[:-1][order]
    acc = np.zeros(deg.size, F32)
    for pos in range(int(sdeg[0]) if deg.size else 0):
        k = int(np.searchsorted(-sdeg, -pos, side="left"))
        e = sst[:k] + pos
        acc[:k] = acc[:k] + term[e] if fused_with is None else _fma(term[e], fused_with[e], acc[:k])
    res = np.empty_like(acc)
    res[order] = acc
    return res


CORRUPTIONS = {            # name: the class whose bar it must exceed twice
    "acc_rescale": "out",       # the rescale of acc (not of l) dropped when the maximum moves
    "final_max": "l",           # the final maximum used for all but the first entry
    "D_zero": "dd",             # D_i = 0 in the second pass of gat_bwd_dst
    "slope_pos": "ds",          # slope in place of 1 for raw > 0
    "skip_last_long": "l",      # the last entry of rows with more than 64 entries skipped (one of 5 201 is under the bar of out)
    "stats_next": "ds",         # stats of row mi + 1 in the source pass
    "drop_lane": "d",           # lane F4 - 1 lost from the group sum of a padded group
    "stale_dsd": "dd",          # dsd of the rows past 65 536 * GROUPS left at the first grid pass's values
}


def restate(c, pat, rows=None, src_rows=None, corrupt: Optional[str] = None) -> Dict[str, np.ndarray]:
    """The three kernels in fp32, in their order (module docstring), on the rows of ``reference``."""
    assert corrupt is None or corrupt in CORRUPTIONS
    rowptr, col, t_rowptr, t_col = pat
    t_len, f = c.t, c.f
    f4, grp = f // 4, expected_group(f)
    drop = f4 - 1 if corrupt == "drop_lane" and f4 < grp else None
    xf = c.x.reshape(-1, f)
    x4 = c.x.reshape(-1, f4, 4)
    go4 = c.dout.reshape(-1, f4, 4)
    us4, ud4 = c.us.reshape(f4, 4), c.ud.reshape(f4, 4)
    if rows is None:
        rows = np.arange(xf.shape[0], dtype=np.int64)
        src_rows = rows

    def gsum(v):
        return _group_sum(v, grp, drop)

    def entry_dots(dst_rows, source_rows, start):
        res = np.empty(dst_rows.size, F32)
        for a, b in _chunks(start, 4 * grp):
            e0, e1 = int(start[a]), int(start[b])
            res[e0:e1] = gsum(_dot4(go4[dst_rows[e0:e1]], x4[source_rows[e0:e1]]))
        return res

    # gat_fwd_kernel
    seg, src, start = expand(rowptr, col, t_len, rows)
    usrc, inv_src = np.unique(src, return_inverse=True)
    d = gsum(_dot4(x4[rows], ud4))
    raw = gsum(_dot4(x4[usrc], us4))[inv_src] + d[seg]
    ev = _lrelu32(raw)
    deg = np.diff(start)
    order = np.argsort(-deg, kind="stable")
    sdeg, sst = deg[order], start[:-1][order]
    fdeg = sdeg.copy()
    if corrupt == "skip_last_long":
        fdeg[sdeg > 64] -= 1
    nr = rows.size
    mx = np.full(nr, -np.inf, F32)
    l = np.zeros(nr, F32)
    acc = np.zeros((nr, f), F32)
    mfin = np.maximum.reduceat(ev, start[:-1])[order] if nr else ev
    for pos in range(int(fdeg[0]) if nr else 0):
        k = int(np.searchsorted(-fdeg, -pos, side="left"))
        e = sst[:k] + pos
        evp, xj = ev[e], xf[src[e]]
        if corrupt == "final_max":
            mn = evp if pos == 0 else mfin[:k]
            sc = np.zeros(k, F32) if pos == 0 else np.ones(k, F32)
        else:
            mn = np.maximum(mx[:k], evp)
            sc = np.exp(mx[:k] - mn)
        w = np.exp(evp - mn)
        l[:k] = l[:k] * sc + w
        acc[:k] = _fma(w[:, None], xj, acc[:k] if corrupt == "acc_rescale" else acc[:k] * sc[:, None])
        mx[:k] = mn
    if corrupt == "final_max":
        mx = np.where(sdeg > 1, mfin, mx).astype(F32)
    with np.errstate(divide="ignore"):
        inv = np.where(l > 0, F32(1) / l, F32(0)).astype(F32)
    unsort = np.empty(nr, dtype=np.int64)
    unsort[order] = np.arange(nr)
    m_o, l_o, inv_o, out = mx[unsort], l[unsort], inv[unsort], (acc * inv[:, None])[unsort]

    # gat_bwd_dst_kernel: the same raw (s_j + st.z) and the alpha of the saved (m, l), twice
    lrp = np.full(raw.size, SLOPE32, F32) if corrupt == "slope_pos" else np.where(raw > 0, F32(1), SLOPE32).astype(F32)
    a_e = np.exp(ev - m_o[seg]) * inv_o[seg]
    g_e = entry_dots(rows[seg], src, start)
    big_d = _seq_sum(a_e, start, fused_with=g_e)
    d_used = np.zeros_like(big_d) if corrupt == "D_zero" else big_d
    dd = _seq_sum(a_e * (g_e - d_used[seg]) * lrp, start)

    # gat_bwd_src_kernel over the transposed pattern
    tseg, dst, tstart = expand(t_rowptr, t_col, t_len, src_rows)
    di = np.searchsorted(rows, dst)
    assert dst.size == 0 or (di.max() < nr and bool((rows[di] == dst).all())), "an out-edge of src_rows ends outside rows"
    if corrupt == "stats_next":
        di = np.minimum(di + 1, nr - 1)
    sj = gsum(_dot4(x4[src_rows], us4))
    traw = sj[tseg] + d[di]
    tlr = np.full(traw.size, SLOPE32, F32) if corrupt == "slope_pos" else np.where(traw > 0, F32(1), SLOPE32).astype(F32)
    ta = np.exp(_lrelu32(traw) - m_o[di]) * inv_o[di]
    tg = entry_dots(dst, src_rows[tseg], tstart)
    ds = _seq_sum(ta * (tg - big_d[di]) * tlr, tstart)
    if corrupt == "stale_dsd":
        first = GRID_CAP * (256 // grp)
        for vals, where in ((dd, rows), (ds, src_rows)):
            late = np.nonzero(where >= first)[0]
            k = np.minimum(np.searchsorted(where, where[late] - first), where.size - 1)
            vals[late] = np.where(where[k] == where[late] - first, vals[k], F32(0))
    return {"out": out, "m": m_o, "l": l_o, "d": d, "D": big_d, "dd": dd, "ds": ds}


# ---- the cases --------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    name: str
    kind: str               # general | hub | regime | stride | single
    n: int
    t: int
    f: int
    regime: str = ""

    @property
    def small(self) -> bool:
        return self.kind != "stride"


@dataclass
class Inputs:
    n: int
    t: int
    f: int
    ei: np.ndarray          # (2, E) int64
    x: np.ndarray           # (N, T, F) fp32
    us: np.ndarray
    ud: np.ndarray
    dout: np.ndarray


GENERAL_F = (4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256)
GENERAL_T = (1, 3)
HUB_N, HUB_DEGREE, HUB_F, HUB_T = 6000, 5200, (32, 132), 2
# per case name: added to the seed of the inputs so that no small case has an ambiguous entry
RESEED = {"general F 16 T 3": 1, "general F 68 T 3": 2, "hub F 32": 2, "hub F 132": 3}
REGIMES = ("ascending", "descending", "equal", "gap", "negative", "zero")
REGIME_N, REGIME_HUB, REGIME_F, REGIME_T = 300, 200, 20, 2
GAP_SOURCE, GAP_SCORE = 100, 121.0
STRIDE_N, STRIDE_T, STRIDE_F = 700001, 12, 4
STRIDE_BLOCK, STRIDE_EVERY = 1024, 997

CASES = [Case(f"general F {f} T {t}", "general", 200 + 7 * (f // 4) % 97, t, f) for f in GENERAL_F for t in GENERAL_T] + \
    [Case(f"hub F {f}", "hub", HUB_N, HUB_T, f) for f in HUB_F] + \
    [Case(f"scores {r}", "regime", REGIME_N, REGIME_T, REGIME_F, r) for r in REGIMES] + \
    [Case("grid stride", "stride", STRIDE_N, STRIDE_T, STRIDE_F), Case("single node", "single", 1, 1, 4)]
CASE = {c.name: c for c in CASES}
DU_CASES = [c.name for c in CASES if c.kind == "hub"] + ["general F 4 T 3", "general F 16 T 3", "general F 20 T 3", "general F 64 T 3",
                                                           "general F 68 T 3", "general F 256 T 3"]


def small_graph(n: int, hub_in: int, seed: int, hub_out: int = 0) -> np.ndarray:
    """The features of window_math.gat_graph at E ~ 10 N: node 0 receives an edge from nodes 1 .. hub_in (in that order: they head
    its CSR row), node 1 sends one to nodes 2 .. hub_out + 1, the last two nodes receive none and the last node sends none either
    (its row of the pattern and of the transposed pattern is the self loop alone), the edge 3 -> 11 is listed twice and the self
    loop 5 -> 5 is listed (the pattern drops it and adds its own)."""
    hub_in = min(hub_in, n - 2)
    g = np.random.default_rng(seed)
    src = [np.arange(1, hub_in + 1), np.ones(hub_out, dtype=np.int64), g.integers(0, n - 1, 10 * n), np.array([3, 3, 5])]
    dst = [np.zeros(hub_in, dtype=np.int64), np.arange(2, hub_out + 2), g.integers(1, n - 2, 10 * n), np.array([11, 11, 5])]
    return np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)


def _scaled_scores(x, g, reach=8.0):
    """Zero-mean score vectors scaled so that |s| + |d| reaches ``reach`` (both signs of raw, a running maximum that moves)."""
    f = x.shape[-1]
    us, ud = g.standard_normal(f), g.standard_normal(f)
    us, ud = us - us.mean(), ud - ud.mean()
    if f == 4:
        us, ud = us + 0.1, ud - 0.1
    x2 = x.reshape(-1, f).astype(F64)
    scale = reach / (np.abs(x2 @ us).max() + np.abs(x2 @ ud).max())
    return (us * scale).astype(F32), (ud * scale).astype(F32)


def _regime_inputs(c: Case, g) -> Inputs:
    """A hub (node 0) of in-degree REGIME_HUB whose CSR row sees the scores of ``c.regime`` in order (the self loop last).
    u_src,0 = 1 and u_dst,0 = 0: component 0 of every x_j sets s_j, and d_i does not depend on it."""
    n, t, f = c.n, c.t, c.f
    ei = small_graph(n, REGIME_HUB, seed=17)
    x = g.random((n, t, f)).astype(F32)
    dout = g.standard_normal((n, t, f)).astype(F32)
    if c.regime == "zero":
        return Inputs(n, t, f, ei, x, np.zeros(f, F32), np.zeros(f, F32), dout)
    us = (0.05 * g.standard_normal(f)).astype(F32)
    ud = (0.02 * g.standard_normal(f)).astype(F32)
    us[0], ud[0] = 1.0, 0.0
    j = np.arange(n, dtype=F64)
    if c.regime == "equal":                      # s_j = 0.5 exactly for every node: raw is constant along every row
        us[1:] = 0.0
        x[:, :, 0] = 0.5
        return Inputs(n, t, f, ei, x, us, ud, dout)
    if c.regime == "ascending":
        want = np.where(j <= REGIME_HUB, 0.3 * j, g.uniform(0.3, 60.0, n))
        want[0] = 0.3 * (REGIME_HUB + 1)
    elif c.regime == "descending":
        want = np.where(j <= REGIME_HUB, 60.3 - 0.3 * (j - 1), g.uniform(0.3, 60.0, n))
        want[0] = 60.3 - 0.3 * REGIME_HUB
    elif c.regime == "negative":
        want = np.where(j <= REGIME_HUB, -0.3 * j, g.uniform(-60.0, -0.3, n))
        want[0] = -0.3 * (REGIME_HUB + 1)
    else:                                        # gap: one source GAP_SCORE, every other in [1, 2)
        want = g.uniform(1.0, 2.0, n)
        want[GAP_SOURCE] = GAP_SCORE
    x64 = x.astype(F64)
    d_hub = x64[0, :, 1:] @ ud[1:].astype(F64)                                   # (T)
    rest = x64[:, :, 1:] @ us[1:].astype(F64)                                    # (N, T)
    x[:, :, 0] = (want[:, None] - d_hub[None, :] - rest).astype(F32)
    return Inputs(n, t, f, ei, x, us, ud, dout)


def _make_inputs(c: Case) -> Inputs:
    g = np.random.default_rng(1000 * c.f + 10 * c.t + c.n + RESEED.get(c.name, 0))
    if c.kind == "regime":
        return _regime_inputs(c, g)
    n, t, f = c.n, c.t, c.f
    if c.kind == "single":
        ei = np.zeros((2, 0), dtype=np.int64)
    elif c.kind == "stride":                     # one random in-edge per node (a listed self loop is dropped) plus the self loop
        ei = np.stack([g.integers(0, n, n), np.arange(n)]).astype(np.int64)
    elif c.kind == "hub":
        ei = small_graph(n, HUB_DEGREE, seed=n, hub_out=HUB_DEGREE)
    else:
        ei = small_graph(n, n - 1, seed=n)
    x = g.random((n, t, f), dtype=F32)
    us, ud = _scaled_scores(x, g)
    dout = g.standard_normal((n, t, f), dtype=F32)
    return Inputs(n, t, f, ei, x, us, ud, dout)


@functools.lru_cache(maxsize=None)
def _small_inputs(name: str) -> Inputs:
    return _make_inputs(CASE[name])


def inputs(c: Case) -> Inputs:
    """The case's inputs (the grid-stride case, 135 MB per buffer, is rebuilt on every call, not kept)."""
    return _make_inputs(c) if c.kind == "stride" else _small_inputs(c.name)


def stride_rows(c: Case, pat):
    """(rows, src_rows) of the grid-stride case.  Stated: the first and the last STRIDE_BLOCK rows, the STRIDE_BLOCK rows on either
    side of row 65 536 * GROUPS (the first row a workgroup reaches on its second pass), every STRIDE_EVERY-th row.  src_rows: the
    sources of the stated rows' entries; rows: the stated rows and the destinations of every out-edge of src_rows, which the
    reference of ds needs."""
    total = c.n * c.t
    first = GRID_CAP * (256 // expected_group(c.f))
    assert total > first + STRIDE_BLOCK
    b = STRIDE_BLOCK
    stated = np.unique(np.concatenate([np.arange(b), np.arange(total - b, total), np.arange(first - b, first + b),
                                       np.arange(0, total, STRIDE_EVERY)]).astype(np.int64))
    src_rows = np.unique(expand(pat[0], pat[1], c.t, stated)[1])
    rows = np.unique(np.concatenate([stated, expand(pat[2], pat[3], c.t, src_rows)[1]]))
    return rows, src_rows


def case_rows(c: Case, pat):
    return stride_rows(c, pat) if c.kind == "stride" else (None, None)


def measure(c: Case, inp: Inputs, pat, ref, got):
    """Rows (class, case label, kernel form, r, description of the worst row) of one case; ``got`` as in ``ratios``."""
    deg = np.diff(ref["start"])
    res = []
    for cls, (r, k) in ratios(ref, got).items():
        if cls == "ds":
            row = int(ref["src_rows"][k]) if ref["src_rows"].size else 0
            node = row // c.t
            where = f"source row {row} (node {node}, out-degree {int(pat[2][node + 1] - pat[2][node])})"
        else:
            row = int(ref["rows"][k]) if ref["rows"].size else 0
            where = f"row {row} (node {row // c.t}, {int(deg[k]) if deg.size else 0} entries)"
        res.append((cls, c.name, kernel_name(c.f), r, where))
    return res


# ---- the HIP kernels, one case (needs the GPU; torch is imported here alone) ------------------------------------------------------

def run_hip(R, c: Case, inp: Inputs, rows=None, src_rows=None):
    """ops.gat_forward and ops.gat_backward on the pattern of graph.prepare_attention_pattern.  Returns (pattern on the host as
    cpu_pattern gives it, ``got`` of ``ratios`` on the rows asked for, D column of stats after the forward alone)."""
    import torch
    dev = torch.device("cuda")
    pat = R.graph.prepare_attention_pattern(torch.from_numpy(inp.ei).to(dev), c.n)
    x, dout = torch.from_numpy(inp.x).to(dev), torch.from_numpy(inp.dout).to(dev)
    us, ud = torch.from_numpy(inp.us).to(dev), torch.from_numpy(inp.ud).to(dev)
    out, stats = R.ops.gat_forward(pat.rowptr, pat.col, x, us, ud, SLOPE)
    fwd_d = stats[:, 3].clone()
    dsd = R.ops.gat_backward(pat.rowptr, pat.col, pat.t_rowptr, pat.t_col, x, us, dout, stats, SLOPE)
    out = out.reshape(-1, c.f)
    if rows is not None:
        ri, si = torch.from_numpy(rows).to(dev), torch.from_numpy(src_rows).to(dev)
        out, stats, fwd_d, dd, ds = out[ri], stats[ri], fwd_d[ri], dsd[ri, 1], dsd[si, 0]
    else:
        dd, ds = dsd[:, 1], dsd[:, 0]
    host = tuple(t.cpu().numpy() for t in (pat.rowptr, pat.col, pat.t_rowptr, pat.t_col))
    st = stats.cpu().numpy()
    got = {"out": out.cpu().numpy(), "m": st[:, 0], "l": st[:, 1], "d": st[:, 2], "D": st[:, 3], "dd": dd.cpu().numpy(),
           "ds": ds.cpu().numpy()}
    return host, got, fwd_d.cpu().numpy()
