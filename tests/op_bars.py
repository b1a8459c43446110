"""Per-element bars for the op-site kernels: regt_linear, regt_wgrad, regt_spmm_csr, regt_spmm_dual, regt_spmm_dual_bf16.

Test helper only (like grad_bars.py).  For ONE output element with terms t_k the statistic is

    r = |got - want64| / sum_k |t_k|

``want64`` is formed in float64 from the same fp32 inputs; the terms are a_mk * w_nk (plus |bias| in the denominator) for
``linear``, d_mn * a_mk for ``wgrad``, d_mn for its bias gradient and val_e * x[col_e] for the SpMMs.  The functions below
return the maximum of r over EVERY element; a denominator of 0 demands an exact 0 (r = inf otherwise).

Activations (1 leaky, 2 relu, 3 sigmoid, 4 tanh) are compared after the activation: the denominator is carried through the
activation's slope at the float64 pre-activation (relu 1 | 0, leaky 1 | slope, sigmoid <= 1/4, tanh <= 1) and one fp32 ulp of the
output is taken off the error.  A relu / leaky pre-activation within bar x denominator of 0 in float64 may be taken on either side
by an fp32 sum: it gets the slope 1 (float64 alone decides this, as tests/test_gpu_spatial.py does); it is not dropped.

bf16 operands (arithmetic 2, kernels that round: ``arithmetic_of``): want64 is the float64 product of the RNE-rounded operands;
products of bf16 values are exact in fp32, so the same bar applies.  bf16 rows out of regt_spmm_dual_bf16 (class ``bf16_store``):
the distance of want64 from the set of reals that round (RNE) to the stored value, over the same denominator.  An exact tie sits
on the edge of two such sets, so this statistic cannot see a wrong rounding direction on ties (no input can make it: any
summation allowance > 0 admits both neighbours); that is what the bit-equality with the fp32 kernel's rounded output is for.

Bars.  A class's bar is 4 x the worst r of the fp32 RESTATEMENT of that class over every case of the tables below, rounded up to a
power of two (4: the summation-order allowance of grad_bars.py; tile and chunk boundaries move with the CU count).  The
restatements: fp32 contraction in k order (linear), the wgrad_chunks grouping in row order followed by the reduce's eight strided
partial sums and tree (wgrad, bias gradient), an fp32 sum in CSR order (SpMM), three RNE bf16 pieces per operand and the six kept
products accumulated in fp32 (bf16x3).  Arithmetics 0 and 1 share a bar.  tests/test_op_bars_cpu.py recomputes the table on the host:

    class        worst restatement r                                              x 4, rounded up      worst HIP r (MI355X)
    linear       3.97e-07  (16385, 2048, 128) act 0, fp32 in k order              2 ** -19  (1.91e-06)  4.13e-07  the same case, gemm_flat_split_kernel<0>
    wgrad        1.90e-07  (513, 128, 64), fp32                                   2 ** -20  (9.54e-07)  2.33e-07  non-cancelling (33, 132, 36), wgrad_split_kernel<3>
    wgrad_bias   8.09e-08  (513, 128, 64)                                         2 ** -21  (4.77e-07)  1.19e-07  the same case
    spmm         4.40e-07  n 41003, bf16 values, width 128, A                     2 ** -19              4.76e-07  n 41003 width 160 L, spmm_panel_kernel<8>
    bf16_store   1.25e-07  (its fp32 sum is the spmm restatement: the spmm bar)   2 ** -19              1.15e-07  width 192 L, spmm_dual_panel_bf16_kernel<8,8>

No kernel was over its bar, so none changed.  Planted corruptions (tests/test_op_bars_cpu.py) exceed their class's bar by at least 2 x.
A bf16x3 kernel that loses one kept product is off by 2^-17.4 .. 2^-16 of a PRODUCT: on random operands that is 4e-7 .. 3e-6 of
sum|terms| (under or barely over the bars; the former 2e-5 accepted it outright), so the split kernels also run the non-cancelling
inputs of ``split_sensitive_inputs`` / ``wgrad_sensitive_inputs``, where any lost product is >= 5.7e-6 in every element.

The HIP kernels' own r per case is in profiles/op_bars.txt (tools/op_bars.py writes it).

``expected_kernel`` restates the host-side dispatch of csrc/gemm_dispatch.hip, gemm_flat.h, wgrad_dispatch.hip, spmm_dispatch.hip and api_ops.hip; the GPU cases are labelled
with its result and tests/test_op_bars_cpu.py asserts that the tables reach every kernel name of KERNELS.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

BAR = {"linear": 2.0 ** -19, "wgrad": 2.0 ** -20, "wgrad_bias": 2.0 ** -21, "spmm": 2.0 ** -19, "bf16_store": 2.0 ** -19}
ORDER_FACTOR = 4.0
LEAKY_SLOPE = 0.01
BF16_U = 2.0 ** -9


def bar_from(worst: float) -> float:
    """4 x worst, rounded up to a power of two."""
    return 2.0 ** math.ceil(math.log2(ORDER_FACTOR * worst))


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(torch.float32)


# ---- the statistic --------------------------------------------------------------------------------------------------------------

def _ratio(err: torch.Tensor, den: torch.Tensor) -> float:
    """max over every element of err / den; den == 0 demands err == 0."""
    assert err.shape == den.shape, (tuple(err.shape), tuple(den.shape))
    if err.numel() == 0:
        return 0.0
    if bool(torch.isnan(err).any()):
        return float("inf")
    zero = den == 0
    if bool((zero & (err != 0)).any()):
        return float("inf")
    return float((err / torch.where(zero, torch.ones_like(den), den)).max())


def _ulp32(v64: torch.Tensor) -> torch.Tensor:
    a = v64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def act64(z: torch.Tensor, act: int, slope: float = LEAKY_SLOPE) -> torch.Tensor:
    if act == 0:
        return z
    if act == 1:
        s = float(torch.tensor(slope, dtype=torch.float32))          # the kernel's slope is an fp32 input
        return torch.where(z > 0, z, z * s)
    if act == 2:
        return torch.relu(z)
    return torch.sigmoid(z) if act == 3 else torch.tanh(z)


def linear_reference(a, w, b, rounded: bool = False):
    """(pre-activation in float64, sum_k |a_mk w_nk| + |bias|)."""
    if rounded:
        a, w = bf16_round(a), bf16_round(w)
    a64, w64 = a.double(), w.double()
    z = a64 @ w64.t()
    den = a64.abs() @ w64.abs().t()
    if b is not None:
        z = z + b.double()
        den = den + b.double().abs()
    return z, den


def linear_ratio(got, a, w, b, act: int = 0, slope: float = LEAKY_SLOPE, rounded: bool = False, bar: float = BAR["linear"], ref=None) -> float:
    """``ref``: linear_reference(a, w, b, rounded) where the caller shares it between activations."""
    z, den = linear_reference(a, w, b, rounded) if ref is None else ref
    want = act64(z, act, slope)
    err = (got.double() - want).abs()
    if act == 0:
        return _ratio(err, den)
    if act in (1, 2):
        low = float(torch.tensor(slope, dtype=torch.float32)) if act == 1 else 0.0
        local = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, low))
        local = torch.where(z.abs() <= bar * den, torch.ones_like(z), local)     # fp32 may take the other side of 0
    elif act == 3:
        local = torch.full_like(z, 0.25)
    else:
        local = torch.ones_like(z)
    return _ratio((err - _ulp32(want)).clamp_min(0.0), local * den)


def wgrad_ratio(dw, d, a, rounded: bool = False) -> float:
    if rounded:
        d, a = bf16_round(d), bf16_round(a)
    d64, a64 = d.double(), a.double()
    return _ratio((dw.double() - d64.t() @ a64).abs(), d64.abs().t() @ a64.abs())


def dbias_ratio(db, d) -> float:
    d64 = d.double()
    return _ratio((db.double() - d64.sum(0)).abs(), d64.abs().sum(0))


def csr_reference(rowptr, col, val, x, nrows: Optional[int] = None, step: int = 1 << 16):
    """(float64 row sums from the CSR itself, sum_e |val_e x[col_e]|) -- x may hold fp32 or bf16 rows."""
    rp, cl = rowptr.long(), col.long()
    n = rp.numel() - 1 if nrows is None else nrows
    rows = torch.repeat_interleave(torch.arange(n, device=rp.device), rp[1:] - rp[:-1])
    v64, x64 = val.double(), x.float().double()
    want = torch.zeros(n, x.shape[1], dtype=torch.float64, device=x.device)
    den = torch.zeros_like(want)
    for s in range(0, rows.numel(), step):
        t = v64[s:s + step, None] * x64[cl[s:s + step]]
        want.index_add_(0, rows[s:s + step], t)
        den.index_add_(0, rows[s:s + step], t.abs())
    return want, den


def spmm_ratio(got, ref) -> float:
    want, den = ref
    return _ratio((got.double() - want).abs(), den)


def bf16_store_ratio(stored, ref) -> float:
    """Distance of want64 from the reals that round to the stored bf16 value, over the denominator."""
    want, den = ref
    v = stored.float().double()
    sgn = torch.where(v < 0, -torch.ones_like(v), torch.ones_like(v))
    wv, av = want * sgn, v.abs()
    m, e = torch.frexp(av)                                   # av = m * 2^e, m in [0.5, 1): 8 significant bits -> spacing 2^(e - 8)
    ulp = torch.where(av > 0, torch.ldexp(torch.ones_like(av), e - 8), torch.zeros_like(av))
    below = torch.where(m == 0.5, ulp / 2, ulp)              # the spacing halves below a power of two
    dist = torch.maximum(wv - (av + ulp / 2), (av - below / 2) - wv).clamp_min(0.0)
    dist = torch.where(av > 0, dist, want.abs())
    return _ratio(dist, den)


# ---- fp32 restatements (host) ----------------------------------------------------------------------------------------------------

def act32(z: torch.Tensor, act: int, slope: float = LEAKY_SLOPE) -> torch.Tensor:
    if act == 0:
        return z
    if act == 1:
        return torch.where(z > 0, z, z * torch.tensor(slope, dtype=torch.float32))
    if act == 2:
        return torch.relu(z)
    return torch.sigmoid(z) if act == 3 else torch.tanh(z)


def contract_k_order(a: torch.Tensor, w: torch.Tensor, drop_tail_row: Optional[int] = None) -> torch.Tensor:
    """fp32 a @ w.T, one k after the other.  drop_tail_row: planted corruption -- that output row misses the K % 32 tail."""
    m, k = a.shape
    acc = torch.zeros(m, w.shape[0], dtype=torch.float32)
    wt = w.t().contiguous()
    for i in range(k):
        if drop_tail_row is not None and i >= k - k % 32:
            col = a[:, i:i + 1].clone()
            col[drop_tail_row] = 0.0
            acc.addcmul_(col, wt[i])
        else:
            acc.addcmul_(a[:, i:i + 1], wt[i])
    return acc


def split3(t: torch.Tensor):
    """Three RNE bf16 pieces of an fp32 tensor (t1 + t2 + t3 == t exactly)."""
    t1 = bf16_round(t)
    t2 = bf16_round(t - t1)
    t3 = bf16_round(t - t1 - t2)
    return t1, t2, t3


SPLIT_PRODUCTS = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))        # a1w1, a1w2, a2w1, a1w3, a2w2, a3w1


def contract_split3(a: torch.Tensor, w: torch.Tensor, drop=None) -> torch.Tensor:
    """bf16x3 emulation of a @ w.T: the six kept products, each exact in fp32, accumulated in fp32, small terms first."""
    ap, wp = split3(a), split3(w)
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for i, j in reversed(SPLIT_PRODUCTS):
        if drop is not None and (i, j) == drop:
            continue
        acc += ap[i] @ wp[j].t()
    return acc


def linear_restatement(a, w, b, arith: int, **corrupt) -> torch.Tensor:
    """fp32 pre-activation in the arithmetic of the kernel (``arithmetic_of``): 0 fp32, 1 bf16x3, 2 bf16 operands."""
    if arith == 1:
        z = contract_split3(a, w, drop=corrupt.get("drop"))
    elif arith == 2:
        z = contract_k_order(bf16_round(a), bf16_round(w), corrupt.get("drop_tail_row"))
    else:
        z = contract_k_order(a, w, corrupt.get("drop_tail_row"))
    return z if b is None else z + b


def wgrad_chunks(m: int) -> Tuple[int, int]:
    """api_ops.hip wgrad_chunks: (rows per chunk, chunks) of regt_wgrad."""
    kc = ((m + 127) // 128 + 31) // 32 * 32
    kc = max(kc, 512)
    return kc, (m + kc - 1) // kc


def reduce_slabs(slabs) -> torch.Tensor:
    """wgrad_reduce.hip wgrad_reduce_body: eight partial sums over every eighth chunk, then ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7))."""
    part = []
    for s in range(8):
        acc = torch.zeros_like(slabs[0])
        for c in range(s, len(slabs), 8):
            acc = acc + slabs[c]
        part.append(acc)
    return ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]))


def wgrad_restatement(d, a, arith: int = 0, drop=None, twice: Optional[int] = None, bias_skip_last: bool = False):
    """(dW, dbias) in fp32: every chunk of wgrad_chunks summed in row order, the slabs reduced as the kernel does.  Planted
    corruptions: ``drop`` -- that product of the bf16x3 split is lost; ``twice`` -- that chunk's slab enters the reduction twice; ``bias_skip_last`` -- dbias misses its last chunk."""
    m = d.shape[0]
    kc, nc = wgrad_chunks(m)
    slabs, sums = [], []
    for c in range(nc):
        dc, ac = d[c * kc:(c + 1) * kc], a[c * kc:(c + 1) * kc]
        if arith == 1:
            slabs.append(contract_split3(dc.t().contiguous(), ac.t().contiguous(), drop=drop))
        elif arith == 2:
            slabs.append(contract_k_order(bf16_round(dc).t().contiguous(), bf16_round(ac).t().contiguous()))
        else:
            slabs.append(contract_k_order(dc.t().contiguous(), ac.t().contiguous()))
        s = torch.zeros(d.shape[1], dtype=torch.float32)
        for r in range(dc.shape[0]):
            s = s + dc[r]
        sums.append(s)
    if twice is not None:
        slabs.append(slabs[twice])
    if bias_skip_last:
        sums = sums[:-1] if len(sums) > 1 else [torch.zeros_like(sums[0])]
    return reduce_slabs(slabs), reduce_slabs(sums)


def spmm_restatement(rowptr, col, val, x, nrows: Optional[int] = None) -> torch.Tensor:
    """fp32 row sums in CSR order (x: fp32 rows, or bf16 rows widened exactly)."""
    rp, cl = rowptr.long(), col.long()
    n = rp.numel() - 1 if nrows is None else nrows
    deg = rp[1:n + 1] - rp[:n]
    order = torch.argsort(deg, descending=True)
    sdeg = deg[order]
    xf = x.float()
    acc = torch.zeros(n, x.shape[1], dtype=torch.float32)
    for j in range(int(sdeg[0]) if n else 0):
        rows = order[:int((sdeg > j).sum())]
        e = rp[rows] + j
        acc[rows] = acc[rows] + val[e, None] * xf[cl[e]]
    return acc


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

SPLIT_MAG = 1.0 + 0.75 * 2.0 ** -8 + 0.375 * 2.0 ** -16


def linear_inputs(m: int, k: int, n: int):
    g = torch.Generator().manual_seed(m * 31 + k * 7 + n)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / max(1.0, k ** 0.5)
    b = torch.randn(n, generator=g)
    return a, w, b


def split_sensitive_inputs(m: int, k: int, n: int):
    """Every operand is +-SPLIT_MAG * 2^e, SPLIT_MAG = 1 + 0.75 * 2^-8 + 0.375 * 2^-16: its bf16 pieces are 1, 0.75 * 2^-8 and
    0.375 * 2^-16, so a2 * w2 is 2^-16.8 and a1 * w3, a3 * w1 are 2^-17.4 of the product, and with equal signs along k nothing
    cancels: a kernel that loses any kept product is off by that share of sum|terms| in EVERY element."""
    g = torch.Generator().manual_seed(m + k + n)
    mag = SPLIT_MAG
    a = mag * torch.ldexp(torch.ones(m, k), torch.randint(-2, 3, (m, k), generator=g))
    w = mag * torch.ldexp(torch.ones(n, k), torch.randint(-2, 3, (n, k), generator=g))
    a = a * (torch.randint(0, 2, (m, 1), generator=g) * 2 - 1)
    w = w * (torch.randint(0, 2, (n, 1), generator=g) * 2 - 1)
    return a, w, torch.zeros(n)


def wgrad_sensitive_inputs(m: int, n: int, k: int):
    """The same for the weight gradient: signs constant along M (one per column of d and of a)."""
    g = torch.Generator().manual_seed(m + n + k)
    d = SPLIT_MAG * torch.ldexp(torch.ones(m, n), torch.randint(-2, 3, (m, n), generator=g))
    a = SPLIT_MAG * torch.ldexp(torch.ones(m, k), torch.randint(-2, 3, (m, k), generator=g))
    return d * (torch.randint(0, 2, (1, n), generator=g) * 2 - 1), a * (torch.randint(0, 2, (1, k), generator=g) * 2 - 1)


def wgrad_inputs(m: int, n: int, k: int):
    g = torch.Generator().manual_seed(m + 3 * n + 5 * k)
    return torch.randn(m, n, generator=g), torch.randn(m, k, generator=g)


FORCED_DEGREES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 300)


def structured_graph(n: int, seed: int = 0, hub: int = 0):
    """Merged two-weight CSR (rowptr, col, val_a, val_l) with the row degrees FORCED_DEGREES at the first rows, in reverse at the
    last rows and (n >= 4096) around the middle; the other rows have 0 .. 12 entries.  Duplicate columns are allowed and one is
    planted in every forced row of degree >= 2.  |weights| = 2^U(-6, 6); val_a positive, val_l with mixed signs.  ``hub``: that many
    entries in row n // 3."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 13, (n,), generator=g)
    k = len(FORCED_DEGREES)
    forced = torch.tensor(FORCED_DEGREES)
    deg[:k] = forced
    deg[n - k:] = forced.flip(0)
    if n >= 4096:
        deg[n // 2:n // 2 + k] = forced
    if hub:
        deg[n // 3] = hub
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(deg, 0)
    nnz = int(rowptr[-1])
    col = torch.randint(0, n, (nnz,), generator=g)
    for r in list(range(k)) + list(range(n - k, n)):
        if deg[r] >= 2:
            col[rowptr[r] + 1] = col[rowptr[r]]
    mag = torch.exp2(torch.rand(nnz, generator=g) * 12 - 6)
    val_a = mag.clone()
    val_l = torch.exp2(torch.rand(nnz, generator=g) * 12 - 6) * (torch.randint(0, 2, (nnz,), generator=g) * 2 - 1)
    return rowptr.int(), col.int(), val_a.float(), val_l.float()


def stacked(rowptr, col, val_a, val_l):
    """[A; L] as one CSR of 2 n rows over the same n rows of X (the overlapping-regions layout)."""
    nnz = int(rowptr[-1])
    return torch.cat([rowptr, rowptr[1:] + nnz]).int(), torch.cat([col, col]), torch.cat([val_a, val_l])


def spmm_x(n: int, width: int, bf16: bool = False):
    x = torch.randn(n, width, generator=torch.Generator().manual_seed(n + width))
    return x.to(torch.bfloat16) if bf16 else x


# ---- the tables of GPU cases -----------------------------------------------------------------------------------------------------

# (M, K, N), acts per arithmetic: act 3 and 4 once per kernel; the long-K shape with two acts
LINEAR_CASES = [
    ((7, 5, 3), (0, 1, 2, 3, 4)),                # scalar flat
    ((129, 257, 65), (0, 1, 2)),                 # scalar flat, several k slabs, odd everything
    ((130, 30, 64), (0, 1, 2, 3, 4)),            # flat with vector stores, K % 4 != 0
    ((300, 64, 192), (0, 1, 2, 3, 4)),           # mode 0: small kernel, partial row and column tiles of its 64 x 64 tile
    ((131, 36, 4), (0, 1, 2)),                   # one partial tile, K not a multiple of 32
    ((16300, 32, 128), (0, 1, 2, 3, 4)),         # mode 0: split core, scalar descriptors, ragged last row tile
    ((16300, 36, 132), (0, 1, 2, 3, 4)),         # mode 0: split core, LDS table, 4-wide partial second column tile
    ((16385, 2048, 128), (0, 2)),                # long K
]
# A = I (K x K) with an asymmetric W (N x K): one shape per kernel name and arithmetic
IDENTITY_CASES = [(5, 3), (30, 64), (64, 192), (128, 16384), (132, 8192)]      # the last two: 128 tiles (mode 0 split core), K % 32 != 0
CHILD_SHAPES = [(16384, 64, 128), (16300, 32, 132)]          # one full-tile and one ragged shape for the environment-only switches
CHILD_WGRAD_SHAPES = [(513, 128, 64), (1100, 132, 36)]       # REGT_FP32_CORE=wide: wgrad_kernel<128> in place of wgrad3_kernel
# non-cancelling inputs (split_sensitive_inputs / wgrad_sensitive_inputs): a lost product of the bf16x3 split shows in every element.
# (M, K, N): the split core with scalar descriptors and with the LDS table; (M, N, K): wgrad_split_kernel<3>, full and partial tiles.
# These cases run under arithmetic 1 only, without bias, and their reductions are short on purpose: a sum of equal-sign terms carries
# the rounding of every addition (fp32 in row order over 40 rows is already at 5e-7 of sum|terms|, over a 512-row chunk at 2.6e-6),
# which says nothing about a lost product; the matrix pipe adds 16 rows per step.
SENSITIVE_LINEAR = [(130, 32, 8), (131, 36, 4)]
SENSITIVE_WGRAD = [(16, 128, 64), (33, 132, 36)]

# (M, N, K)
WGRAD_CASES = [(1, 4, 4), (513, 128, 64), (1100, 132, 36), (1100, 130, 33), (1100, 6, 7), (3000, 256, 8), (3000, 256, 32),
               (70000, 128, 64)]

SPMM_N = 600
SPMM_WIDTHS = (4, 32, 36, 64, 100, 128, 256, 260, 384, 388, 512, 768, 1024, 2048, 2052)
DUAL_WIDTHS = (4, 32, 48, 64, 100, 128, 256, 512, 1024, 2048)
LARGE_N = 41003                       # not a multiple of 8: the eight XCD chunks are unequal
LARGE_WIDTHS = (160, 192)             # 128-byte panels, 256-byte panels
LARGE_BF16_WIDTHS = (192, 128)        # 384-byte rows (128-byte panels), 256-byte rows
HUB = 12000                           # entries of the hub row of the large graph: more than rows_cap() in its workgroup
MODES = (0, 1, 2)


# ---- the dispatch, restated ------------------------------------------------------------------------------------------------------

GBM = GBN = 128
GBK = 32
SM_B = 64
G_MAX_ITERS = 80
SMALL_TILE_LIMIT = 128
SP_WIDE_SLICE_MAX = 9 << 19


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def panel_wide(nnodes: int) -> bool:
    # spmm_dispatch.hip panel_wide (REGT_SPMM_PL unset): an XCD's slice of X at 256 B per node stays around its L2
    return _cdiv(nnodes, 8) * 256 <= SP_WIDE_SLICE_MAX


def rows_rpg(nnodes: int, pl: int, bf: bool) -> int:
    # spmm_dispatch.hip rows_rpg
    return max(1, _cdiv(_cdiv(nnodes, 8), (256 // pl) * (150 if bf else 240)))


def rows_cap(bf: bool) -> int:
    # spmm_dispatch.hip rows_cap: LDS entries per workgroup of the row-block kernel
    return (163840 // (5 if bf else 8) - 260 * 4 - 64) // 16


def rows_ok(nnodes: int, x_rows: int, rowbytes: int, pl: int, spmm_rows: int) -> bool:
    # spmm_dispatch.hip rows_wanted + rows_ok
    return bool(spmm_rows) and rowbytes % (pl * 16) == 0 and x_rows * rowbytes < (1 << 32) - 4096 and \
        nnodes * rowbytes < (1 << 32) - 4096 and (256 // pl) * rows_rpg(nnodes, pl, False) <= 256


def arithmetic_of(name: str) -> int:
    """The arithmetic a kernel name stands for: 2 -- operands enter the matrix cores as single RNE bf16 values; 1 -- bf16x3; 0 -- fp32
    (the flat, small and generic kernels are fp32 whatever the process-wide arithmetic)."""
    if name.startswith(("gemm_flat_split_kernel<1>", "wgrad_split_kernel<1>")):
        return 2
    return 1 if name.startswith(("gemm_flat_split_kernel<3>", "wgrad_split_kernel<3>")) else 0


def expected_kernel(op: str, mode: int, shape, options: Optional[Dict] = None) -> str:
    """Name of the kernel (and, where the launch function picks one, its form) that the op-site entry point launches.
    op: linear (M, K, N) | wgrad (M, N, K) | spmm_csr (nrows, x_rows, W) | spmm_dual (n, W) | spmm_dual_bf16 (n, x_rows, W).
    options: fp32_core_wide (REGT_FP32_CORE=wide), desc_table (REGT_GEMM_DESC=table), spmm_rows, with_bias (wgrad)."""
    o = dict(fp32_core_wide=0, desc_table=0, spmm_rows=0, with_bias=1)
    o.update(options or {})
    if op == "linear":
        m, k, n = shape
        # gemm_fwd.hip launch_gemm_bias_act: contiguous fp32 tensors, ldo = N; api_internal.h make_seg: SEG_VEC_A / _B need lda = ldb = K % 4 == 0
        vec = n % 4 == 0
        # gemm_dispatch.hip fast_class: one BT segment, no region, no relu on A
        fast = vec and k % 4 == 0 and _cdiv(k, GBK) <= G_MAX_ITERS and k < (1 << 22)
        if not fast:
            return f"gemm_flat_kernel<vec={int(vec)}>"              # gemm_flat.h launch_flat: fp32 in every arithmetic
        tiles = _cdiv(m, GBM) * _cdiv(n, GBN)
        # gemm_flat.h launch_fast
        if mode == 0 and tiles < SMALL_TILE_LIMIT:
            return "gemm_flat_small_kernel"
        if mode == 0 and o["fp32_core_wide"]:
            return "gemm_flat_fast_kernel<FastCore>"
        # gemm_dispatch.hip uniform_ok: scalar slab descriptors need K % 32 == 0 (bf16 operands: at most 64 slabs)
        uniform = not o["desc_table"] and k % GBK == 0 and k * 4 * (GBM + 1) < (1 << 31) and not (mode == 2 and k // GBK > 64)
        return f"gemm_flat_split_kernel<{(0, 3, 1)[mode]}>/{'scalar' if uniform else 'table'}"
    if op == "wgrad":
        m, nout, nin = shape
        # api_ops.hip wgrad_chunks + api_step.hip wgrad_full: one right-hand side, fp32 rows, ldp = Nout, ldq = Nin
        kc, nc = wgrad_chunks(m)
        # wgrad_dispatch.hip wgrad_pick
        wide = nin > 32
        fast = nout % 4 == 0 and nin % 4 == 0 and kc <= 65536
        if wide and fast:
            name = "wgrad_split_kernel<3>" if mode == 1 else "wgrad_split_kernel<1>" if mode == 2 else \
                "wgrad_kernel<128>" if o["fp32_core_wide"] else "wgrad3_kernel"
        elif wide:
            name = "wgrad_kernel_generic<128>"
        elif fast:
            name = "wgrad_kernel<32>"
        else:
            name = "wgrad_kernel_generic<32>"
        # wgrad_reduce.hip wgrad_reduce_vec_ok: slab stride = Nout * Nin (+ Nout with a bias gradient), ldo = Nin
        stride = nout * nin + (nout if o["with_bias"] else 0)
        v4 = nin % 4 == 0 and stride % 4 == 0
        return f"{name} + wgrad_reduce_kernel/{'v4' if v4 else 'scalar'} x{nc}"
    if op == "spmm_csr":
        nrows, x_rows, w = shape
        w4 = w // 4
        # spmm_dispatch.hip spmm_pick, SP_SINGLE (launch_spmm_csr).  regt_spmm_csr (api_ops.hip) always passes nstack = 1, so a stacked operator runs as a plain CSR of
        # 2 n rows over n rows of X: the nstack > 1 indexing of spmm_panel_kernel cannot be reached from the op site
        if w4 % 8 == 0 and x_rows * w * 4 > (24 << 20) and nrows >= 4096:
            pl = 16 if panel_wide(nrows) and w4 % 16 == 0 else 8
            if rows_ok(nrows, x_rows, 4 * w, pl, o["spmm_rows"]):
                return f"spmm_rows_kernel<{pl},false,false>"
            return f"spmm_panel_kernel<{pl}>"
        if w4 > 512:
            return "spmm_csr_kernel<64,8>/column-pass"
        for lim, g, ch in ((8, 8, 1), (16, 16, 1), (32, 32, 1), (64, 64, 1), (96, 32, 3), (128, 64, 2), (192, 64, 3), (256, 64, 4),
                           (512, 64, 8)):
            if w4 <= lim:
                return f"spmm_csr_kernel<{g},{ch}>"
    if op == "spmm_dual":
        n, w = shape
        w4 = w // 4
        # spmm_dispatch.hip spmm_pick, SP_DUAL (launch_spmm_dual_x; regt_spmm_dual: x_rows = n)
        if w % 32 != 0 or (n * w * 4 <= (24 << 20) and w4 <= 512):
            for lim, g, ch in ((8, 8, 1), (16, 16, 1), (32, 32, 1), (64, 64, 1), (128, 64, 2), (256, 64, 4), (512, 64, 8)):
                if w4 <= lim:
                    return f"spmm_dual_csr_kernel<{g},{ch}>"
        pl = 16 if panel_wide(n) and w4 % 16 == 0 else 8
        if rows_ok(n, n, 4 * w, pl, o["spmm_rows"]):
            return f"spmm_rows_kernel<{pl},true,false>"
        return f"spmm_dual_panel_kernel<{pl},{pl}>"
    if op == "spmm_dual_bf16":
        n, x_rows, w = shape
        # spmm_dispatch.hip spmm_pick, SP_DUAL_BF16 (launch_spmm_dual_bf16)
        pl = 16 if panel_wide(n) and (2 * w) % 256 == 0 else 8
        if o["spmm_rows"] and (256 // pl) * rows_rpg(n, pl, True) <= 256:
            return f"spmm_rows_kernel<{pl},true,true>"
        return f"spmm_dual_panel_bf16_kernel<{pl},{pl}>"
    raise ValueError(f"expected_kernel: {op} {shape}")


# kernel names the GPU tables must reach, per arithmetic in which the name exists (the reduce form is a suffix of the wgrad names)
KERNELS = {
    "linear": {0: ("gemm_flat_kernel<vec=0>", "gemm_flat_kernel<vec=1>", "gemm_flat_small_kernel", "gemm_flat_split_kernel<0>/scalar",
                   "gemm_flat_split_kernel<0>/table"),
               1: ("gemm_flat_kernel<vec=0>", "gemm_flat_kernel<vec=1>", "gemm_flat_split_kernel<3>/scalar", "gemm_flat_split_kernel<3>/table"),
               2: ("gemm_flat_kernel<vec=0>", "gemm_flat_kernel<vec=1>", "gemm_flat_split_kernel<1>/scalar", "gemm_flat_split_kernel<1>/table")},
    "wgrad": {0: ("wgrad_kernel<32>", "wgrad3_kernel", "wgrad_kernel_generic<128>", "wgrad_kernel_generic<32>"),
              1: ("wgrad_kernel<32>", "wgrad_split_kernel<3>", "wgrad_kernel_generic<128>", "wgrad_kernel_generic<32>"),
              2: ("wgrad_kernel<32>", "wgrad_split_kernel<1>", "wgrad_kernel_generic<128>", "wgrad_kernel_generic<32>")},
    "wgrad_reduce": ("/v4 x1", "/v4 x2", "/v4 x3", "/scalar x3", "/v4 x122"),
    "spmm_csr": tuple(f"spmm_csr_kernel<{g},{c}>" for g, c in ((8, 1), (16, 1), (32, 1), (64, 1), (32, 3), (64, 2), (64, 3), (64, 4), (64, 8)))
    + ("spmm_csr_kernel<64,8>/column-pass", "spmm_panel_kernel<8>", "spmm_panel_kernel<16>", "spmm_rows_kernel<8,false,false>",
       "spmm_rows_kernel<16,false,false>"),
    "spmm_dual": tuple(f"spmm_dual_csr_kernel<{g},{c}>" for g, c in ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 8)))
    + ("spmm_dual_panel_kernel<8,8>", "spmm_dual_panel_kernel<16,16>", "spmm_rows_kernel<8,true,false>", "spmm_rows_kernel<16,true,false>"),
    "spmm_dual_bf16": ("spmm_dual_panel_bf16_kernel<8,8>", "spmm_dual_panel_bf16_kernel<16,16>", "spmm_rows_kernel<8,true,true>",
                       "spmm_rows_kernel<16,true,true>"),
}


def table_kernels():
    """{op: {mode or None: set of names}} that the GPU tables reach (the environment-only switches stay out: children run them)."""
    out = {"linear": {m: set() for m in MODES}, "wgrad": {m: set() for m in MODES}, "spmm_csr": {None: set()}, "spmm_dual": {None: set()},
           "spmm_dual_bf16": {None: set()}}
    for mode in MODES:
        for shape, _ in LINEAR_CASES:
            out["linear"][mode].add(expected_kernel("linear", mode, shape))
        for k, n in IDENTITY_CASES:
            out["linear"][mode].add(expected_kernel("linear", mode, (k, k, n)))
        for shape in WGRAD_CASES:
            for wb in (0, 1):
                out["wgrad"][mode].add(expected_kernel("wgrad", mode, shape, {"with_bias": wb}))
    for w in SPMM_WIDTHS:
        out["spmm_csr"][None].add(expected_kernel("spmm_csr", 0, (SPMM_N, SPMM_N, w)))
    for w in DUAL_WIDTHS:
        out["spmm_dual"][None].add(expected_kernel("spmm_dual", 0, (SPMM_N, w)))
    for rows in (0, 1):
        opt = {"spmm_rows": rows}
        for w in LARGE_WIDTHS:
            out["spmm_csr"][None].add(expected_kernel("spmm_csr", 0, (LARGE_N, LARGE_N, w), opt))
            out["spmm_csr"][None].add(expected_kernel("spmm_csr", 0, (2 * LARGE_N, LARGE_N, w), opt))
            out["spmm_dual"][None].add(expected_kernel("spmm_dual", 0, (LARGE_N, w), opt))
        for w in LARGE_BF16_WIDTHS:
            out["spmm_dual_bf16"][None].add(expected_kernel("spmm_dual_bf16", 0, (LARGE_N, LARGE_N, w), opt))
    return out


# ---- one case, both ways: rows (class, case label, kernel name, r of the HIP kernel | None, r of the restatement | None) ----------

_MEMO: Dict = {}


def _memo(key, make):
    """A restatement depends on the inputs and the arithmetic alone: shared between modes, activations and bias forms."""
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def linear_case(shape, acts, mode: int, hip=None, restate: bool = True, options: Optional[Dict] = None, inputs=None):
    """hip(a, w, b, act) -> the kernel's output (any device); restate: also evaluate the fp32 restatement; inputs: the generator
    (default linear_inputs)."""
    a, w, b = (inputs or linear_inputs)(*shape)
    tag = "" if inputs is None else " non-cancelling"
    name = expected_kernel("linear", mode, shape, options)
    ar = arithmetic_of(name)
    ref = linear_reference(a, w, b, rounded=ar == 2)
    z32 = _memo(("linear", tag, shape, ar), lambda: linear_restatement(a, w, b, ar)) if restate else None
    rows = []
    for act in acts:
        r_hip = None if hip is None else linear_ratio(hip(a, w, b, act).cpu(), a, w, b, act, ref=ref)
        r_ref = linear_ratio(act32(z32, act), a, w, b, act, ref=ref) if restate else None
        rows.append(("linear", f"linear{tag} {shape} act {act} mode {mode}", name, r_hip, r_ref))
    return rows


def identity_case(k: int, n: int, mode: int, hip=None, restate: bool = True):
    """A = I (K x K) with the asymmetric W (N x K) = arange / 100; hip(a, w) -> output.  Returns (rows, a, w, output)."""
    w = torch.arange(n * k, dtype=torch.float32).reshape(n, k) / 100.0
    a = torch.eye(k)
    name = expected_kernel("linear", mode, (k, k, n))
    ar = arithmetic_of(name)
    ref = linear_reference(a, w, None, rounded=ar == 2)
    got = None if hip is None else hip(a, w).cpu()
    r_ref = linear_ratio(_memo(("identity", k, n, ar), lambda: linear_restatement(a, w, None, ar)), a, w, None, ref=ref) if restate else None
    return [("linear", f"linear identity K {k} N {n} mode {mode}", name, None if got is None else linear_ratio(got, a, w, None, ref=ref),
             r_ref)], a, w, got


def wgrad_case(shape, mode: int, with_bias: bool, hip=None, restate: bool = True, options: Optional[Dict] = None, inputs=None):
    """hip(d, a, with_bias) -> (dW, dbias | None)."""
    d, a = (inputs or wgrad_inputs)(*shape)
    name = expected_kernel("wgrad", mode, shape, dict(options or {}, with_bias=int(with_bias)))
    ar = arithmetic_of(name)
    dw32, db32 = _memo(("wgrad", inputs is None, shape, ar), lambda: wgrad_restatement(d, a, ar)) if restate else (None, None)
    dw, db = hip(d, a, with_bias) if hip is not None else (None, None)
    label = f"wgrad{'' if inputs is None else ' non-cancelling'} {shape} {'with' if with_bias else 'no'} dbias mode {mode}"
    rows = [("wgrad", label, name, None if dw is None else wgrad_ratio(dw.cpu(), d, a, ar == 2),
             wgrad_ratio(dw32, d, a, ar == 2) if restate else None)]
    if with_bias:            # the bias gradient is an fp32 column sum in every arithmetic
        rows.append(("wgrad_bias", label, name, None if db is None else dbias_ratio(db.cpu(), d), dbias_ratio(db32, d) if restate else None))
    return rows


_GRAPHS: Dict = {}


def graph(n: int, hub: int = 0):
    if (n, hub) not in _GRAPHS:
        _GRAPHS[(n, hub)] = structured_graph(n, seed=n, hub=hub)
    return _GRAPHS[(n, hub)]
