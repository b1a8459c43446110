"""Guarded operand windows and plain references for the op-site entry points of include/regtgcn.h (regt_linear, regt_wgrad,
regt_spmm_csr / _dual, regt_pack_x, regt_gat_forward / _backward).  Test helper only, pure torch, CPU and GPU.

A ``Window`` places a logical rows x cols fp32 array (or a vector) inside one larger allocation that the test owns: a margin in
front of it and behind it, a leading dimension that may exceed the width, a column offset.  Every word of the allocation that is
not an element of the window holds POISON, one quiet-NaN bit pattern, and so does the inside of an output window.  A kernel
that stores outside its window changes a poisoned word (``check_untouched``); one that skips an element leaves one
(``check_written``); one that reads outside its window and lets the value reach the result -- multiplied by zero instead of
selected, for instance -- produces a NaN, which no comparison with a reference survives.  The margins (128 rows, a whole row
tile of the GEMM kernels, on either side) keep such an overrun inside the test's own memory.
"""
from __future__ import annotations

import functools

import torch

from fused_math import bf16_round
from gru_math import bar, rel_err

POISON = 0x7FC5A5A5            # a quiet NaN (exponent all ones, mantissa msb set) that no arithmetic produces; compared as int32
MARGIN_ROWS = 128              # rows of a GEMM row tile
MARGIN_WORDS = 128 * 128       # margin of a vector window: one whole 128 x 128 tile of floats
LAYOUTS = ("dense", "padded16", "odd", "odd_out", "odd_in")


class Window:
    """rows x cols floats at ``base + front`` with row stride ``ld`` inside a poisoned allocation; ``data`` (rows x cols, or a
    vector for rows == 1) fills an input window, ``data=None`` makes an output window (poisoned inside as well)."""

    def __init__(self, rows, cols, ld=None, col_off=0, data=None, device="cpu", margin_rows=MARGIN_ROWS, margin_words=None):
        ld = cols if ld is None else ld
        assert rows >= 1 and cols >= 1 and ld >= cols and col_off >= 0 and margin_rows >= 128
        self.rows, self.cols, self.ld, self.col_off = rows, cols, ld, col_off
        margin = margin_rows * ld if margin_words is None else margin_words
        self.front = margin + col_off
        self.total = self.front + (rows - 1) * ld + cols + margin
        self.buf = torch.full((self.total,), POISON, dtype=torch.int32, device=device)
        self.output = data is None
        if data is not None:
            self.view.copy_(data.reshape(rows, cols).to(torch.float32))

    @property
    def view(self) -> torch.Tensor:
        """The window as a strided fp32 tensor over the allocation."""
        return self.buf.view(torch.float32).as_strided((self.rows, self.cols), (self.ld, 1), self.front)

    @property
    def bits(self) -> torch.Tensor:
        return self.buf.as_strided((self.rows, self.cols), (self.ld, 1), self.front)

    def data_ptr(self) -> int:
        return self.buf.data_ptr() + 4 * self.front

    def aligned16(self) -> bool:
        return self.data_ptr() % 16 == 0

    def get(self) -> torch.Tensor:
        return self.view.clone()

    def repoison(self):
        assert self.output
        self.bits.fill_(POISON)

    def check_untouched(self, what=""):
        bad = self.buf != POISON
        bad.as_strided((self.rows, self.cols), (self.ld, 1), self.front).fill_(False)
        if bool(bad.any()):
            rel = int(torch.nonzero(bad)[0, 0]) - self.front
            row = rel // self.ld
            raise AssertionError(f"{what}: word outside the {self.rows} x {self.cols} window (ld {self.ld}) changed, first at "
                                 f"(row {row}, col {rel - row * self.ld}) relative to the window")

    def check_written(self, what="", cols=None):
        """No element (of the first ``cols`` columns) still holds the poison."""
        left = self.bits[:, :cols] == POISON
        if bool(left.any()):
            r, c = (int(v) for v in torch.nonzero(left)[0])
            raise AssertionError(f"{what}: element ({r}, {c}) of the {self.rows} x {self.cols} output window was not written")


def form_of(layout: str, role: str) -> str:
    """The form (dense | padded16 | odd) of one operand.  ``role``: "a" = the left operand (A of linear; A and dOut of wgrad),
    "in" = every other input, "out" = outputs together with bias / dbias / slab."""
    assert layout in LAYOUTS and role in ("a", "in", "out")
    if layout == "odd_out":
        return "odd" if role == "out" else "padded16"
    if layout == "odd_in":
        return "odd" if role == "a" else "padded16"
    return layout


def make(layout, role, rows, cols, data=None, device="cpu", strided=True) -> Window:
    """The window of one operand in a named layout.  ``strided=False``: an operand whose entry point takes no leading dimension
    (a vector, packed rows): only the layout's column offset applies."""
    form = form_of(layout, role)
    off = {"dense": 0, "padded16": 4, "odd": 1}[form]
    if not strided or form == "dense":
        ld = cols
    elif form == "padded16":
        ld = (cols + 3) // 4 * 4 + 8
    else:
        ld = cols + 3
    if rows == 1 and not strided:
        return Window(1, cols, cols, off, data, device, margin_words=MARGIN_WORDS)
    return Window(rows, cols, ld, off, data, device)


# ---- references (any dtype) ----------------------------------------------------------------------------------------------------------

def activation(z, act, slope=0.01):
    if act == 1:
        return torch.nn.functional.leaky_relu(z, slope)
    return {0: lambda v: v, 2: torch.relu, 3: torch.sigmoid, 4: torch.tanh}[act](z)


def ref_linear(a, w, b, act, dtype, slope=0.01):
    z = a.to(dtype) @ w.to(dtype).t()
    if b is not None:
        z = z + b.to(dtype)
    return activation(z, act, slope)


def ref_wgrad(d, a, dtype):
    """(dW, dbias) = (d^T a, column sums of d)."""
    return d.to(dtype).t() @ a.to(dtype), d.to(dtype).sum(0)


def csr_dense(rowptr, col, val, ncols, dtype=torch.float64):
    """The dense operator of a CSR (duplicate entries add up)."""
    rowptr, col = rowptr.cpu().long(), col.cpu().long()
    rows = torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr[1:] - rowptr[:-1])
    return torch.zeros(rowptr.numel() - 1, ncols, dtype=dtype).index_put_((rows, col), val.cpu().to(dtype), accumulate=True)


def ref_spmm(op64, x, dtype):
    return op64.to(dtype) @ x.to(dtype)


def attention_counts(edge_index, n):
    """Multiplicity of every in-edge j -> i without self loops, plus one self loop per node: the pattern of GATConv."""
    cnt = torch.zeros(n, n, dtype=torch.float64)
    keep = edge_index[0] != edge_index[1]
    cnt.index_put_((edge_index[1][keep], edge_index[0][keep]), torch.ones(int(keep.sum()), dtype=torch.float64), accumulate=True)
    return cnt + torch.eye(n, dtype=torch.float64)


def ref_gat(xp, us, ud, cnt, slope, dtype):
    """Dense GATConv attention aggregation on packed rows xp (N, T, F), period by period -> (N, T, F)."""
    xp, us, ud, cnt = xp.to(dtype), us.to(dtype), ud.to(dtype), cnt.to(dtype)
    outs = []
    for t in range(xp.shape[1]):
        xt = xp[:, t, :]
        score = torch.nn.functional.leaky_relu((xt @ ud).view(-1, 1) + (xt @ us).view(1, -1), slope)
        w = cnt * torch.exp(score - score.max(dim=1, keepdim=True).values)
        outs.append((w / w.sum(dim=1, keepdim=True)) @ xt)
    return torch.stack(outs, dim=1)


# ---- bars ----------------------------------------------------------------------------------------------------------------------------

def gap_bar(ref32, ref64):
    """(gap, bar): the fp32 evaluation's own distance from float64 and the tolerance gru_math.bar makes of it."""
    gap = rel_err(ref32, ref64)
    return gap, bar(gap)


ABS_ACT_BAR = 2e-5             # act 3 / 4 (outputs bounded by 1): the bar of test_linear_full_tiles_every_row_every_run


def must_be_rounded(layout, n, k):
    """bf16 arithmetic: operands the vector path accepts at a shape the bf16 pipe covers are rounded (the dense tests assert it)."""
    return layout in ("dense", "padded16") and n % 8 == 0 and k % 8 == 0 and k > 32


# ---- the cases of tests/test_gpu_windows.py, with inputs and references computed once ---------------------------------------------

LINEAR_SHAPES = [(1, 1, 1), (7, 4, 4), (129, 68, 36), (129, 65, 33), (8193, 256, 32), (5505, 260, 36)]        # (M, N, K)
LINEAR_ACT_SHAPES = [(129, 68, 36), (8193, 256, 32)]
WGRAD_SHAPES = [(1, 1, 1), (5, 4, 4), (700, 128, 33), (3000, 132, 36), (1037, 260, 132), (16897, 36, 32)]
MODES = (0, 1, 2)              # regt_set_gemm_mode: fp32 MFMA, bf16x3 split, bf16 operands
SPMM_WIDTHS = (4, 36, 96, 132)
DUAL_WIDTHS = (48, 64)
PACK_SHAPES = [(37, 8, 12), (5, 3, 1)]
GAT_F = (4, 12, 100, 132, 256)
GAT_T = (1, 3)
GAT_NODES = 48


@functools.lru_cache(maxsize=None)
def linear_inputs(m, n, k):
    g = torch.Generator().manual_seed(m * 31 + n * 7 + k)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / max(1.0, k ** 0.5)
    b = torch.randn(n, generator=g)
    return a, w, b


@functools.lru_cache(maxsize=None)
def linear_refs(m, n, k, with_bias, act, rounded):
    """(ref64, gap, bar) of one linear case; ``rounded``: both matrix operands rounded to bf16 first (the bias never is)."""
    a, w, b = linear_inputs(m, n, k)
    if rounded:
        a, w = bf16_round(a), bf16_round(w)
    b = b if with_bias else None
    ref64 = ref_linear(a, w, b, act, torch.float64)
    gap, tol = gap_bar(ref_linear(a, w, b, act, torch.float32), ref64)
    return ref64, gap, tol


@functools.lru_cache(maxsize=None)
def wgrad_inputs(m, n, k):
    g = torch.Generator().manual_seed(m + 13 * n + 101 * k)
    return torch.randn(m, n, generator=g), torch.randn(m, k, generator=g)


@functools.lru_cache(maxsize=None)
def wgrad_refs(m, n, k, rounded):
    """((dW64, gap, bar), (db64, gap, bar))."""
    d, a = wgrad_inputs(m, n, k)
    if rounded:
        d, a = bf16_round(d), bf16_round(a)
    dw64, db64 = ref_wgrad(d, a, torch.float64)
    dw32, db32 = ref_wgrad(d, a, torch.float32)
    return (dw64,) + gap_bar(dw32, dw64), (db64,) + gap_bar(db32, db64)


def spmm_graph(n=300):
    """Edges (2, E) and weights: row 0 receives an edge from every other node (hub), rows 200.. receive none, one edge is listed
    twice."""
    g = torch.Generator().manual_seed(n)
    src = torch.cat([torch.arange(1, n), torch.randint(0, n, (900,), generator=g), torch.tensor([7, 7])])
    dst = torch.cat([torch.zeros(n - 1, dtype=torch.long), torch.randint(1, 200, (900,), generator=g), torch.tensor([9, 9])])
    loops = src == dst
    src[loops] = (src[loops] + 1) % n                           # raw_csr drops self loops: list none
    return torch.stack([src, dst]), torch.rand(src.numel(), generator=g) + 0.5


def gat_graph(n=GAT_NODES):
    """Node 0 receives an edge from every other node; the last two nodes receive none (their rows hold the self loop alone);
    one edge is listed twice and one self loop is listed (the pattern drops it and adds its own)."""
    g = torch.Generator().manual_seed(n)
    src = torch.cat([torch.arange(1, n), torch.randint(0, n, (200,), generator=g), torch.tensor([3, 3, 5])])
    dst = torch.cat([torch.zeros(n - 1, dtype=torch.long), torch.randint(1, n - 2, (200,), generator=g), torch.tensor([11, 11, 5])])
    return torch.stack([src, dst])


@functools.lru_cache(maxsize=None)
def gat_case(f, t, n=GAT_NODES, slope=0.2):
    """Inputs and float64 references of one attention case: x in [0, 1), zero-mean score vectors scaled so that the raw scores
    over the pattern reach +-8 (both signs: both branches of the leaky relu, a running maximum that moves)."""
    ei = gat_graph(n)
    cnt = attention_counts(ei, n)
    g = torch.Generator().manual_seed(1000 * f + t)
    xp = torch.rand(n, t, f, generator=g)
    us, ud = torch.randn(f, generator=g), torch.randn(f, generator=g)
    us, ud = us - us.mean(), ud - ud.mean()
    raw = torch.einsum("ntf,f->nt", xp, ud).unsqueeze(1) + torch.einsum("ntf,f->nt", xp, us).unsqueeze(0)      # (i, j, t)
    raw = raw[(cnt > 0)]
    scale = 8.0 / float(raw.abs().max())
    us, ud = us * scale, ud * scale
    go = torch.randn(n, t, f, generator=g)
    us64, ud64 = us.double().requires_grad_(True), ud.double().requires_grad_(True)
    out64 = ref_gat(xp, us64, ud64, cnt, slope, torch.float64)
    (out64 * go.double()).sum().backward()
    us32, ud32 = us.clone().requires_grad_(True), ud.clone().requires_grad_(True)
    out32 = ref_gat(xp, us32, ud32, cnt, slope, torch.float32)
    (out32 * go).sum().backward()
    return {"ei": ei, "xp": xp, "us": us, "ud": ud, "go": go, "raw": raw * scale, "out64": out64.detach(), "dus64": us64.grad,
            "dud64": ud64.grad, "out32": out32.detach(), "dus32": us32.grad, "dud32": ud32.grad}


GAT_OUT_BAR = 1e-5             # absolute, on a convex combination of values in [0, 1); the arithmetic's own per-row bars: gat_math.py


def gat_grad_ok(got, ref64, scale):
    """The bar of test_gat_aggregate_forward_and_score_gradients: atol 2e-5 x scale, rtol 1e-4.  Returns (ok, largest err / bound)."""
    err = (got.double() - ref64).abs()
    bound = 2e-5 * scale + 1e-4 * ref64.abs()
    ratio = float((err / bound).max())
    return ratio <= 1.0, ratio
