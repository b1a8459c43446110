"""Thin tensor-level wrappers over the op-site entry points of the C ABI (used by tests, bench and the
reference-side binding shown in INTEGRATION.md).  No arithmetic happens in Python."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda or t.dtype != torch.float32:
        raise _lib.RegtError(f"{name} must be a float32 CUDA tensor (no CPU path)")
    return t.contiguous()


def pack_x(x: torch.Tensor) -> torch.Tensor:
    """(N,F,T) -> (N,T,F)."""
    x = _f32c(x, "x")
    n, f, t = x.shape
    out = torch.empty(n, t, f, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().regt_pack_x(_lib.ptr(x), _lib.ptr(out), n, f, t, _stream()), "regt_pack_x")
    return out


def _pack_into(name: str, dtype, short: str, x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    x = _f32c(x, "x")
    n, f, t = x.shape
    if (out.dtype != dtype or not out.is_contiguous() or out.device != x.device or out.dim() != 3
            or out.shape[0] < n or tuple(out.shape[1:]) != (t, f)):
        raise ValueError(f"{name}_into: out must be a contiguous {short} (>= {n}, {t}, {f}) tensor on {x.device}")
    _lib.check(getattr(_lib.load(), "regt_" + name)(_lib.ptr(x), _lib.ptr(out), n, f, t, _stream()), "regt_" + name)
    return out


def pack_x_into(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """(N,F,T) -> rows [0, N) of ``out`` (>= N rows of (T,F)); the remaining rows are left alone (halo slots)."""
    return _pack_into("pack_x", torch.float32, "fp32", x, out)


def pack_x_bf16_into(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """(N,F,T) fp32 -> rows [0, N) of the bf16 tensor ``out`` (>= N rows of (T,F)), rounded to nearest even (REGT_GEMM_MODE=bf16:
    the packed rows a region shard exchanges and hands to ``forward_packed``); F % 8 == 0."""
    return _pack_into("pack_x_bf16", torch.bfloat16, "bf16", x, out)


def spmm_dual_bf16(rowptr, col, val_a, val_l, x: torch.Tensor):
    """(A x, L x) as bf16 rows from bf16 rows ``x`` (x_rows >= N, W): fp32 accumulation, one rounding per element; W % 64 == 0."""
    if not x.is_cuda or x.dtype != torch.bfloat16 or x.dim() != 2:
        raise _lib.RegtError("x must be a 2-D bfloat16 CUDA tensor (no CPU path)")
    x = x.contiguous()
    n = rowptr.numel() - 1
    ya = torch.empty(n, x.shape[1], dtype=torch.bfloat16, device=x.device)
    yl = torch.empty_like(ya)
    _lib.check(_lib.load().regt_spmm_dual_bf16(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val_a), _lib.ptr(val_l), _lib.ptr(x),
                                               _lib.ptr(ya), _lib.ptr(yl), n, x.shape[0], x.shape[1], _stream()), "regt_spmm_dual_bf16")
    return ya, yl


def spmm_csr(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, x: torch.Tensor, out: Optional[torch.Tensor] = None):
    """Y[r,:] = sum_e val[e] * X[col[e],:] for r in range(len(rowptr)-1)."""
    x = _f32c(x, "x")
    nrows = rowptr.numel() - 1
    width = x.shape[1]
    if out is None:
        out = torch.empty(nrows, width, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().regt_spmm_csr(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(x), _lib.ptr(out),
                                         nrows, x.shape[0], width, _stream()), "regt_spmm_csr")
    return out


def spmm_dual(rowptr, col, val_a, val_l, x: torch.Tensor):
    """(A x, L x) from the merged two-weight CSR in one gather pass; x.shape[1] % 4 == 0."""
    x = _f32c(x, "x")
    n = rowptr.numel() - 1
    ya = torch.empty(n, x.shape[1], dtype=torch.float32, device=x.device)
    yl = torch.empty_like(ya)
    _lib.check(_lib.load().regt_spmm_dual(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val_a), _lib.ptr(val_l), _lib.ptr(x),
                                          _lib.ptr(ya), _lib.ptr(yl), n, x.shape[1], _stream()), "regt_spmm_dual")
    return ya, yl


def linear(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = 0, slope: float = 0.01):
    """act(a @ w.T + bias) on the fp32 matrix cores."""
    a, w = _f32c(a, "a"), _f32c(w, "w")
    m, k = a.shape
    n = w.shape[0]
    out = torch.empty(m, n, dtype=torch.float32, device=a.device)
    b = None if bias is None else _f32c(bias, "bias")
    _lib.check(_lib.load().regt_linear(_lib.ptr(a), k, m, k, _lib.ptr(w), k, n, _lib.ptr(b), act, slope, _lib.ptr(out), n,
                                       _stream()), "regt_linear")
    return out


def wgrad(dout: torch.Tensor, a: torch.Tensor, with_bias: bool = True):
    """(dout.T @ a, dout.sum(0)) -- the weight / bias gradient of ``linear``."""
    dout, a = _f32c(dout, "dout"), _f32c(a, "a")
    m, n = dout.shape
    k = a.shape[1]
    lib = _lib.load()
    slab = torch.empty(lib.regt_wgrad_slab_floats(m, n, k, 1 if with_bias else 0), dtype=torch.float32, device=a.device)
    dw = torch.empty(n, k, dtype=torch.float32, device=a.device)
    db = torch.empty(n, dtype=torch.float32, device=a.device) if with_bias else None
    _lib.check(lib.regt_wgrad(_lib.ptr(dout), n, _lib.ptr(a), k, m, n, k, _lib.ptr(dw), k, _lib.ptr(db), _lib.ptr(slab),
                              _stream()), "regt_wgrad")
    return dw, db


def mse_loss_grad(pred: torch.Tensor, y: torch.Tensor, global_count: Optional[int] = None):
    """(loss, dloss/dpred) of ``mean((pred - y)**2)`` (run.py:180); mean over ``global_count`` entries."""
    pred, y = _f32c(pred, "pred"), _f32c(y, "y")
    dpred = torch.empty_like(pred)
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    cnt = pred.numel()
    _lib.check(_lib.load().regt_mse_loss_grad(_lib.ptr(pred), _lib.ptr(y), _lib.ptr(dpred), _lib.ptr(loss), cnt,
                                              cnt if global_count is None else global_count, _stream()), "regt_mse_loss_grad")
    return loss, dpred


WINDOW_MAX_T = 255


def window_forward(ring: torch.Tensor, first_slot: int, windows: int, attention: torch.Tensor, l1w: torch.Tensor, l1b: torch.Tensor,
                   l2w: torch.Tensor, l2b: torch.Tensor, pred: Optional[torch.Tensor] = None, hidden: Optional[torch.Tensor] = None):
    """Streaming inference (regt_window_forward): ``ring`` (ring_len, N, C) holds per-time-step cell outputs; window w < ``windows`` is
    ``hidden[w] = sum_p softmax(attention)_p * ring[(first_slot + w + p) % ring_len]`` (p ascending, one fmaf each: the same bits
    whatever ``windows`` / ``first_slot`` / ``ring_len``), ``pred[w]`` the head on it.  Returns ``(pred (windows, N, O), hidden
    (windows, N, C))``; ``pred`` / ``hidden``: contiguous float32 outputs of those shapes to write into, allocated when None.
    ``ring`` must be contiguous (it is not copied); more than one window needs ``windows + T - 1 <= ring_len``."""
    tensors = {"ring": ring, "attention": attention, "l1w": l1w, "l1b": l1b, "l2w": l2w, "l2b": l2b}
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise _lib.RegtError(f"{name} must be a float32 CUDA tensor (no CPU path)")
    if ring.dim() != 3 or not ring.is_contiguous():
        raise ValueError(f"ring must be a contiguous (ring_len, N, C) tensor, got {tuple(ring.shape)} strides {ring.stride()}")
    ring_len, n, c = ring.shape
    if attention.dim() != 1 or not 1 <= attention.numel() <= WINDOW_MAX_T:
        raise ValueError(f"attention must hold 1 .. {WINDOW_MAX_T} logits, got {tuple(attention.shape)}")
    t = attention.numel()
    if l1w.dim() != 2 or l1w.shape[1] != c or l2w.dim() != 2 or l2w.shape[1] != l1w.shape[0]:
        raise ValueError(f"l1w must be (H1, {c}) and l2w (O, H1), got {tuple(l1w.shape)} and {tuple(l2w.shape)}")
    h1, o = l1w.shape[0], l2w.shape[0]
    if tuple(l1b.shape) != (h1,) or tuple(l2b.shape) != (o,):
        raise ValueError(f"l1b must be ({h1},) and l2b ({o},), got {tuple(l1b.shape)} and {tuple(l2b.shape)}")
    first_slot, windows = int(first_slot), int(windows)
    if n < 1 or c < 4 or c % 4:
        raise ValueError(f"ring needs N >= 1 and C a positive multiple of 4, got N={n} C={c}")
    if ring_len < t or not 0 <= first_slot < ring_len or windows < 1:
        raise ValueError(f"need ring_len >= T, 0 <= first_slot < ring_len and windows >= 1 (ring_len={ring_len} T={t} first_slot={first_slot} "
                         f"windows={windows})")
    if windows > 1 and windows + t - 1 > ring_len:
        raise ValueError(f"{windows} windows of {t} periods need {windows + t - 1} slots, the ring has {ring_len} (only a single window may wrap)")
    attention, l1w, l1b, l2w, l2b = (x.detach().contiguous() for x in (attention, l1w, l1b, l2w, l2b))
    for name, out, shape in (("pred", pred, (windows, n, o)), ("hidden", hidden, (windows, n, c))):
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != ring.device
                                or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 {shape} tensor on {ring.device}")
    if pred is None:
        pred = torch.empty(windows, n, o, dtype=torch.float32, device=ring.device)
    if hidden is None:
        hidden = torch.empty(windows, n, c, dtype=torch.float32, device=ring.device)
    lib = _lib.load()
    nbytes = lib.regt_window_workspace_bytes(n, c, h1, o, windows)
    if nbytes == 0:
        _lib.check(1, "regt_window_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ring.device)
    _lib.check(lib.regt_window_forward(_lib.ptr(ring), ring_len, first_slot, windows, n, t, c, o, h1, _lib.ptr(attention), _lib.ptr(l1w),
                                       _lib.ptr(l1b), _lib.ptr(l2w), _lib.ptr(l2b), _lib.ptr(pred), _lib.ptr(hidden), _lib.ptr(ws), nbytes,
                                       _stream()), "regt_window_forward")
    return pred, hidden


def window_backward_max_t() -> int:
    """Periods the window backward covers (regt_window_backward_max_t)."""
    return int(_lib.load().regt_window_backward_max_t())


def window_backward(ring: torch.Tensor, first_slot: int, windows: int, attention: torch.Tensor, l1w: torch.Tensor, l1b: torch.Tensor,
                    l2w: torch.Tensor, l2b: torch.Tensor, hidden: torch.Tensor, dpred: torch.Tensor, dring: torch.Tensor,
                    accumulate: bool, d_attention: torch.Tensor, d_l1w: torch.Tensor, d_l1b: torch.Tensor, d_l2w: torch.Tensor,
                    d_l2b: torch.Tensor) -> None:
    """Streamed training (regt_window_backward): the backward of :func:`window_forward` for the same ``ring`` / ``first_slot`` /
    ``windows``.  ``hidden`` (windows, N, C) is the forward's output, ``dpred`` (windows, N, O) the loss gradient.  The head's backward
    runs on all windows' rows; then ``dring[(first_slot + j) % ring_len] (+)= sum_w softmax(attention)[j - w] * dhidden[w]`` for the
    windows + T - 1 covered slots (windows ascending, one fmaf each, starting from the value ``dring`` holds under ``accumulate``, else
    from 0: the same bits however the windows are split over consecutive accumulating calls), and the gradients of the attention logits
    and of the head go to ``d_attention`` (T), ``d_l1w``, ``d_l1b``, ``d_l2w``, ``d_l2b`` -- added to under ``accumulate``, written
    otherwise.  Slots of ``dring`` outside the covered ones are not touched.  Every output is a contiguous float32 CUDA tensor of its
    parameter's shape, ``dring`` of the ring's; T <= :func:`window_backward_max_t`; ``windows + T - 1 <= ring_len``."""
    inputs = {"ring": ring, "attention": attention, "l1w": l1w, "l1b": l1b, "l2w": l2w, "l2b": l2b, "hidden": hidden, "dpred": dpred,
              "dring": dring, "d_attention": d_attention, "d_l1w": d_l1w, "d_l1b": d_l1b, "d_l2w": d_l2w, "d_l2b": d_l2b}
    for name, t in inputs.items():
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise _lib.RegtError(f"{name} must be a float32 CUDA tensor (no CPU path)")
    if ring.dim() != 3 or not ring.is_contiguous():
        raise ValueError(f"ring must be a contiguous (ring_len, N, C) tensor, got {tuple(ring.shape)} strides {ring.stride()}")
    ring_len, n, c = ring.shape
    lib = _lib.load()
    max_t = int(lib.regt_window_backward_max_t())
    if attention.dim() != 1 or not 1 <= attention.numel() <= max_t:
        raise ValueError(f"attention must hold 1 .. {max_t} logits (the window backward's limit), got {tuple(attention.shape)}")
    t = attention.numel()
    if l1w.dim() != 2 or l1w.shape[1] != c or l2w.dim() != 2 or l2w.shape[1] != l1w.shape[0]:
        raise ValueError(f"l1w must be (H1, {c}) and l2w (O, H1), got {tuple(l1w.shape)} and {tuple(l2w.shape)}")
    h1, o = l1w.shape[0], l2w.shape[0]
    if tuple(l1b.shape) != (h1,) or tuple(l2b.shape) != (o,):
        raise ValueError(f"l1b must be ({h1},) and l2b ({o},), got {tuple(l1b.shape)} and {tuple(l2b.shape)}")
    first_slot, windows = int(first_slot), int(windows)
    if n < 1 or c < 4 or c % 4:
        raise ValueError(f"ring needs N >= 1 and C a positive multiple of 4, got N={n} C={c}")
    if ring_len < t or not 0 <= first_slot < ring_len or windows < 1 or windows + t - 1 > ring_len:
        raise ValueError(f"need 0 <= first_slot < ring_len, windows >= 1 and windows + T - 1 <= ring_len (ring_len={ring_len} T={t} "
                         f"first_slot={first_slot} windows={windows})")
    shapes = {"hidden": (windows, n, c), "dpred": (windows, n, o), "dring": (ring_len, n, c), "d_attention": (t,), "d_l1w": (h1, c),
              "d_l1b": (h1,), "d_l2w": (o, h1), "d_l2b": (o,)}
    for name, shape in shapes.items():
        x = inputs[name]
        if x.device != ring.device or tuple(x.shape) != shape or not x.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 {shape} tensor on {ring.device}, got {tuple(x.shape)} strides {x.stride()}")
    attention, l1w, l1b, l2w, l2b = (x.detach().contiguous() for x in (attention, l1w, l1b, l2w, l2b))
    nbytes = lib.regt_window_backward_workspace_bytes(n, c, h1, o, windows, t)
    if nbytes == 0:
        _lib.check(1, "regt_window_backward_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=ring.device)
    _lib.check(lib.regt_window_backward(_lib.ptr(ring), ring_len, first_slot, windows, n, t, c, o, h1, _lib.ptr(attention), _lib.ptr(l1w),
                                        _lib.ptr(l1b), _lib.ptr(l2w), _lib.ptr(l2b), _lib.ptr(hidden), _lib.ptr(dpred), _lib.ptr(dring),
                                        1 if accumulate else 0, _lib.ptr(d_attention), _lib.ptr(d_l1w), _lib.ptr(d_l1b), _lib.ptr(d_l2w),
                                        _lib.ptr(d_l2b), _lib.ptr(ws), nbytes, _stream()), "regt_window_backward")


def gat_forward(rowptr: torch.Tensor, col: torch.Tensor, xp: torch.Tensor, u_src: torch.Tensor, u_dst: torch.Tensor, slope: float = 0.2):
    """GATConv attention aggregation on packed input rows xp (N,T,F): returns (out (N,T,F), stats (N*T,4))."""
    xp, u_src, u_dst = _f32c(xp, "xp"), _f32c(u_src, "u_src"), _f32c(u_dst, "u_dst")
    n, t, f = xp.shape
    out = torch.empty_like(xp)
    stats = torch.empty(n * t, 4, dtype=torch.float32, device=xp.device)
    _lib.check(_lib.load().regt_gat_forward(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(xp), _lib.ptr(u_src), _lib.ptr(u_dst), slope,
                                            n, t, f, _lib.ptr(out), _lib.ptr(stats), _stream()), "regt_gat_forward")
    return out, stats


def gat_backward(rowptr, col, t_rowptr, t_col, xp: torch.Tensor, u_src: torch.Tensor, dout: torch.Tensor, stats: torch.Tensor,
                 slope: float = 0.2) -> torch.Tensor:
    """Score gradients dsd (N*T, 2) = (dL/ds, dL/dd) of gat_forward given dL/dout (N,T,F)."""
    xp, u_src, dout = _f32c(xp, "xp"), _f32c(u_src, "u_src"), _f32c(dout, "dout")
    n, t, f = xp.shape
    dsd = torch.empty(n * t, 2, dtype=torch.float32, device=xp.device)
    _lib.check(_lib.load().regt_gat_backward(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(t_rowptr), _lib.ptr(t_col), _lib.ptr(xp),
                                             _lib.ptr(u_src), slope, n, t, f, _lib.ptr(dout), _lib.ptr(stats), _lib.ptr(dsd), _stream()),
               "regt_gat_backward")
    return dsd


SPATIAL_CHANNELS = 64        # out_channels of SpatialGCN's first ChebConv (models/SpatialGCN.py:14)


def _keep_ptr(keep: Optional[torch.Tensor], rows: int, dev):
    if keep is None:
        return None
    if keep.dtype != torch.int32 or not keep.is_cuda or keep.device != dev or tuple(keep.shape) != (rows, 2) or not keep.is_contiguous():
        raise ValueError(f"keep must be a contiguous int32 ({rows}, 2) tensor on {dev}")
    return _lib.ptr(keep)


def spatial_embed_forward(xp: torch.Tensor, lxp: torch.Tensor, w0: torch.Tensor, w1: torch.Tensor, bias: torch.Tensor,
                          keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """S (N, 64) = sum_t keep_t * 2 * relu(x_t W0^T + lx_t W1^T + b) from packed rows xp, lxp (N, T, F); keep (N*T, 2) int32 mask
    bits (row node*T + t, bit j of word w keeps channel 32w + j) or None (eval: no mask, no scale)."""
    xp, lxp = _f32c(xp, "x_packed"), _f32c(lxp, "lx_packed")
    w0, w1, bias = _f32c(w0, "w0"), _f32c(w1, "w1"), _f32c(bias, "bias")
    n, t, f = xp.shape
    if tuple(lxp.shape) != (n, t, f) or tuple(w0.shape) != (SPATIAL_CHANNELS, f) or tuple(w1.shape) != (SPATIAL_CHANNELS, f) \
            or bias.numel() != SPATIAL_CHANNELS:
        raise ValueError("spatial_embed_forward: inconsistent shapes")
    s = torch.empty(n, SPATIAL_CHANNELS, dtype=torch.float32, device=xp.device)
    _lib.check(_lib.load().regt_spatial_embed_forward(_lib.ptr(xp), _lib.ptr(lxp), _lib.ptr(w0), _lib.ptr(w1), _lib.ptr(bias),
                                                      _keep_ptr(keep, n * t, xp.device), n, t, f, _lib.ptr(s), _stream()),
               "regt_spatial_embed_forward")
    return s


def spatial_embed_backward(xp: torch.Tensor, lxp: torch.Tensor, w0: torch.Tensor, w1: torch.Tensor, bias: torch.Tensor,
                           keep: Optional[torch.Tensor], ds: torch.Tensor, return_scratch: bool = False):
    """(dW0, dW1, db) of :func:`spatial_embed_forward` given dL/dS (N, 64); with ``return_scratch`` also the slab the kernels left
    (per-wave partial rows, then the chunk sums), for tests of the reduction order."""
    xp, lxp = _f32c(xp, "x_packed"), _f32c(lxp, "lx_packed")
    w0, w1, bias, ds = _f32c(w0, "w0"), _f32c(w1, "w1"), _f32c(bias, "bias"), _f32c(ds, "ds")
    n, t, f = xp.shape
    if tuple(ds.shape) != (n, SPATIAL_CHANNELS):
        raise ValueError(f"ds must be ({n}, {SPATIAL_CHANNELS})")
    lib = _lib.load()
    nslab = lib.regt_spatial_embed_slab_floats(n, t, f)
    if nslab == 0:
        raise _lib.RegtError(f"regt_spatial_embed_slab_floats: unsupported dims N={n} T={t} F={f}")
    slab = torch.empty(nslab, dtype=torch.float32, device=xp.device)
    dw0, dw1 = torch.empty_like(w0), torch.empty_like(w1)
    db = torch.empty(SPATIAL_CHANNELS, dtype=torch.float32, device=xp.device)
    _lib.check(lib.regt_spatial_embed_backward(_lib.ptr(xp), _lib.ptr(lxp), _lib.ptr(w0), _lib.ptr(w1), _lib.ptr(bias),
                                               _keep_ptr(keep, n * t, xp.device), _lib.ptr(ds), n, t, f, _lib.ptr(dw0), _lib.ptr(dw1),
                                               _lib.ptr(db), _lib.ptr(slab), _stream()), "regt_spatial_embed_backward")
    return (dw0, dw1, db, slab) if return_scratch else (dw0, dw1, db)


# ---- STNorm (models/STNorm.py) -------------------------------------------------------------------------------------------------------

STNORM_CHANNELS = 16         # channels the kernels are built for (models/STNorm.py default)
STNORM_HEAD, STNORM_PER_LAYER = 6, 12
STNORM_MAX_DIM = 256         # in_dim / out_dim: the LDS rows of the start-conv and head backward kernels (include/regtgcn.h)


def stnorm_dims(n: int, batch: int, tnorm_group: int, seq_len: int, in_dim: int, out_dim: int, blocks: int, layers: int,
                tnorm: bool, snorm: bool, training: bool) -> _lib.StnormDims:
    return _lib.StnormDims(n, batch, tnorm_group, seq_len, in_dim, out_dim, blocks, layers, int(bool(tnorm)), int(bool(snorm)),
                           int(bool(training)))


def _sizes(entry: str, dims):
    ws, sc = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(getattr(_lib.load(), entry)(ctypes.byref(dims), ctypes.byref(ws), ctypes.byref(sc)), entry)
    return ws.value, sc.value


def stnorm_sizes(dims: _lib.StnormDims):
    """(workspace floats, scratch floats) of regt_stnorm_forward / _backward."""
    return _sizes("regt_stnorm_sizes", dims)


def _ptr_table(tensors):
    return (ctypes.c_void_p * max(1, len(tensors)))(*[None if t is None else t.data_ptr() for t in tensors])


def _check_table(what: str, kind: str, tensors, shapes, device, off: str = ""):
    """RegtError unless every entry of ``tensors`` is a contiguous float32 tensor of its shape in ``shapes`` on ``device``, or None
    where the shape is None (``off`` names the switch that is off there): the kernels read the entries through raw device pointers."""
    for i, (t, shape) in enumerate(zip(tensors, shapes)):
        if shape is None:
            if t is not None:
                raise _lib.RegtError(f"{what}: {kind} entry {i} must be None ({off})")
            continue
        if not isinstance(t, torch.Tensor):
            raise _lib.RegtError(f"{what}: {kind} entry {i} is missing")
        if t.dtype != torch.float32 or t.device != torch.device(device) or not t.is_contiguous() or tuple(t.shape) != shape:
            raise _lib.RegtError(f"{what}: {kind} entry {i} must be a contiguous float32 {shape} tensor on {device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}" + ("" if t.is_contiguous() else " (not contiguous)"))


def _check_dout(dout: torch.Tensor, shape, device):
    if tuple(dout.shape) != shape or dout.device != device:
        raise ValueError(f"dout must be {shape} on {device}, got {tuple(dout.shape)} on {dout.device}")


def _check_ws(ws: Optional[torch.Tensor], floats: int, device, source: str, saved=True):
    """``ws`` has to be what ``source`` left for the backward: the kernels read ``floats`` floats of it (``saved``: the forward's
    dims said so)."""
    if not saved or ws is None or ws.dtype != torch.float32 or ws.device != device or ws.numel() != floats or not ws.is_contiguous():
        raise ValueError(f"ws must be the workspace {source} returned for these dims")


def stnorm_out_len(seq_len: int, blocks: int, layers: int) -> int:
    rf = 1 + blocks * ((1 << layers) - 1)
    return max(seq_len, rf) - rf + 1


def stnorm_table_shapes(dims: _lib.StnormDims):
    """Expected shapes of the parameter table (None where the entry must be None) and of the running-buffer table."""
    c, n, k = STNORM_CHANNELS, dims.num_nodes, (1 + bool(dims.tnorm) + bool(dims.snorm)) * STNORM_CHANNELS
    shapes = [(c, dims.in_dim, 1, 1), (c,), (c, c, 1, 1), (c,), (dims.out_dim, c, 1, 1), (dims.out_dim,)]
    running = []
    for _ in range(dims.blocks * dims.layers):
        shapes += [(c, k, 1, 2), (c,), (c, k, 1, 2), (c,), (c, c, 1, 1), (c,), (c, c, 1, 1), (c,)]
        shapes += [(1, c, n, 1)] * 2 if dims.tnorm else [None, None]
        shapes += [(c,)] * 2 if dims.snorm else [None, None]
        running += [(1, c, n, 1)] * 2 if dims.tnorm else []
    return shapes, running


def stnorm_check_tables(dims: _lib.StnormDims, device, params, running, what: str = "STNorm"):
    """RegtError unless every parameter and running buffer is a contiguous float32 tensor of its reference shape on ``device``:
    the kernels read them through raw device pointers."""
    shapes, rshapes = stnorm_table_shapes(dims)
    if len(params) != len(shapes) or len(running) != len(rshapes):
        raise _lib.RegtError(f"{what}: expected {len(shapes)} parameter and {len(rshapes)} buffer entries, got {len(params)}, {len(running)}")
    _check_table(what, "parameter", params, shapes, device, "TNorm / SNorm off")
    _check_table(what, "running buffer", running, rshapes, device)


def stnorm_forward(dims: _lib.StnormDims, x: torch.Tensor, params, running):
    """out (B, O, N, L_out) of STNorm for x (B, L, N, C_in); ``params`` in the table order of regt_stnorm_forward (None where TNorm /
    SNorm is off), ``running`` [rm_0, rv_0, rm_1, ...] (updated in place in training mode).  Returns (out, workspace): the workspace
    holds what regt_stnorm_backward reads."""
    x = _f32c(x, "x")
    if tuple(x.shape) != (dims.batch, dims.seq_len, dims.num_nodes, dims.in_dim):
        raise ValueError(f"x must be ({dims.batch}, {dims.seq_len}, {dims.num_nodes}, {dims.in_dim}), got {tuple(x.shape)}")
    stnorm_check_tables(dims, x.device, params, running, "regt_stnorm_forward")
    ws_n, _ = stnorm_sizes(dims)
    out = torch.empty(dims.batch, dims.out_dim, dims.num_nodes, stnorm_out_len(dims.seq_len, dims.blocks, dims.layers),
                      dtype=torch.float32, device=x.device)
    ws = torch.empty(ws_n, dtype=torch.float32, device=x.device)
    pt, rt = _ptr_table(params), _ptr_table(running)
    _lib.check(_lib.load().regt_stnorm_forward(ctypes.byref(dims), _lib.ptr(x), pt, rt if dims.tnorm else None, _lib.ptr(out),
                                               _lib.ptr(ws), _stream()), "regt_stnorm_forward")
    return out, ws


def stnorm_backward(dims: _lib.StnormDims, x: torch.Tensor, params, running, dout: torch.Tensor, ws: torch.Tensor):
    """Gradients of every entry of ``params`` (None where the entry is None) from dL/dout; ``ws`` is the forward's workspace."""
    x, dout = _f32c(x, "x"), _f32c(dout, "dout")
    stnorm_check_tables(dims, x.device, params, running, "regt_stnorm_backward")
    ws_n, sc_n = stnorm_sizes(dims)
    out_shape = (dims.batch, dims.out_dim, dims.num_nodes, stnorm_out_len(dims.seq_len, dims.blocks, dims.layers))
    _check_dout(dout, out_shape, x.device)
    _check_ws(ws, ws_n, x.device, "stnorm_forward")
    sc = torch.empty(sc_n, dtype=torch.float32, device=x.device)
    grads = [None if p is None else torch.empty_like(p) for p in params]
    pt, rt, gt = _ptr_table(params), _ptr_table(running), _ptr_table(grads)
    _lib.check(_lib.load().regt_stnorm_backward(ctypes.byref(dims), _lib.ptr(x), pt, rt if dims.tnorm else None, _lib.ptr(dout), gt,
                                                _lib.ptr(ws), _lib.ptr(sc), _stream()), "regt_stnorm_backward")
    return grads


# ---- STID (models/STID.py) -----------------------------------------------------------------------------------------------------------

STID_DIM = 32                # embed_dim and node_dim the kernels are built for (models/STID.py defaults)
STID_MAX_LAYERS = 8
STID_MAX_KIN = 192           # input_dim * input_len: rows of the embedding weight in LDS (include/regtgcn.h)
STID_MAX_OUT = 64
STID_DROPOUT = 0.15          # nn.Dropout(p=0.15) of models/STID.py:15


def stid_limits(input_len: int, output_len: int, input_dim: int, embed_dim: int, node_dim: int, num_layer: int):
    """ValueError naming the field unless the dims are inside what regt_stid_* accept (include/regtgcn.h)."""
    if embed_dim != STID_DIM or node_dim != STID_DIM:
        raise ValueError(f"STID runs with embed_dim = node_dim = {STID_DIM} only, got embed_dim={embed_dim}, node_dim={node_dim}")
    if not 1 <= num_layer <= STID_MAX_LAYERS:
        raise ValueError(f"STID runs with 1 <= num_layer <= {STID_MAX_LAYERS}, got num_layer={num_layer}")
    if not 1 <= input_len <= 255:
        raise ValueError(f"STID runs with 1 <= input_len <= 255, got input_len={input_len}")
    if not 1 <= input_dim <= 256 or input_dim * input_len > STID_MAX_KIN:
        raise ValueError(f"STID runs with 1 <= input_dim <= 256 and input_dim * input_len <= {STID_MAX_KIN}, got input_dim={input_dim}, "
                         f"input_len={input_len}")
    if not 1 <= output_len <= STID_MAX_OUT:
        raise ValueError(f"STID runs with 1 <= output_len <= {STID_MAX_OUT}, got output_len={output_len}")


def stid_dims(n: int, batch: int, input_len: int, in_features: int, input_dim: int, num_layer: int, output_len: int, if_node: bool = True,
              embed_dim: int = STID_DIM, node_dim: int = STID_DIM, dropout_p: float = STID_DROPOUT) -> _lib.StidDims:
    return _lib.StidDims(n, batch, input_len, in_features, input_dim, embed_dim, node_dim, num_layer, output_len, int(bool(if_node)),
                         float(dropout_p))


def stid_hidden(dims: _lib.StidDims) -> int:
    return dims.embed_dim + (dims.node_dim if dims.if_node else 0)


def stid_sizes(dims: _lib.StidDims):
    """(workspace floats, scratch floats) of regt_stid_forward / _backward."""
    return _sizes("regt_stid_sizes", dims)


def stid_table_shapes(dims: _lib.StidDims):
    """Expected shapes of the parameter table in state_dict order (None: the entry must be None, if_node off)."""
    h = stid_hidden(dims)
    shapes = [(dims.num_nodes, dims.node_dim) if dims.if_node else None, (dims.embed_dim, dims.input_dim * dims.input_len, 1, 1),
              (dims.embed_dim,)]
    for _ in range(dims.num_layer):
        shapes += [(h, h, 1, 1), (h,), (h, h, 1, 1), (h,)]
    return shapes + [(dims.output_len, h, 1, 1), (dims.output_len,)]


def stid_check_tables(dims: _lib.StidDims, device, params, what: str = "STID"):
    """RegtError unless every parameter is a contiguous float32 tensor of its reference shape on ``device``: the kernels read them
    through raw device pointers."""
    shapes = stid_table_shapes(dims)
    if len(params) != len(shapes):
        raise _lib.RegtError(f"{what}: expected {len(shapes)} parameter entries, got {len(params)}")
    _check_table(what, "parameter", params, shapes, device, "if_node off")


def stid_keep_shape(dims: _lib.StidDims):
    return (dims.num_layer, dims.batch, dims.num_nodes, stid_hidden(dims) // 32)


def _stid_keep_ptr(dims: _lib.StidDims, keep: Optional[torch.Tensor], dev):
    if keep is None:
        return None
    shape = stid_keep_shape(dims)
    if keep.dtype != torch.int32 or keep.device != dev or tuple(keep.shape) != shape or not keep.is_contiguous():
        raise ValueError(f"keep must be a contiguous int32 {shape} tensor on {dev}")
    return _lib.ptr(keep)


def _stid_x(dims: _lib.StidDims, x: torch.Tensor) -> torch.Tensor:
    x = _f32c(x, "x")
    shape = (dims.batch, dims.input_len, dims.num_nodes, dims.in_features)
    if tuple(x.shape) != shape:
        raise ValueError(f"x must be {shape}, got {tuple(x.shape)}")
    return x


def stid_forward(dims: _lib.StidDims, x: torch.Tensor, params, keep: Optional[torch.Tensor] = None, save: bool = True):
    """out (B, output_len, N, 1) of STID for x (B, L, N, C); ``params`` in state_dict order (None for node_emb when if_node is off);
    ``keep``: int32 keep bits (num_layer, B, N, hidden / 32) or None (eval).  Returns (out, workspace): with ``save`` the workspace
    holds what regt_stid_backward reads, else it is None."""
    x = _stid_x(dims, x)
    stid_check_tables(dims, x.device, params, "regt_stid_forward")
    kp = _stid_keep_ptr(dims, keep, x.device)
    out = torch.empty(dims.batch, dims.output_len, dims.num_nodes, 1, dtype=torch.float32, device=x.device)
    ws = torch.empty(stid_sizes(dims)[0], dtype=torch.float32, device=x.device) if save else None
    _lib.check(_lib.load().regt_stid_forward(ctypes.byref(dims), _lib.ptr(x), _ptr_table(params), kp, _lib.ptr(out),
                                             None if ws is None else _lib.ptr(ws), _stream()), "regt_stid_forward")
    return out, ws


def stid_backward(dims: _lib.StidDims, x: torch.Tensor, params, keep: Optional[torch.Tensor], dout: torch.Tensor, ws: torch.Tensor,
                  return_scratch: bool = False):
    """Gradients of every entry of ``params`` (None where the entry is None) from dL/dout; ``ws`` is the forward's workspace and
    ``keep`` the keep bits it ran with.  With ``return_scratch``: (gradients, scratch), the scratch as the kernels left it (the
    workgroups' slabs, then the per-batch node-embedding rows), for tests of the reduction order."""
    x, dout = _stid_x(dims, x), _f32c(dout, "dout")
    stid_check_tables(dims, x.device, params, "regt_stid_backward")
    kp = _stid_keep_ptr(dims, keep, x.device)
    ws_n, sc_n = stid_sizes(dims)
    out_shape = (dims.batch, dims.output_len, dims.num_nodes, 1)
    _check_dout(dout, out_shape, x.device)
    _check_ws(ws, ws_n, x.device, "stid_forward(save=True)")
    sc = torch.empty(sc_n, dtype=torch.float32, device=x.device)
    grads = [None if p is None else torch.empty_like(p) for p in params]
    _lib.check(_lib.load().regt_stid_backward(ctypes.byref(dims), _lib.ptr(x), _ptr_table(params), kp, _lib.ptr(dout), _ptr_table(grads),
                                              _lib.ptr(ws), _lib.ptr(sc), _stream()), "regt_stid_backward")
    return (grads, sc) if return_scratch else grads


# ---- GRU layer and StackedGRU (models/StackedGRU.py) ---------------------------------------------------------------------------------

GRU_HIDDEN = 256             # hidden size the kernels are built for (models/StackedGRU.py:7)
GRU_MAX_INPUT = 255


def gru_limits(input_size: int, hidden: int = GRU_HIDDEN):
    """ValueError naming the field unless the sizes are inside what regt_gru_* accept (include/regtgcn.h)."""
    if hidden != GRU_HIDDEN:
        raise ValueError(f"the GRU kernels run with hidden = {GRU_HIDDEN} only, got hidden={hidden}")
    if not 1 <= input_size <= GRU_MAX_INPUT:
        raise ValueError(f"the GRU kernels run with 1 <= input_size <= {GRU_MAX_INPUT}, got input_size={input_size}")


def gru_dims(seq_len: int, rows: int, input_size: int, x_strides=None, training: bool = True, hidden: int = GRU_HIDDEN) -> _lib.GruDims:
    """``x_strides``: element strides of x over (step, row, input); default: a contiguous (seq_len, rows, input_size) tensor."""
    ss, sr, st = (rows * input_size, input_size, 1) if x_strides is None else x_strides
    return _lib.GruDims(seq_len, rows, input_size, hidden, int(bool(training)), ss, sr, st)


def gru_sizes(dims: _lib.GruDims):
    """(workspace floats, scratch floats) of regt_gru_forward / _backward."""
    return _sizes("regt_gru_sizes", dims)


def _gru_x(x: torch.Tensor) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
        raise _lib.RegtError("x must be a float32 CUDA tensor (no CPU path)")
    if x.dim() != 3:
        raise ValueError(f"x must be (seq_len, rows, input_size), got {tuple(x.shape)}")
    if any(s < 0 for s in x.stride()) or x.data_ptr() % 4:
        x = x.contiguous()
    return x


def gru_check_weights(input_size: int, device, weights, what: str = "GRU"):
    """RegtError unless the four tensors are contiguous float32 (768, input_size), (768, 256), (768,), (768,) on ``device``: the
    kernels read them through raw device pointers."""
    g = 3 * GRU_HIDDEN
    shapes = [(g, input_size), (g, GRU_HIDDEN), (g,), (g,)]
    if len(weights) != 4:
        raise _lib.RegtError(f"{what}: expected weight_ih, weight_hh, bias_ih, bias_hh, got {len(weights)} entries")
    _check_table(what, "weight", weights, shapes, device)


def _gru_state(t: Optional[torch.Tensor], rows: int, dev, name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = _f32c(t, name)
    if t.numel() != rows * GRU_HIDDEN or t.shape[-1] != GRU_HIDDEN or t.device != dev:
        raise ValueError(f"{name} must hold ({rows}, {GRU_HIDDEN}) values on {dev}, got {tuple(t.shape)} on {t.device}")
    return t


def gru_forward(x: torch.Tensor, weights, h0: Optional[torch.Tensor] = None, want_out: bool = True, want_last: bool = True,
                save: bool = True):
    """One GRU layer over x (seq_len, rows, input_size), read in place through its strides.  ``weights``: weight_ih, weight_hh,
    bias_ih, bias_hh of torch.nn.GRU.  Returns (out (seq_len, rows, 256) | None, h_last (1, rows, 256) | None, dims, workspace);
    with ``save`` the workspace holds what regt_gru_backward reads."""
    x = _gru_x(x)
    n, rows, t = x.shape
    gru_limits(t)
    gru_check_weights(t, x.device, weights, "regt_gru_forward")
    if not (want_out or want_last):
        raise ValueError("gru_forward: nothing to compute (want_out and want_last are both off)")
    h0 = _gru_state(h0, rows, x.device, "h0")
    dims = gru_dims(n, rows, t, x.stride(), save)
    ws = torch.empty(gru_sizes(dims)[0], dtype=torch.float32, device=x.device)
    out = torch.empty(n, rows, GRU_HIDDEN, dtype=torch.float32, device=x.device) if want_out else None
    last = torch.empty(1, rows, GRU_HIDDEN, dtype=torch.float32, device=x.device) if want_last else None
    _lib.check(_lib.load().regt_gru_forward(ctypes.byref(dims), _lib.ptr(x), *[_lib.ptr(w) for w in weights], _lib.ptr(h0), _lib.ptr(out),
                                            _lib.ptr(last), _lib.ptr(ws), _stream()), "regt_gru_forward")
    return out, last, dims, ws


def gru_backward(dims: _lib.GruDims, x: torch.Tensor, weights, dout: Optional[torch.Tensor], dh_last: Optional[torch.Tensor],
                 ws: torch.Tensor, want_dh0: bool = False, return_scratch: bool = False):
    """(gradients of weight_ih, weight_hh, bias_ih, bias_hh; dh0 (1, rows, 256) | None) from dL/dout and / or dL/dh_last; ``dims``
    and ``ws`` are what gru_forward(save=True) returned for the same x.  With ``return_scratch`` a third entry: the scratch as the
    kernels left it (its tail is the hidden gradients' slab), for tests of the reduction order."""
    x = _gru_x(x)
    if tuple(x.shape) != (dims.seq_len, dims.rows, dims.input_size) or tuple(x.stride()) != (dims.x_stride_seq, dims.x_stride_row,
                                                                                             dims.x_stride_t):
        raise ValueError("gru_backward: x must be the tensor gru_forward ran on")
    gru_check_weights(dims.input_size, x.device, weights, "regt_gru_backward")
    if dout is not None:
        dout = _f32c(dout, "dout")
        _check_dout(dout, (dims.seq_len, dims.rows, GRU_HIDDEN), x.device)
    dh_last = _gru_state(dh_last, dims.rows, x.device, "dh_last")
    if dout is None and dh_last is None:
        raise ValueError("gru_backward: dout and dh_last are both None")
    ws_n, sc_n = gru_sizes(dims)
    _check_ws(ws, ws_n, x.device, "gru_forward(save=True)", dims.training)
    sc = torch.empty(sc_n, dtype=torch.float32, device=x.device)
    grads = [torch.empty_like(w) for w in weights]
    dh0 = torch.empty(1, dims.rows, GRU_HIDDEN, dtype=torch.float32, device=x.device) if want_dh0 else None
    _lib.check(_lib.load().regt_gru_backward(ctypes.byref(dims), _lib.ptr(x), _ptr_table(weights), None, _lib.ptr(dout), _lib.ptr(dh_last),
                                             _ptr_table(grads), _lib.ptr(dh0), _lib.ptr(ws), _lib.ptr(sc), _stream()), "regt_gru_backward")
    return (grads, dh0, sc) if return_scratch else (grads, dh0)


def relu_backward_(y: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """relu's gradient in place: d = 0 where y <= 0."""
    y, dd = _f32c(y, "y"), _f32c(d, "d")
    if dd.data_ptr() != d.data_ptr() or y.numel() != d.numel():
        raise ValueError("relu_backward_: d must be contiguous and of y's size")
    _lib.check(_lib.load().regt_relu_backward(_lib.ptr(y), _lib.ptr(d), d.numel(), _stream()), "regt_relu_backward")
    return d


# ---- STAEformer inference (models/STAEformer.py) ---------------------------------------------------------------------------------------

STAE_HEAD_DIM = 32           # head width the attention kernel is built for (include/regtgcn.h)
STAE_MAX_DIM = 256           # model_dim
STAE_MAX_FF = 1024           # feed_forward_dim
STAE_MAX_LAYERS = 8
STAE_MAX_OUT = 64            # out_steps * output_dim
STAE_LN_EPS = 1e-5           # nn.LayerNorm's default, which the reference keeps


def stae_limits(in_steps: int, out_steps: int, input_dim: int, output_dim: int, model_dim: int, num_heads: int, feed_forward_dim: int,
                num_layers: int, use_mixed_proj: bool = True):
    """NotImplementedError naming the limits unless the construction is inside what regt_stae_* accept (include/regtgcn.h)."""
    limits = (f"STAEformer runs with head width model_dim / num_heads == {STAE_HEAD_DIM}, model_dim a multiple of 32 up to {STAE_MAX_DIM}, "
              f"feed_forward_dim a multiple of 32 up to {STAE_MAX_FF}, 1 <= in_steps <= 255, 1 <= num_layers <= {STAE_MAX_LAYERS}, "
              f"input_dim >= 1, out_steps * output_dim <= {STAE_MAX_OUT} and use_mixed_proj=True")
    ok = (use_mixed_proj and num_heads >= 1 and model_dim == num_heads * STAE_HEAD_DIM and model_dim <= STAE_MAX_DIM
          and feed_forward_dim >= 32 and feed_forward_dim % 32 == 0 and feed_forward_dim <= STAE_MAX_FF and 1 <= in_steps <= 255
          and 1 <= num_layers <= STAE_MAX_LAYERS and 1 <= input_dim <= 256 and out_steps >= 1 and output_dim >= 1
          and out_steps * output_dim <= STAE_MAX_OUT)
    if not ok:
        raise NotImplementedError(f"{limits}; got model_dim={model_dim}, num_heads={num_heads}, feed_forward_dim={feed_forward_dim}, "
                                  f"in_steps={in_steps}, num_layers={num_layers}, input_dim={input_dim}, out_steps={out_steps}, "
                                  f"output_dim={output_dim}, use_mixed_proj={use_mixed_proj}")


def stae_model_dim(dims: _lib.StaeDims) -> int:
    return (dims.input_embedding_dim + dims.tod_embedding_dim + dims.dow_embedding_dim + dims.spatial_embedding_dim
            + dims.adaptive_embedding_dim)


def stae_sizes(dims: _lib.StaeDims) -> int:
    """Workspace floats of regt_stae_forward."""
    ws = ctypes.c_size_t()
    _lib.check(_lib.load().regt_stae_sizes(ctypes.byref(dims), ctypes.byref(ws)), "regt_stae_sizes")
    return ws.value


def stae_table_shapes(dims: _lib.StaeDims):
    """Expected shapes of the parameter table in state_dict order (None: the entry must be None, that embedding is off)."""
    d, ff, n, t = stae_model_dim(dims), dims.feed_forward_dim, dims.num_nodes, dims.in_steps
    shapes = [(n, dims.spatial_embedding_dim) if dims.spatial_embedding_dim else None,
              (t, n, dims.adaptive_embedding_dim) if dims.adaptive_embedding_dim else None,
              (dims.input_embedding_dim, dims.input_dim), (dims.input_embedding_dim,),
              (dims.steps_per_day, dims.tod_embedding_dim) if dims.tod_embedding_dim else None,
              (dims.days_per_week, dims.dow_embedding_dim) if dims.dow_embedding_dim else None,
              (dims.out_steps * dims.output_dim, t * d), (dims.out_steps * dims.output_dim,)]
    for _ in range(2 * dims.num_layers):
        shapes += [(d, d), (d,)] * 4 + [(ff, d), (ff,), (d, ff), (d,)] + [(d,)] * 4
    return shapes


def stae_check_tables(dims: _lib.StaeDims, device, params, what: str = "STAEformer"):
    """RegtError unless every parameter is a contiguous float32 tensor of its reference shape on ``device``: the kernels read them
    through raw device pointers."""
    shapes = stae_table_shapes(dims)
    if len(params) != len(shapes):
        raise _lib.RegtError(f"{what}: expected {len(shapes)} parameter entries, got {len(params)}")
    _check_table(what, "parameter", params, shapes, device, "embedding width 0")


def stae_forward(dims: _lib.StaeDims, x: torch.Tensor, params) -> torch.Tensor:
    """out (B, out_steps, N, output_dim) of STAEformer in inference for x (B, T, N, F); ``params`` in state_dict order (None where an
    embedding is off).  The whole launch sequence is one C call; nothing is kept for a backward."""
    x = _f32c(x, "x")
    shape = (dims.batch, dims.in_steps, dims.num_nodes, dims.in_features)
    if tuple(x.shape) != shape:
        raise ValueError(f"x must be {shape}, got {tuple(x.shape)}")
    stae_check_tables(dims, x.device, params, "regt_stae_forward")
    ws = torch.empty(stae_sizes(dims), dtype=torch.float32, device=x.device)
    out = torch.empty(dims.batch, dims.out_steps, dims.num_nodes, dims.output_dim, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().regt_stae_forward(ctypes.byref(dims), _lib.ptr(x), _ptr_table(params), _lib.ptr(out), _lib.ptr(ws), _stream()),
               "regt_stae_forward")
    return out


def _stae_rows(t: torch.Tensor, name: str, rows: int, width: int) -> int:
    """Row stride of a (rows, width) float32 CUDA view whose rows are dense (a column window of a wider buffer is fine)."""
    if not t.is_cuda or t.dtype != torch.float32:
        raise _lib.RegtError(f"{name} must be a float32 CUDA tensor (no CPU path)")
    if t.dim() != 2 or tuple(t.shape) != (rows, width) or t.stride(1) != 1:
        raise ValueError(f"{name} must be a ({rows}, {width}) view with unit column stride, got {tuple(t.shape)} strides {t.stride()}")
    return t.stride(0) if rows > 1 else max(t.stride(0), width)


def stae_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, batch: int, in_steps: int, num_nodes: int, heads: int, axis: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(Q K^T / sqrt(32)) V per head along ``axis`` (1: time, 2: nodes) of (B, T, N, 32 * heads) rows.  q, k, v: (M, 32 * heads)
    views with one common row stride (for instance column windows of a Q|K|V buffer); ``out``: an (M, 32 * heads) view, allocated
    when None."""
    m, d = batch * in_steps * num_nodes, heads * STAE_HEAD_DIM
    ld = _stae_rows(q, "q", m, d)
    if _stae_rows(k, "k", m, d) != ld or _stae_rows(v, "v", m, d) != ld:
        raise ValueError("q, k and v must share one row stride")
    if out is None:
        out = torch.empty(m, d, dtype=torch.float32, device=q.device)
    ldo = _stae_rows(out, "out", m, d)
    _lib.check(_lib.load().regt_stae_attention(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), ld, batch, in_steps, num_nodes, heads, axis,
                                               _lib.ptr(out), ldo, _stream()), "regt_stae_attention")
    return out


def stae_add_layernorm(residual: torch.Tensor, y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = STAE_LN_EPS,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm(residual + y) * gamma + beta over the last axis of (M, D) rows; ``out`` may be ``residual`` itself (in place)."""
    if out is not None and out is not residual and (not out.is_contiguous() or out.shape != residual.shape or out.dtype != torch.float32
                                                    or out.device != residual.device):
        raise ValueError("out must be a contiguous float32 tensor of residual's shape on its device")
    if out is residual and not residual.is_contiguous():
        raise ValueError("an in-place residual must be contiguous")
    residual, y, gamma, beta = _f32c(residual, "residual"), _f32c(y, "y"), _f32c(gamma, "gamma"), _f32c(beta, "beta")
    m, d = residual.shape
    if tuple(y.shape) != (m, d) or tuple(gamma.shape) != (d,) or tuple(beta.shape) != (d,):
        raise ValueError(f"y must be ({m}, {d}) and gamma, beta ({d},)")
    if out is None:
        out = torch.empty_like(residual)
    _lib.check(_lib.load().regt_stae_add_layernorm(_lib.ptr(residual), _lib.ptr(y), _lib.ptr(gamma), _lib.ptr(beta), eps, m, d,
                                                   _lib.ptr(out), _stream()), "regt_stae_add_layernorm")
    return out


# ---- STAEformer training: the self-attention layer's backward (csrc/staeformer_bwd.hip) ------------------------------------------------

def stae_layer_limits(model_dim: int, num_heads: int, feed_forward_dim: int):
    """NotImplementedError naming the limit unless one self-attention layer is inside what the kernels and the dense entry points take."""
    if num_heads < 1 or model_dim != num_heads * STAE_HEAD_DIM:
        raise NotImplementedError(f"SelfAttentionLayer runs with head width model_dim / num_heads == {STAE_HEAD_DIM} only, got "
                                  f"model_dim={model_dim}, num_heads={num_heads}")
    if model_dim > STAE_MAX_DIM:
        raise NotImplementedError(f"SelfAttentionLayer runs with model_dim <= {STAE_MAX_DIM}, got model_dim={model_dim}")
    if feed_forward_dim < 32 or feed_forward_dim % 32 or feed_forward_dim > STAE_MAX_FF:
        raise NotImplementedError(f"SelfAttentionLayer runs with feed_forward_dim a multiple of 32 in [32, {STAE_MAX_FF}] (what the dense "
                                  f"entry points regt_linear / regt_wgrad are used with here), got feed_forward_dim={feed_forward_dim}")


def stae_attention_train(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, batch: int, in_steps: int, num_nodes: int, heads: int, axis: int,
                         out: Optional[torch.Tensor] = None):
    """:func:`stae_attention` for training: (out, lse), lse (M, heads) the log-sum-exp of each (row, head)'s scaled scores.  ``out`` is
    the same, bit for bit, as :func:`stae_attention`'s."""
    m, d = batch * in_steps * num_nodes, heads * STAE_HEAD_DIM
    ld = _stae_rows(q, "q", m, d)
    if _stae_rows(k, "k", m, d) != ld or _stae_rows(v, "v", m, d) != ld:
        raise ValueError("q, k and v must share one row stride")
    if out is None:
        out = torch.empty(m, d, dtype=torch.float32, device=q.device)
    ldo = _stae_rows(out, "out", m, d)
    lse = torch.empty(m, heads, dtype=torch.float32, device=q.device)
    _lib.check(_lib.load().regt_stae_attention_train(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), ld, batch, in_steps, num_nodes, heads, axis,
                                                     _lib.ptr(out), ldo, _lib.ptr(lse), _stream()), "regt_stae_attention_train")
    return out, lse


def stae_attention_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor,
                            batch: int, in_steps: int, num_nodes: int, heads: int, axis: int, grads: Optional[torch.Tensor] = None):
    """(dq, dk, dv) of :func:`stae_attention_train` given dL/dout: the three (M, 32 * heads) column windows of one (M, 3 * 32 * heads)
    buffer (``grads``: any 2-D float32 view with unit column stride at least that large, whose first 3 * 32 * heads columns are used;
    allocated when None).  q, k, v share a row stride, out and dout share one."""
    m, d = batch * in_steps * num_nodes, heads * STAE_HEAD_DIM
    ld = _stae_rows(q, "q", m, d)
    if _stae_rows(k, "k", m, d) != ld or _stae_rows(v, "v", m, d) != ld:
        raise ValueError("q, k and v must share one row stride")
    ldo = _stae_rows(out, "out", m, d)
    if _stae_rows(dout, "dout", m, d) != ldo:
        raise ValueError("out and dout must share one row stride")
    if not lse.is_cuda or lse.dtype != torch.float32 or tuple(lse.shape) != (m, heads) or not lse.is_contiguous():
        raise _lib.RegtError(f"lse must be a contiguous float32 CUDA ({m}, {heads}) tensor (no CPU path)")
    if grads is None:
        grads = torch.empty(m, 3 * d, dtype=torch.float32, device=q.device)
    dq, dk, dv = grads[:, :d], grads[:, d:2 * d], grads[:, 2 * d:3 * d]
    ldg = _stae_rows(dq, "dq", m, d)
    if _stae_rows(dk, "dk", m, d) != ldg or _stae_rows(dv, "dv", m, d) != ldg:
        raise ValueError("grads must hold three (M, 32 * heads) column windows")
    lib = _lib.load()
    n = lib.regt_stae_attention_backward_scratch_floats(batch, in_steps, num_nodes, heads)
    if n == 0:
        raise _lib.RegtError("regt_stae_attention_backward_scratch_floats: " + lib.regt_last_error().decode("utf-8", "replace"))
    scratch = torch.empty(n, dtype=torch.float32, device=q.device)
    _lib.check(lib.regt_stae_attention_backward(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), ld, _lib.ptr(out), _lib.ptr(dout), ldo, _lib.ptr(lse),
                                                batch, in_steps, num_nodes, heads, axis, _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), ldg,
                                                _lib.ptr(scratch), _stream()), "regt_stae_attention_backward")
    return dq, dk, dv


def stae_add_layernorm_backward(residual: torch.Tensor, y: torch.Tensor, gamma: torch.Tensor, dout: torch.Tensor, eps: float = STAE_LN_EPS):
    """(dz, dgamma, dbeta) of ``LayerNorm(residual + y) * gamma + beta`` given dL/dout; dz (M, D) is the gradient of both residual and y.
    The row statistics are recomputed from residual and y exactly as :func:`stae_add_layernorm` computes them."""
    residual, y, gamma, dout = _f32c(residual, "residual"), _f32c(y, "y"), _f32c(gamma, "gamma"), _f32c(dout, "dout")
    if residual.dim() != 2:
        raise ValueError(f"residual must be (M, D), got {tuple(residual.shape)}")
    m, d = residual.shape
    if tuple(y.shape) != (m, d) or tuple(dout.shape) != (m, d) or tuple(gamma.shape) != (d,):
        raise ValueError(f"y and dout must be ({m}, {d}) and gamma ({d},)")
    lib = _lib.load()
    n = lib.regt_stae_add_layernorm_backward_scratch_floats(m, d)
    if n == 0:
        raise _lib.RegtError("regt_stae_add_layernorm_backward_scratch_floats: " + lib.regt_last_error().decode("utf-8", "replace"))
    scratch = torch.empty(n, dtype=torch.float32, device=residual.device)
    dz = torch.empty_like(residual)
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
    _lib.check(lib.regt_stae_add_layernorm_backward(_lib.ptr(residual), _lib.ptr(y), _lib.ptr(gamma), _lib.ptr(dout), eps, m, d, _lib.ptr(dz),
                                                    _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(scratch), _stream()),
               "regt_stae_add_layernorm_backward")
    return dz, dgamma, dbeta


# ---- STAEformer training: the whole model (csrc/staeformer_train.hip) -------------------------------------------------------------------

def _scratch(lib, name: str, device, *args) -> torch.Tensor:
    n = getattr(lib, name)(*args)
    if n == 0:
        raise _lib.RegtError(f"{name}: " + lib.regt_last_error().decode("utf-8", "replace"))
    return torch.empty(n, dtype=torch.float32, device=device)


def _stae_x(dims: _lib.StaeDims, x: torch.Tensor) -> torch.Tensor:
    x = _f32c(x, "x")
    shape = (dims.batch, dims.in_steps, dims.num_nodes, dims.in_features)
    if tuple(x.shape) != shape:
        raise ValueError(f"x must be {shape}, got {tuple(x.shape)}")
    return x


def _stae_act(dims: _lib.StaeDims, t: torch.Tensor, name: str) -> torch.Tensor:
    t = _f32c(t, name)
    shape = (dims.batch * dims.in_steps * dims.num_nodes, stae_model_dim(dims))
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    return t


def stae_embed(dims: _lib.StaeDims, x: torch.Tensor, params) -> torch.Tensor:
    """Layer 0's input (M, model_dim) for x (B, T, N, F): input_proj | tod | dow | node_emb | adaptive_embedding, by the kernel
    regt_stae_forward starts with.  ``params``: the first six entries of the parameter table (None where an embedding is off)."""
    x = _stae_x(dims, x)
    _check_table("regt_stae_embed", "parameter", params, stae_table_shapes(dims)[:6], x.device, "embedding width 0")
    out = torch.empty(dims.batch * dims.in_steps * dims.num_nodes, stae_model_dim(dims), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().regt_stae_embed(ctypes.byref(dims), _lib.ptr(x), _ptr_table(list(params)), _lib.ptr(out), _stream()),
               "regt_stae_embed")
    return out


def stae_embed_backward(dims: _lib.StaeDims, x: torch.Tensor, dx0: torch.Tensor):
    """Gradients of :func:`stae_embed`'s six parameters given dL/dX0 (M, model_dim), in table order (None where an embedding is off).
    A table row's gradient goes to the row the forward read after its clamp; x gets none."""
    x, dx0 = _stae_x(dims, x), _stae_act(dims, dx0, "dx0")
    lib = _lib.load()
    scratch = _scratch(lib, "regt_stae_embed_backward_scratch_floats", x.device, ctypes.byref(dims))
    grads = [None if s is None else torch.empty(s, dtype=torch.float32, device=x.device) for s in stae_table_shapes(dims)[:6]]
    _lib.check(lib.regt_stae_embed_backward(ctypes.byref(dims), _lib.ptr(x), _lib.ptr(dx0), _ptr_table(grads), _lib.ptr(scratch), _stream()),
               "regt_stae_embed_backward")
    return grads


def _stae_proj_params(dims: _lib.StaeDims, w: torch.Tensor, b: Optional[torch.Tensor], device):
    shapes = stae_table_shapes(dims)[6:8]
    _check_table("regt_stae_output_proj", "parameter", [w] if b is None else [w, b], shapes[:1] if b is None else shapes, device)


def stae_output_proj(dims: _lib.StaeDims, x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """out (B, out_steps, N, output_dim) of the use_mixed_proj tail for x (M, model_dim), by the kernel regt_stae_forward ends with."""
    x = _stae_act(dims, x, "x")
    _stae_proj_params(dims, w, b, x.device)
    out = torch.empty(dims.batch, dims.out_steps, dims.num_nodes, dims.output_dim, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().regt_stae_output_proj(ctypes.byref(dims), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), _stream()),
               "regt_stae_output_proj")
    return out


def stae_output_proj_backward(dims: _lib.StaeDims, x: torch.Tensor, w: torch.Tensor, dout: torch.Tensor, need_dx: bool = True):
    """(dx, dw, db) of :func:`stae_output_proj` given dL/dout (B, out_steps, N, output_dim), read in place through its strides (a
    strided window or an expanded tensor is fine); dx is None unless ``need_dx``."""
    x = _stae_act(dims, x, "x")
    _stae_proj_params(dims, w, None, x.device)
    shape = (dims.batch, dims.out_steps, dims.num_nodes, dims.output_dim)
    if not dout.is_cuda or dout.dtype != torch.float32:
        raise _lib.RegtError("dout must be a float32 CUDA tensor (no CPU path)")
    _check_dout(dout, shape, x.device)
    if any(s < 0 for s in dout.stride()):
        dout = dout.contiguous()
    lib = _lib.load()
    scratch = _scratch(lib, "regt_stae_output_proj_backward_scratch_floats", x.device, ctypes.byref(dims))
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(w)
    db = torch.empty(w.shape[0], dtype=torch.float32, device=x.device)
    _lib.check(lib.regt_stae_output_proj_backward(ctypes.byref(dims), _lib.ptr(x), _lib.ptr(w), _lib.ptr(dout), *dout.stride(), _lib.ptr(dx),
                                                  _lib.ptr(dw), _lib.ptr(db), _lib.ptr(scratch), _stream()), "regt_stae_output_proj_backward")
    return dx, dw, db


def _stae_keep(keep: Optional[torch.Tensor], m: int, d: int, device, p: float) -> Optional[torch.Tensor]:
    if not 0.0 <= p < 1.0:
        raise ValueError(f"p must be in [0, 1), got {p}")
    if keep is None:
        return None
    if keep.dtype != torch.int32 or tuple(keep.shape) != (m, d // 32) or keep.device != device or not keep.is_contiguous():
        raise _lib.RegtError(f"keep must be a contiguous int32 ({m}, {d // 32}) tensor on {device}, got {keep.dtype} {tuple(keep.shape)} "
                             f"on {keep.device}")
    return keep


def stae_drop_add_layernorm(residual: torch.Tensor, y: torch.Tensor, keep: Optional[torch.Tensor], p: float, gamma: torch.Tensor,
                            beta: torch.Tensor, eps: float = STAE_LN_EPS) -> torch.Tensor:
    """LayerNorm(residual + keep * y / (1 - p)) * gamma + beta over (M, D) rows; ``keep`` int32 (M, D / 32), bit j of word w keeps column
    32 w + j.  ``keep=None``: no dropout and no scaling, the bits of :func:`stae_add_layernorm`."""
    residual, y, gamma, beta = _f32c(residual, "residual"), _f32c(y, "y"), _f32c(gamma, "gamma"), _f32c(beta, "beta")
    if residual.dim() != 2:
        raise ValueError(f"residual must be (M, D), got {tuple(residual.shape)}")
    m, d = residual.shape
    if tuple(y.shape) != (m, d) or tuple(gamma.shape) != (d,) or tuple(beta.shape) != (d,):
        raise ValueError(f"y must be ({m}, {d}) and gamma, beta ({d},)")
    keep = _stae_keep(keep, m, d, residual.device, p)
    out = torch.empty_like(residual)
    _lib.check(_lib.load().regt_stae_drop_add_layernorm(_lib.ptr(residual), _lib.ptr(y), _lib.ptr(keep), p, _lib.ptr(gamma), _lib.ptr(beta), eps,
                                                        m, d, _lib.ptr(out), _stream()), "regt_stae_drop_add_layernorm")
    return out


def stae_drop_add_layernorm_backward(residual: torch.Tensor, y: torch.Tensor, keep: Optional[torch.Tensor], p: float, gamma: torch.Tensor,
                                     dout: torch.Tensor, eps: float = STAE_LN_EPS):
    """(dz, dy, dgamma, dbeta) of :func:`stae_drop_add_layernorm` given dL/dout: dz (M, D) the gradient of residual, dy = keep * dz /
    (1 - p) that of y, written in the same pass.  ``keep=None``: dy is dz itself."""
    residual, y, gamma, dout = _f32c(residual, "residual"), _f32c(y, "y"), _f32c(gamma, "gamma"), _f32c(dout, "dout")
    if residual.dim() != 2:
        raise ValueError(f"residual must be (M, D), got {tuple(residual.shape)}")
    m, d = residual.shape
    if tuple(y.shape) != (m, d) or tuple(dout.shape) != (m, d) or tuple(gamma.shape) != (d,):
        raise ValueError(f"y and dout must be ({m}, {d}) and gamma ({d},)")
    keep = _stae_keep(keep, m, d, residual.device, p)
    lib = _lib.load()
    scratch = _scratch(lib, "regt_stae_drop_add_layernorm_backward_scratch_floats", residual.device, m, d)
    dz = torch.empty_like(residual)
    dy = None if keep is None else torch.empty_like(residual)
    dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
    _lib.check(lib.regt_stae_drop_add_layernorm_backward(_lib.ptr(residual), _lib.ptr(y), _lib.ptr(keep), p, _lib.ptr(gamma), _lib.ptr(dout), eps,
                                                         m, d, _lib.ptr(dz), _lib.ptr(dy), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(scratch),
                                                         _stream()), "regt_stae_drop_add_layernorm_backward")
    return dz, (dz if keep is None else dy), dgamma, dbeta


# ---- one TGCN cell step (regt_tgcn_*; functional.TGCNStepFunction builds the structs and owns the workspace) ---------------------------

def tgcn_dims(n: int, f: int, c: int, arith: int = 0, flags: int = 0) -> _lib.Dims:
    """regt_dims of one cell step: T = 1, regional = 0; R, O and H1 are ignored by the cell-only entry points."""
    return _lib.Dims(n, 1, f, c, 1, 1, 1, 0, 0.0, int(arith), int(flags))


def tgcn_forward(dims: _lib.Dims, gs: _lib.Graph, ps: _lib.Params, x: torch.Tensor, h_in: Optional[torch.Tensor], h_out: torch.Tensor,
                 ws: torch.Tensor) -> torch.Tensor:
    """h_out (N, C) = TGCN(x (N, F), A_hat, h_in (N, C) or None = zeros); ``ws``: regt_tgcn_workspace_bytes(dims) bytes."""
    _lib.check(_lib.load().regt_tgcn_forward(ctypes.byref(dims), ctypes.byref(gs), ctypes.byref(ps), _lib.ptr(x), _lib.ptr(h_in),
                                             _lib.ptr(h_out), _lib.ptr(ws), ws.numel(), _stream()), "regt_tgcn_forward")
    return h_out


def tgcn_backward(dims: _lib.Dims, gs: _lib.Graph, ps: _lib.Params, gr: _lib.Grads, dh_out: torch.Tensor, h_in: Optional[torch.Tensor],
                  h_out: torch.Tensor, op, dx: Optional[torch.Tensor], dh_in: Optional[torch.Tensor], ws: torch.Tensor) -> None:
    """Parameter gradients into ``gr``; ``dx`` (N, F) / ``dh_in`` (N, C) are written where given (None = not wanted).  ``op``: the
    GcnOperator, whose transposed CSR carries dAx back to x."""
    _lib.check(_lib.load().regt_tgcn_backward(ctypes.byref(dims), ctypes.byref(gs), ctypes.byref(ps), ctypes.byref(gr), _lib.ptr(dh_out),
                                              _lib.ptr(h_in), _lib.ptr(h_out), _lib.ptr(op.t_rowptr), _lib.ptr(op.t_col), _lib.ptr(op.t_val),
                                              _lib.ptr(dx), _lib.ptr(dh_in), _lib.ptr(ws), ws.numel(), _stream()), "regt_tgcn_backward")


def input_gradient(dims: _lib.Dims, gs: _lib.Graph, ps: _lib.Params, t_op, dx: torch.Tensor, ws: torch.Tensor,
                   scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """regt_input_gradient: dL/dx (N, F, T) into ``dx`` from what regt_backward left in ``ws``.  ``t_op``: (t_rowptr, t_col, t_val_a,
    t_val_l) of ``PreparedGraph.transposed_merged`` (None: the library refuses the call with its reason).  ``scratch``: a uint8 tensor of
    at least regt_input_gradient_scratch_bytes (default: allocated here)."""
    lib = _lib.load()
    if scratch is None:
        nbytes = lib.regt_input_gradient_scratch_bytes(ctypes.byref(dims))
        if nbytes == 0:
            _lib.check(1, "regt_input_gradient_scratch_bytes")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dx.device)
    t = t_op if t_op is not None else (None, None, None, None)
    _lib.check(lib.regt_input_gradient(ctypes.byref(dims), ctypes.byref(gs), ctypes.byref(ps), _lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]),
                                       _lib.ptr(t[3]), _lib.ptr(dx), _lib.ptr(ws), ws.numel(), _lib.ptr(scratch), scratch.numel(), _stream()),
               "regt_input_gradient")
    return dx
