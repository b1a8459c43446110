"""autograd bridge: one Function = one regt_forward / regt_backward pair of the C ABI."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, List, Optional

import torch

from . import _lib
from .graph import PreparedGraph
from .ops import _stream

HEAD_HIDDEN = 128

# canonical parameter order handed to the Function (state_dict names of the reference)
GATES = ("z", "r", "h")
PARAM_NAMES_COMMON = (
    ["tgnn._attention"]
    + [f"tgnn._base_tgcn.conv_{k}.lin.weight" for k in GATES]
    + [f"tgnn._base_tgcn.conv_{k}.bias" for k in GATES]
    + [f"tgnn._base_tgcn.linear_{k}.weight" for k in GATES]
    + [f"tgnn._base_tgcn.linear_{k}.bias" for k in GATES]
    + ["tgnn.conv.lins.0.weight", "tgnn.conv.lins.1.weight", "tgnn.conv.bias"]
)
PARAM_NAMES_REGION = ["tgnn.linear.weight", "tgnn.linear.bias"]
PARAM_NAMES_HEAD = ["linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias"]


# parameters whose last dimension is the node-feature width F
F_WIDE_PARAMS = tuple([f"tgnn._base_tgcn.conv_{k}.lin.weight" for k in GATES] + ["tgnn.conv.lins.0.weight", "tgnn.conv.lins.1.weight"])


def param_names(regional: bool) -> List[str]:
    return PARAM_NAMES_COMMON + (PARAM_NAMES_REGION if regional else []) + PARAM_NAMES_HEAD


def _fill(struct, tensors: Dict[str, Optional[torch.Tensor]], regional: bool):
    g = lambda n: None if tensors.get(n) is None else tensors[n].data_ptr()
    struct.attention = g("tgnn._attention")
    for i, k in enumerate(GATES):
        struct.conv_lin_w[i] = g(f"tgnn._base_tgcn.conv_{k}.lin.weight")
        struct.conv_bias[i] = g(f"tgnn._base_tgcn.conv_{k}.bias")
        struct.gate_w[i] = g(f"tgnn._base_tgcn.linear_{k}.weight")
        struct.gate_b[i] = g(f"tgnn._base_tgcn.linear_{k}.bias")
    struct.cheb_w0 = g("tgnn.conv.lins.0.weight")
    struct.cheb_w1 = g("tgnn.conv.lins.1.weight")
    struct.cheb_bias = g("tgnn.conv.bias")
    struct.region_w = g("tgnn.linear.weight") if regional else None
    struct.region_b = g("tgnn.linear.bias") if regional else None
    struct.head1_w = g("linear1.weight")
    struct.head1_b = g("linear1.bias")
    struct.head2_w = g("linear2.weight")
    struct.head2_b = g("linear2.bias")
    return struct


class _WorkspacePool:
    """The forward leaves its activations in a multi-GB workspace that the backward reads.  Blocks are recycled
    here (keyed by device and size) instead of going back to the allocator after every step: a step then never
    depends on allocator behaviour for its one large buffer, and two forwards in flight simply use two blocks.  Blocks are
    keyed by the launch stream as well (like the caching allocator's own free lists): work enqueued on another stream may still be
    using a block that the host has already released."""

    def __init__(self):
        self._free = {}
        self._stream_of = {}

    def acquire(self, nbytes: int, device) -> torch.Tensor:
        stream = _stream()
        lst = self._free.get((device, stream, nbytes))
        ws = lst.pop() if lst else torch.empty(nbytes, dtype=torch.uint8, device=device)
        self._stream_of[ws.data_ptr()] = stream
        return ws

    def release(self, ws: torch.Tensor):
        stream = self._stream_of.pop(ws.data_ptr(), None)
        lst = self._free.setdefault((ws.device, stream, ws.numel()), [])
        if len(lst) < 2:
            lst.append(ws)


_POOL = _WorkspacePool()


class _WsHandle:
    """A pooled block of ``nbytes``; returns it to the pool when the autograd node that owns it goes away."""

    def __init__(self, nbytes: int, device):
        self.ws = _POOL.acquire(nbytes, device)

    def release_now(self):
        """A forward-only call gives its block back when it returns.  Stream-ordered: the pool hands the block out again on this
        stream only."""
        _POOL.release(self.ws)
        self.ws = None

    def __del__(self):
        try:
            if self.ws is not None:              # (a forward-only call has released its block already)
                _POOL.release(self.ws)
        except Exception:  # interpreter shutdown
            pass


def _workspace_bytes(sizer: str, *args) -> int:
    """What the library's ``sizer`` asks for ``args``; it returns 0 for dims it refuses (the reason is in regt_last_error)."""
    nbytes = getattr(_lib.load(), sizer)(*args)
    if nbytes == 0:
        _lib.check(1, sizer)
    return nbytes


def _graph_struct(graph: PreparedGraph, periods: int) -> _lib.Graph:
    cache = graph.__dict__.setdefault("_struct_cache", {})       # the struct only holds pointers into the graph's own tensors
    if periods in cache:
        return cache[periods]
    tab, reg, n = graph.chunks_for(periods)
    g = _lib.Graph()
    g.rowptr, g.col, g.val = graph.rowptr.data_ptr(), graph.col.data_ptr(), graph.val.data_ptr()
    g.node_region = graph.node_region.data_ptr()
    g.chunk_tab, g.chunk_region, g.n_chunks = tab.data_ptr(), reg.data_ptr(), n
    if graph.m_rowptr is not None:
        g.m_rowptr, g.m_col = graph.m_rowptr.data_ptr(), graph.m_col.data_ptr()
        g.m_val_a, g.m_val_l = graph.m_val_a.data_ptr(), graph.m_val_l.data_ptr()
    g.overlap = 1 if graph.overlap else 0
    g.region_lo, g.region_hi = graph.region_lo, graph.region_hi
    g.region_sorted = 1 if graph.region_sorted else 0
    cache[periods] = g
    return g


# run.py accumulates the gradients of all snapshots of an epoch before one optimiser step (run.py:178-194): with autograd doing the
# accumulation every backward ends in one `p.grad += g` kernel per parameter (21 launches of ~6 us each).  With this switch on,
# RegTGCNFunction.backward adds its gradients to the existing `.grad` tensors itself -- ONE multi-tensor add -- and returns None
# for the parameters (autograd then has nothing left to accumulate); a parameter without `.grad` receives this call's gradient
# tensor directly.  Same values bit for bit (`tests/test_gpu_model.py`).  Off by default: `torch.autograd.grad(...)` and tensor
# hooks on the parameters would see no gradient; `train.py` and `bench.py` (plain `loss.backward()` loops) switch it on.
_ACCUMULATE_IN_BACKWARD = False


def set_grad_accumulation_in_backward(flag: bool) -> bool:
    """Returns the previous setting."""
    global _ACCUMULATE_IN_BACKWARD
    prev, _ACCUMULATE_IN_BACKWARD = _ACCUMULATE_IN_BACKWARD, bool(flag)
    return prev


@contextlib.contextmanager
def grad_accumulation_in_backward():
    """:func:`set_grad_accumulation_in_backward` on for the body (a plain ``loss.backward()`` loop); the previous setting is back on exit."""
    prev = set_grad_accumulation_in_backward(True)
    try:
        yield
    finally:
        set_grad_accumulation_in_backward(prev)


def _deliver_grads(params, grads):
    """Gradients of ``params`` as autograd's return values, or, under :func:`set_grad_accumulation_in_backward`, added to ``.grad``
    here (one fused add) with None returned for each."""
    live = [(p, g) for p, g in zip(params, grads) if p is not None and g is not None]
    if _ACCUMULATE_IN_BACKWARD and all(p.is_leaf and p.requires_grad for p, _ in live):
        have, new = [], []
        for p, g in live:
            if p.grad is None:
                p.grad = g                       # (this call's own buffer, which nothing else refers to)
            else:
                have.append(p.grad)
                new.append(g)
        if have:
            torch._foreach_add_(have, new)
        return (None,) * len(params)
    return tuple(grads)


def _upstream_grads(dpred, dhidden, dims, device):
    """The gradients of ``(pred, hidden)`` as the library reads them: contiguous, zeros for a ``pred`` the loss did not use; the
    gradient of an unused ``hidden`` stays None (the Functions do not materialise it)."""
    if dpred is None:
        dpred = torch.zeros(dims.N, dims.O, dtype=torch.float32, device=device)
    return dpred.contiguous(), None if dhidden is None else dhidden.contiguous()


# Evaluation (train.evaluate*, evaluate.predict_metrics*, a plain model(x) under torch.no_grad()) needs no backward: the modules then
# call the library with REGT_DIMS_FORWARD_ONLY -- same pred / hidden bit for bit, no activation stores, a workspace of
# regt_forward_only_workspace_bytes (no M x C array at all on the fused bf16 forward, four instead of nine elsewhere) that goes back
# to the pool when the call returns.  The decision is made by the callers of the Functions below (inside Function.forward grad mode
# is always off).  The switch exists for A/B tests and as an escape hatch.
_FORWARD_ONLY_IN_NO_GRAD = True


def set_forward_only_in_no_grad(flag: bool) -> bool:
    """Returns the previous setting."""
    global _FORWARD_ONLY_IN_NO_GRAD
    prev, _FORWARD_ONLY_IN_NO_GRAD = _FORWARD_ONLY_IN_NO_GRAD, bool(flag)
    return prev


def wants_forward_only(*tensors) -> bool:
    """True when no gradient can be asked of a forward on ``tensors`` (grad mode off, or none of them requires one)."""
    if not _FORWARD_ONLY_IN_NO_GRAD:
        return False
    return not torch.is_grad_enabled() or not any(t_ is not None and t_.requires_grad for t_ in tensors)


class _FwdState:
    """What one regt_forward / regt_cell_forward call leaves for its backward; the Function keeps it on ``ctx`` as it is.  ``graph``
    is the prepared graph or operator (the pointer structs point into its tensors), ``saved`` the tensors that go to
    ``save_for_backward`` after ``hidden``; the cell fills only the first five."""
    __slots__ = ("graph", "dims", "handle", "wsb", "saved", "regional", "ps", "gs", "xp", "names", "f_real", "f_pad")

    def __init__(self, **fields):
        for k, v in fields.items():
            setattr(self, k, v)


def _regt_forward_call(x: torch.Tensor, graph: PreparedGraph, regional: bool, slope: float, packed, params, forward_only: bool,
                       hidden_out: Optional[torch.Tensor] = None):
    """The library call behind :class:`RegTGCNFunction` and :func:`regt_run`: returns ``(pred, hidden, state)``; ``state`` is
    None for a forward-only call (its workspace block is back in the pool).  ``hidden_out``: a contiguous float32 (N, C) tensor the
    library writes ``hidden`` into instead of a fresh one (a ring slab of serve.StreamingPredictor)."""
    arith = flags = 0
    if isinstance(packed, tuple):
        packed, arith, flags = packed
    if forward_only:
        flags = int(flags) | _lib.DIMS_FORWARD_ONLY
    lib = _lib.load()
    if not x.is_cuda:
        raise _lib.RegtError("RegT-GCN forward needs CUDA/HIP tensors: there is no CPU path in this package")
    xbf = packed and x.dtype == torch.bfloat16        # region shard that packs and exchanges its rows as bf16 (REGT_GEMM_MODE=bf16)
    if (x.dtype != torch.float32 and not xbf) or x.dim() != 3:
        raise ValueError(f"x must be float32 (N,F,T) (or packed bfloat16 (x_rows,T,F)), got {x.dtype} {tuple(x.shape)}")
    names = param_names(regional)
    if len(params) != len(names):
        raise ValueError(f"expected {len(names)} parameter tensors, got {len(params)}")
    for n_, p_ in zip(names, params):
        if p_.dtype != torch.float32 or not p_.is_cuda or not p_.is_contiguous():
            raise ValueError(f"parameter {n_} must be a contiguous float32 CUDA tensor")
    x = x.contiguous()
    # The kernels read 16-byte feature rows (F a multiple of 4; the reference uses F = 8).  Any other width is staged
    # padded: zero feature columns in x and zero weight columns for them change nothing in the forward, and their
    # gradient columns (ds^T x_pad = 0) are sliced off in the backward.
    f_real = x.shape[2] if packed else x.shape[1]
    f_pad = (-f_real) % 4
    if f_pad and xbf:
        raise ValueError("bf16 packed input needs a feature width that is a multiple of 4")
    if f_pad:
        x = torch.nn.functional.pad(x, (0, f_pad) if packed else (0, 0, 0, f_pad)).contiguous()
        params = tuple(torch.nn.functional.pad(p_, (0, f_pad)).contiguous() if n_ in F_WIDE_PARAMS else p_
                       for n_, p_ in zip(names, params))
    if packed:
        x_rows, T, F = x.shape
        N = graph.num_nodes
        if x_rows < N:
            raise ValueError(f"packed input has {x_rows} rows but the shard owns {N} nodes")
    else:
        N, F, T = x.shape
        x_rows = N
        if N != graph.num_nodes:
            raise ValueError(f"x has {N} nodes but the prepared graph has {graph.num_nodes}")
    # shape validation, the dims / parameter-pointer structs and the workspace size only depend on (shapes, parameter
    # addresses): remembered per graph, so a steady-state step skips ~60 us of Python (TPIMS-scale steps are host-bound)
    plan_key = (N, T, F, x_rows, regional, float(slope), arith, flags, tuple((p_.data_ptr(), tuple(p_.shape)) for p_ in params))
    plans = graph.__dict__.setdefault("_plan_cache", {})
    plan = plans.get(plan_key)
    if plan is None:
        tens = dict(zip(names, params))
        Cdim = tens["tgnn.conv.bias"].numel()
        O = tens["linear2.weight"].shape[0]
        H1 = tens["linear1.weight"].shape[0]
        R = graph.num_regions
        expect = {"tgnn._attention": (T,), "tgnn.conv.lins.0.weight": (Cdim, F), "tgnn.conv.lins.1.weight": (Cdim, F),
                  "linear1.weight": (H1, Cdim), "linear2.weight": (O, H1)}
        for k in GATES:
            expect[f"tgnn._base_tgcn.conv_{k}.lin.weight"] = (Cdim, F)
            expect[f"tgnn._base_tgcn.linear_{k}.weight"] = (Cdim, 2 * Cdim)
        if regional:
            expect["tgnn.linear.weight"] = (Cdim, R * Cdim)
        for k, shp in expect.items():
            if tuple(tens[k].shape) != shp:
                raise ValueError(f"parameter {k} has shape {tuple(tens[k].shape)}, expected {shp}")
        dims = _lib.Dims(N, T, F, Cdim, R, O, H1, 1 if regional else 0, float(slope), int(arith), int(flags))
        gs = _graph_struct(graph, T)
        if forward_only and packed:                   # (x_rows and the row type enter the form and the layout)
            wsb = _workspace_bytes("regt_forward_only_packed_workspace_bytes", C.byref(dims), C.byref(gs), x_rows, 1 if xbf else 0)
        elif forward_only:
            wsb = _workspace_bytes("regt_forward_only_workspace_bytes", C.byref(dims), C.byref(gs))
        else:
            wsb = _workspace_bytes("regt_workspace_bytes", C.byref(dims), gs.n_chunks, gs.overlap)
        if len(plans) > 16:
            plans.clear()
        plan = plans[plan_key] = (dims, gs, wsb, _fill(_lib.Params(), tens, regional), Cdim, O)
    dims, gs, wsb, ps, Cdim, O = plan
    handle = _WsHandle(wsb, x.device)
    ws = handle.ws
    # (DIMS_NO_HEAD: the library runs no head and takes a NULL pred)
    pred = None if int(flags) & _lib.DIMS_NO_HEAD else torch.empty(N, O, dtype=torch.float32, device=x.device)
    if hidden_out is None:
        hidden = torch.empty(N, Cdim, dtype=torch.float32, device=x.device)
    else:
        if (hidden_out.dtype != torch.float32 or hidden_out.device != x.device or tuple(hidden_out.shape) != (N, Cdim)
                or not hidden_out.is_contiguous() or hidden_out.data_ptr() % 16):
            raise ValueError(f"hidden_out must be a contiguous, 16-byte aligned float32 ({N}, {Cdim}) tensor on {x.device}")
        hidden = hidden_out
    if xbf:
        _lib.check(lib.regt_forward_packed_bf16(C.byref(dims), C.byref(gs), C.byref(ps), _lib.ptr(x), x_rows, _lib.ptr(pred),
                                                _lib.ptr(hidden), _lib.ptr(ws), wsb, _stream()), "regt_forward_packed_bf16")
    elif packed:
        _lib.check(lib.regt_forward_packed(C.byref(dims), C.byref(gs), C.byref(ps), _lib.ptr(x), x_rows, _lib.ptr(pred),
                                           _lib.ptr(hidden), _lib.ptr(ws), wsb, _stream()), "regt_forward_packed")
    else:
        _lib.check(lib.regt_forward(C.byref(dims), C.byref(gs), C.byref(ps), _lib.ptr(x), _lib.ptr(pred),
                                    _lib.ptr(hidden), _lib.ptr(ws), wsb, _stream()), "regt_forward")
    if forward_only:
        handle.release_now()
        return pred, hidden, None
    # (ps, gs: the parameter / graph pointer structs, unchanged until backward)
    return pred, hidden, _FwdState(graph=graph, dims=dims, handle=handle, wsb=wsb, saved=params, regional=regional, ps=ps, gs=gs,
                                   xp=x if packed else None, names=names, f_real=f_real, f_pad=f_pad)


def regt_run(x: torch.Tensor, graph: PreparedGraph, regional: bool, slope: float, packed, *params: torch.Tensor):
    """:class:`RegTGCNFunction` where a gradient may be asked for, the forward-only library call where none can
    (:func:`wants_forward_only`); same arguments and results as ``RegTGCNFunction.apply``."""
    if wants_forward_only(x, *params):
        pred, hidden, _ = _regt_forward_call(x, graph, regional, slope, packed, params, True)
        return pred, hidden
    return RegTGCNFunction.apply(x, graph, regional, slope, packed, *params)


class RegTGCNFunction(torch.autograd.Function):
    """(x, *params) -> (pred (N,O), hidden (N,C)); whole-model forward and backward in HIP."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, graph: PreparedGraph, regional: bool, slope: float, packed,
                *params: torch.Tensor):
        """``packed`` False: x is the reference's (N,F,T) snapshot.  True: x is the extended packed input
        (x_rows >= N, T, F) of the region-sharded path (own rows first, halo rows after; see dist.py).
        ``packed`` may also be a tuple ``(packed, arith, flags)``: the per-call GEMM arithmetic (``_lib.ARITH_*``) and
        ``_lib.DIMS_*`` switches of regt_dims (0, 0 = the process defaults)."""
        ctx.leaf_params = params                 # the caller's tensors (before any padding): whose .grad an accumulating backward updates
        ctx.set_materialize_grads(False)         # an output the loss does not use arrives as None in backward, not as a tensor of zeros
                                                 # (N x C floats filled and read back for nothing: `hidden` in every training loop)
        pred, hidden, ctx.st = _regt_forward_call(x, graph, regional, slope, packed, params, False)
        ctx.save_for_backward(hidden, *ctx.st.saved)
        return pred, hidden

    @staticmethod
    def backward(ctx, dpred, dhidden):
        lib = _lib.load()
        hidden, *params = ctx.saved_tensors
        st = ctx.st
        names, regional, dims = st.names, st.regional, st.dims
        dev = hidden.device
        dpred, dhid = _upstream_grads(dpred, dhidden, dims, dev)
        # one allocation for all gradients (16-byte aligned views), not one per parameter
        sizes = [(p_.numel() + 3) & ~3 for p_ in params]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        grads, off = {}, 0
        for n_, p_, sz in zip(names, params, sizes):
            grads[n_] = flat[off:off + p_.numel()].view_as(p_)
            off += sz
        gr = _fill(_lib.Grads(), grads, regional)
        _lib.check(lib.regt_backward(C.byref(dims), C.byref(st.gs), C.byref(st.ps), C.byref(gr), _lib.ptr(dpred), _lib.ptr(dhid),
                                     _lib.ptr(hidden), _lib.ptr(st.xp), _lib.ptr(st.handle.ws), st.wsb, _stream()), "regt_backward")
        # dL/dx only where x asked for it (nothing is launched or allocated otherwise); a form the library does not cover raises
        dx = _input_gradient(st, dev) if ctx.needs_input_grad[0] else None
        if st.f_pad:
            for n_ in F_WIDE_PARAMS:
                if n_ in grads:
                    grads[n_] = grads[n_][:, :st.f_real].contiguous()
        return (dx, None, None, None, None) + _deliver_grads(ctx.leaf_params, [grads[n_] for n_ in names])


def _input_gradient(st: _FwdState, dev) -> torch.Tensor:
    """regt_input_gradient behind :class:`RegTGCNFunction`: dL/dx (N, F, T) from what regt_backward just left in the workspace of ``st``
    (DESIGN.md 4e).  Padded feature columns are sliced off.  The bf16 arithmetic, overlapping regions and the packed (sharded) input are
    refused by the library: RegtError with its message."""
    from . import ops
    dims = st.dims
    dx = torch.empty(dims.N, dims.F, dims.T, dtype=torch.float32, device=dev)
    # (a packed input is refused on the workspace's record; its shard's operator has halo columns and no square transpose to build)
    t = None if st.xp is not None else st.graph.transposed_merged
    ops.input_gradient(dims, st.gs, st.ps, t, dx, st.handle.ws)
    return dx[:, :st.f_real] if st.f_pad else dx


def regt_period_gradients(x: torch.Tensor, graph: PreparedGraph, regional: bool, slope: float, arith: int, flags: int, leaf_params,
                          d_s: torch.Tensor) -> None:
    """Streamed training: the cell's backward from dL/dS alone.  ``x`` (rows, F, 1) holds one raw time step per graph
    copy, ``leaf_params`` the model's parameters in ``param_names`` order with a ONE-element attention tensor in first place,
    ``d_s`` (rows, C) the gradient of the cell outputs.  One training-layout T = 1 forward without the head (a recompute:
    DIMS_NO_HEAD) and regt_backward with ``dhidden = d_s``; the gradients of the cell and embedding parameters are added to their
    ``.grad`` (:func:`_deliver_grads` under :func:`grad_accumulation_in_backward`); the attention logit's and the head's are not formed."""
    lib = _lib.load()
    detached = [p.detach() for p in leaf_params]
    _, hidden, st = _regt_forward_call(x, graph, regional, slope, (False, arith, int(flags) | _lib.DIMS_NO_HEAD), detached, False)
    dims, names = st.dims, st.names
    if d_s.dtype != torch.float32 or d_s.device != hidden.device or tuple(d_s.shape) != tuple(hidden.shape) or not d_s.is_contiguous() \
            or d_s.data_ptr() % 16:
        raise ValueError(f"d_s must be a contiguous, 16-byte aligned float32 {tuple(hidden.shape)} tensor on {hidden.device}")
    head = set(PARAM_NAMES_HEAD)
    sizes = [0 if n_ in head else (p_.numel() + 3) & ~3 for n_, p_ in zip(names, st.saved)]
    flat = torch.empty(sum(sizes), dtype=torch.float32, device=hidden.device)
    grads, off = {}, 0
    for n_, p_, sz in zip(names, st.saved, sizes):
        if sz:
            grads[n_] = flat[off:off + p_.numel()].view_as(p_)
            off += sz
    gr = _fill(_lib.Grads(), grads, regional)
    _lib.check(lib.regt_backward(C.byref(dims), C.byref(st.gs), C.byref(st.ps), C.byref(gr), None, _lib.ptr(d_s), _lib.ptr(hidden), None,
                                 _lib.ptr(st.handle.ws), st.wsb, _stream()), "regt_backward")
    if st.f_pad:
        for n_ in F_WIDE_PARAMS:
            if n_ in grads:
                grads[n_] = grads[n_][:, :st.f_real].contiguous()
    # the one-element attention stand-in is no parameter of the model: its dummy gradient is dropped, like the head's absent ones
    live = [(p_, grads[n_]) for n_, p_ in zip(names, leaf_params) if n_ in grads and n_ != "tgnn._attention"]
    if not all(p_.is_leaf and p_.requires_grad for p_, _ in live):
        raise ValueError("period gradients are added to .grad: every cell / embedding parameter must be a leaf that requires grad")
    with grad_accumulation_in_backward():
        _deliver_grads([p_ for p_, _ in live], [g_ for _, g_ in live])


class MseLossFunction(torch.autograd.Function):
    """sum((pred - y)^2) / global_count and its gradient in one kernel (regt_mse_loss_grad; run.py:180 with the mean taken over the
    GLOBAL graph: a region shard passes the global element count)."""

    @staticmethod
    def forward(ctx, pred: torch.Tensor, y: torch.Tensor, global_count: int):
        lib = _lib.load()
        if not pred.is_cuda or pred.dtype != torch.float32 or y.dtype != torch.float32 or pred.shape != y.shape:
            raise ValueError("mse_loss: pred and y must be float32 CUDA tensors of one shape")
        pred, y = pred.contiguous(), y.contiguous()
        dpred = torch.empty_like(pred)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        _lib.check(lib.regt_mse_loss_grad(_lib.ptr(pred), _lib.ptr(y), _lib.ptr(dpred), _lib.ptr(loss), pred.numel(), int(global_count),
                                          _stream()), "regt_mse_loss_grad")
        ctx.save_for_backward(dpred)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None


def mse_loss(pred: torch.Tensor, y: torch.Tensor, global_count: Optional[int] = None) -> torch.Tensor:
    return MseLossFunction.apply(pred, y, pred.numel() if global_count is None else global_count)


class FusedTrainStep:
    """The per-snapshot body of run.py::train() (forward, ``mean((out - y)**2)``, backward with accumulating gradients,
    run.py:178-191) as three C-ABI calls -- regt_forward, regt_mse_loss_grad, regt_backward -- plus ONE axpy, without
    autograd.  Same kernels and arithmetic as :class:`RegTGCNFunction`; what goes away is the host work per step
    (autograd graph, 22 gradient allocations, 22 AccumulateGrad launches, the loss ops).  Measured at TPIMS size:
    0.60 -> 0.54 ms per step -- that regime is bound by the ~45 dependent small kernels themselves, not by the host.

    The parameters' ``.grad`` become views of one flat accumulator, so any torch optimizer works; clear them with
    :meth:`zero_grad` (or ``optimizer.zero_grad(set_to_none=False)``).  Build it after ``model.to(device)``."""

    def __init__(self, model, graph: PreparedGraph, num_features: int, periods: int, slope: float = 0.01,
                 loss_count: Optional[int] = None):
        """``loss_count``: the divisor of the squared-error sum (default: all N*O entries = the mean).  A batched graph of B
        snapshots (prepare_graph(copies=B)) passes the entries of ONE snapshot: the loss is then the SUM of the B snapshot means
        and the gradients are the sum run.py accumulates over those snapshots."""
        lib = _lib.load()
        self.loss_count = loss_count
        arith = _lib.arith_code(getattr(model, "arithmetic", None))
        self.lib, self.graph, self.regional = lib, graph, bool(model.regional)
        names = param_names(self.regional)
        named = dict(model.named_parameters())
        self.params = [named[n] for n in names]
        for n_, p_ in zip(names, self.params):
            if p_.dtype != torch.float32 or not p_.is_cuda or not p_.is_contiguous():
                raise ValueError(f"parameter {n_} must be a contiguous float32 CUDA tensor")
        dev = self.params[0].device
        tens = dict(zip(names, self.params))
        N, F, T = graph.num_nodes, num_features, periods
        Cdim = tens["tgnn.conv.bias"].numel()
        O, H1 = tens["linear2.weight"].shape[0], tens["linear1.weight"].shape[0]
        # (the model's per-call switches -- DIMS_NO_BF16_ROWS / _NO_FUSED_BWD / _NO_SIDE_STREAM -- apply here as under autograd)
        self.dims = _lib.Dims(N, T, F, Cdim, graph.num_regions, O, H1, 1 if self.regional else 0, float(slope), arith,
                              int(getattr(model, "call_flags", 0)))
        self.gs = _graph_struct(graph, T)
        self.wsb = _workspace_bytes("regt_workspace_bytes", C.byref(self.dims), self.gs.n_chunks, self.gs.overlap)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=dev)
        total = sum(p_.numel() for p_ in self.params)
        pad = [(-p_.numel()) % 4 for p_ in self.params]              # keep every view 16-byte aligned
        self.acc = torch.zeros(total + sum(pad), dtype=torch.float32, device=dev)
        self.step_grad = torch.empty_like(self.acc)
        views, off = {}, 0
        self._acc_views = []
        for n_, p_, extra in zip(names, self.params, pad):
            p_.grad = self.acc[off:off + p_.numel()].view_as(p_)
            self._acc_views.append(p_.grad)
            views[n_] = self.step_grad[off:off + p_.numel()].view_as(p_)
            off += p_.numel() + extra
        self.ps = _fill(_lib.Params(), tens, self.regional)
        self.gr = _fill(_lib.Grads(), views, self.regional)
        self._keep = (tens, views)
        self.pred = torch.empty(N, O, dtype=torch.float32, device=dev)
        self.hidden = torch.empty(N, Cdim, dtype=torch.float32, device=dev)
        self.dpred = torch.empty_like(self.pred)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.shape_x = (N, F, T)

    def __call__(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """One training step on snapshot (x (N,F,T), y (N,O)); returns the loss as a 1-element device tensor that the
        next call overwrites."""
        lib, st = self.lib, _stream()
        if tuple(x.shape) != self.shape_x or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
            raise ValueError(f"x must be a contiguous float32 CUDA tensor of shape {self.shape_x}")
        if tuple(y.shape) != tuple(self.pred.shape) or y.dtype != torch.float32 or not y.is_contiguous():
            raise ValueError(f"y must be a contiguous float32 tensor of shape {tuple(self.pred.shape)}")
        for p_, view in zip(self.params, self._acc_views):
            if p_.grad is not view:
                # optimizer.zero_grad() with its default set_to_none=True dropped the views: the optimiser would skip every
                # parameter while this object kept accumulating into a detached buffer.  Re-attach (cleared, as requested).
                if p_.grad is None:
                    view.zero_()
                else:
                    view.copy_(p_.grad)
                p_.grad = view
        _lib.check(lib.regt_forward(C.byref(self.dims), C.byref(self.gs), C.byref(self.ps), _lib.ptr(x), _lib.ptr(self.pred),
                                    _lib.ptr(self.hidden), _lib.ptr(self.ws), self.wsb, st), "regt_forward")
        cnt = self.pred.numel()
        _lib.check(lib.regt_mse_loss_grad(_lib.ptr(self.pred), _lib.ptr(y), _lib.ptr(self.dpred), _lib.ptr(self.loss), cnt,
                                          self.loss_count or cnt, st),
                   "regt_mse_loss_grad")
        _lib.check(lib.regt_backward(C.byref(self.dims), C.byref(self.gs), C.byref(self.ps), C.byref(self.gr), _lib.ptr(self.dpred),
                                     None, _lib.ptr(self.hidden), None, _lib.ptr(self.ws), self.wsb, st), "regt_backward")
        self.acc.add_(self.step_grad)
        return self.loss

    def zero_grad(self):
        self.acc.zero_()


# ---- models whose embedding stage is not the regional one: cell on a caller-supplied hidden input ---------------------

# the common list without the Chebyshev embedding ("tgnn.conv.*"), then the head
PARAM_NAMES_CELL = [n_ for n_ in PARAM_NAMES_COMMON if not n_.startswith("tgnn.conv.")] + PARAM_NAMES_HEAD


def _gcn_graph_struct(op) -> _lib.Graph:
    g = _lib.Graph()
    g.rowptr, g.col, g.val = op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr()
    return g


def _cell_forward_call(x, h_in, op, params, forward_only: bool):
    """regt_cell_forward behind :class:`CellFunction` and :func:`cell_run`: returns ``(pred, hidden, state)``; ``state`` is None for
    a forward-only call (its workspace block is back in the pool)."""
    lib = _lib.load()
    if not x.is_cuda:
        raise _lib.RegtError("RegT-GCN forward needs CUDA/HIP tensors: there is no CPU path in this package")
    names = PARAM_NAMES_CELL
    if len(params) != len(names):
        raise ValueError(f"expected {len(names)} parameter tensors, got {len(params)}")
    x, h_in = x.contiguous(), h_in.contiguous()
    N, F, T = x.shape
    tens = dict(zip(names, params))
    Cdim = tens["tgnn._base_tgcn.conv_z.bias"].numel()
    O, H1 = tens["linear2.weight"].shape[0], tens["linear1.weight"].shape[0]
    if tuple(h_in.shape) != (N * T, Cdim) or h_in.dtype != torch.float32:
        raise ValueError(f"h_in must be float32 ({N * T}, {Cdim}), got {h_in.dtype} {tuple(h_in.shape)}")
    if N != op.num_nodes:
        raise ValueError(f"x has {N} nodes but the prepared operator has {op.num_nodes}")
    dims = _lib.Dims(N, T, F, Cdim, 1, O, H1, 0, 0.0, 0, _lib.DIMS_FORWARD_ONLY if forward_only else 0)
    gs = _gcn_graph_struct(op)
    if forward_only:
        wsb = _workspace_bytes("regt_forward_only_workspace_bytes", C.byref(dims), C.byref(gs))
    else:
        wsb = _workspace_bytes("regt_workspace_bytes", C.byref(dims), 0, 0)
    handle = _WsHandle(wsb, x.device)
    pred = torch.empty(N, O, dtype=torch.float32, device=x.device)
    hidden = torch.empty(N, Cdim, dtype=torch.float32, device=x.device)
    ps = _fill(_lib.Params(), tens, False)
    _lib.check(lib.regt_cell_forward(C.byref(dims), C.byref(gs), C.byref(ps), _lib.ptr(x), _lib.ptr(h_in), _lib.ptr(pred),
                                     _lib.ptr(hidden), _lib.ptr(handle.ws), wsb, _stream()), "regt_cell_forward")
    if forward_only:
        handle.release_now()
        return pred, hidden, None
    return pred, hidden, _FwdState(graph=op, dims=dims, handle=handle, wsb=wsb, saved=(h_in, *params))


def cell_run(x, h_in, op, *params):
    """:class:`CellFunction` where a gradient may be asked for, the forward-only library call where none can
    (:func:`wants_forward_only`); same arguments and results as ``CellFunction.apply``."""
    if wants_forward_only(x, h_in, *params):
        return _cell_forward_call(x, h_in, op, params, True)[:2]
    return CellFunction.apply(x, h_in, op, *params)


class CellFunction(torch.autograd.Function):
    """(x (N,F,T), h_in (N*T, C), *cell params) -> (pred (N,O), hidden (N,C)): regt_cell_forward / regt_cell_backward."""

    @staticmethod
    def forward(ctx, x, h_in, op, *params):
        pred, hidden, ctx.st = _cell_forward_call(x, h_in, op, params, False)
        ctx.save_for_backward(hidden, *ctx.st.saved)
        ctx.set_materialize_grads(False)         # an unused output (hidden) arrives as None in backward, not as zeros
        return pred, hidden

    @staticmethod
    def backward(ctx, dpred, dhidden):
        lib = _lib.load()
        hidden, h_in, *params = ctx.saved_tensors
        names, st = PARAM_NAMES_CELL, ctx.st
        dims = st.dims
        tens = dict(zip(names, params))
        dpred, dhid = _upstream_grads(dpred, dhidden, dims, hidden.device)
        grads = {n_: torch.empty_like(p_) for n_, p_ in tens.items()}
        dh_in = torch.empty_like(h_in)
        gs = _gcn_graph_struct(st.graph)
        ps = _fill(_lib.Params(), tens, False)
        gr = _fill(_lib.Grads(), grads, False)
        _lib.check(lib.regt_cell_backward(C.byref(dims), C.byref(gs), C.byref(ps), C.byref(gr), _lib.ptr(dpred), _lib.ptr(dhid),
                                          _lib.ptr(hidden), _lib.ptr(h_in), _lib.ptr(dh_in), _lib.ptr(st.handle.ws), st.wsb,
                                          _stream()), "regt_cell_backward")
        return (None, dh_in, None) + tuple(grads[n_] for n_ in names)


# ---- one TGCN cell step: TGCN.forward(X, edge_index, edge_weight, H), differentiable in X and H -----------------------------------------

# conv_{z,r,h}.lin.weight, conv_{z,r,h}.bias, linear_{z,r,h}.weight, linear_{z,r,h}.bias under the prefix the structs are filled by
PARAM_NAMES_TGCN = [n_ for n_ in PARAM_NAMES_COMMON if n_.startswith("tgnn._base_tgcn.")]
F_WIDE_TGCN = tuple(n_ for n_ in PARAM_NAMES_TGCN if n_ in F_WIDE_PARAMS)


def _tgcn_forward_call(x, h_in, op, params, forward_only: bool):
    """regt_tgcn_forward behind :class:`TGCNStepFunction` and :func:`tgcn_run`: returns ``(h_out, state)``; ``state`` is None for a
    forward-only call (its workspace block is back in the pool)."""
    from . import ops
    if not x.is_cuda:
        raise _lib.RegtError("the TGCN cell needs CUDA/HIP tensors: there is no CPU path in this package")
    names = PARAM_NAMES_TGCN
    if len(params) != len(names):
        raise ValueError(f"expected {len(names)} parameter tensors, got {len(params)}")
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError(f"x must be float32 (N, F), got {x.dtype} {tuple(x.shape)}")
    for n_, p_ in zip(names, params):
        if p_.dtype != torch.float32 or not p_.is_cuda:
            raise ValueError(f"parameter {n_} must be a float32 CUDA tensor")
    N, f_real = x.shape
    if N != op.num_nodes:
        raise ValueError(f"x has {N} nodes but the prepared operator has {op.num_nodes}")
    # (16-byte feature rows: zero feature columns and zero weight columns, as _regt_forward_call pads them; a strided view -- the
    # reference passes X[:, :, period] -- is staged contiguous on the way)
    f_pad = (-f_real) % 4
    x = torch.nn.functional.pad(x, (0, f_pad)).contiguous() if f_pad else x.contiguous()
    params = tuple((torch.nn.functional.pad(p_, (0, f_pad)) if (f_pad and n_ in F_WIDE_TGCN) else p_).contiguous()
                   for n_, p_ in zip(names, params))
    tens = dict(zip(names, params))
    Cdim = tens["tgnn._base_tgcn.conv_z.bias"].numel()
    F = f_real + f_pad
    for k in GATES:
        for n_, shp in ((f"tgnn._base_tgcn.conv_{k}.lin.weight", (Cdim, F)), (f"tgnn._base_tgcn.linear_{k}.weight", (Cdim, 2 * Cdim))):
            if tuple(tens[n_].shape) != shp:
                raise ValueError(f"parameter {n_} has shape {tuple(tens[n_].shape)}, expected {shp}")
    if h_in is not None:
        if tuple(h_in.shape) != (N, Cdim) or h_in.dtype != torch.float32 or h_in.device != x.device:
            raise ValueError(f"H must be float32 ({N}, {Cdim}) on {x.device}, got {h_in.dtype} {tuple(h_in.shape)}")
        h_in = h_in.contiguous()
    dims = ops.tgcn_dims(N, F, Cdim, 0, _lib.DIMS_FORWARD_ONLY if forward_only else 0)
    gs = _gcn_graph_struct(op)
    wsb = _workspace_bytes("regt_tgcn_workspace_bytes", C.byref(dims))
    handle = _WsHandle(wsb, x.device)
    ps = _fill(_lib.Params(), tens, False)
    h_out = ops.tgcn_forward(dims, gs, ps, x, h_in, torch.empty(N, Cdim, dtype=torch.float32, device=x.device), handle.ws)
    if forward_only:
        handle.release_now()
        return h_out, None
    return h_out, _FwdState(graph=op, dims=dims, handle=handle, wsb=wsb, saved=(h_in, *params), ps=ps, gs=gs, names=names, f_real=f_real,
                            f_pad=f_pad)


def tgcn_run(x, h_in, op, *params):
    """:class:`TGCNStepFunction` where a gradient may be asked for, the forward-only library call where none can
    (:func:`wants_forward_only`); ``(x (N, F), h_in (N, C) | None, op: GcnOperator, *PARAM_NAMES_TGCN tensors) -> h_out (N, C)``."""
    if wants_forward_only(x, h_in, *params):
        return _tgcn_forward_call(x, h_in, op, params, True)[0]
    return TGCNStepFunction.apply(x, h_in, op, *params)


class TGCNStepFunction(torch.autograd.Function):
    """(x (N, F), h_in (N, C) | None, op, *12 cell params) -> h_out (N, C): regt_tgcn_forward / regt_tgcn_backward.  The backward
    returns dx only when x requires a gradient and dh_in only when h_in does (the library launches nothing for a gradient nobody asked
    for).  Honours :func:`set_grad_accumulation_in_backward`."""

    @staticmethod
    def forward(ctx, x, h_in, op, *params):
        ctx.leaf_params = params
        h_out, ctx.st = _tgcn_forward_call(x, h_in, op, params, False)
        ctx.has_h = h_in is not None
        ctx.save_for_backward(h_out, *(t_ for t_ in ctx.st.saved if t_ is not None))
        return h_out

    @staticmethod
    def backward(ctx, dh_out):
        from . import ops
        h_out, *rest = ctx.saved_tensors
        h_in = rest.pop(0) if ctx.has_h else None
        params, st = rest, ctx.st
        names, dims = st.names, st.dims
        dev = h_out.device
        sizes = [(p_.numel() + 3) & ~3 for p_ in params]             # one allocation, 16-byte aligned views
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        grads, off = {}, 0
        for n_, p_, sz in zip(names, params, sizes):
            grads[n_] = flat[off:off + p_.numel()].view_as(p_)
            off += sz
        gr = _fill(_lib.Grads(), grads, False)
        dx = torch.empty(dims.N, dims.F, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dh_in = torch.empty_like(h_out) if (ctx.has_h and ctx.needs_input_grad[1]) else None
        ops.tgcn_backward(dims, st.gs, st.ps, gr, dh_out.contiguous(), h_in, h_out, st.graph, dx, dh_in, st.handle.ws)
        if st.f_pad:
            for n_ in F_WIDE_TGCN:
                grads[n_] = grads[n_][:, :st.f_real].contiguous()
            if dx is not None:
                dx = dx[:, :st.f_real]
        return (dx, dh_in, None) + _deliver_grads(ctx.leaf_params, [grads[n_] for n_ in names])


class AggregateFunction(torch.autograd.Function):
    """Y = A_hat @ H for a learned H (N, W): forward pulls over the CSR of A_hat, backward over the CSR of A_hat^T."""

    @staticmethod
    def forward(ctx, h, op):
        from . import ops
        ctx.op = op
        return ops.spmm_csr(op.rowptr, op.col, op.val, h)

    @staticmethod
    def backward(ctx, dy):
        from . import ops
        op = ctx.op
        return ops.spmm_csr(op.t_rowptr, op.t_col, op.t_val, dy.contiguous()), None


class LinearFunction(torch.autograd.Function):
    """y = a @ w.T + b on the matrix cores; backward: da = dy @ w, (dw, db) = wgrad(dy, a)."""

    @staticmethod
    def forward(ctx, a, w, b):
        from . import ops
        ctx.save_for_backward(a, w)
        ctx.need_da = a.requires_grad
        ctx.has_bias = b is not None
        return ops.linear(a, w, b, 0)

    @staticmethod
    def backward(ctx, dy):
        from . import ops
        a, w = ctx.saved_tensors
        dy = dy.contiguous()
        da = ops.linear(dy, w.t().contiguous(), None, 0) if ctx.need_da else None
        dw, db = ops.wgrad(dy, a, with_bias=ctx.has_bias)
        return da, dw, db


class Cell0Function(torch.autograd.Function):
    """Zero-hidden TGCN cell + attention + head (regt_cell0_forward / regt_cell0_backward):
    (a_z (M,kz), a_h (M,kh), gz (C,kz), gh (C,kh), cz (C), ch (C), attention (T), linear1.weight, linear1.bias, linear2.weight,
    linear2.bias, num_nodes) -> (pred (N,O), hidden (N,C))."""

    @staticmethod
    def forward(ctx, a_z, a_h, gz, gh, cz, ch, att, l1w, l1b, l2w, l2b, num_nodes: int):
        lib = _lib.load()
        tens = [a_z, a_h, gz, gh, cz, ch, att, l1w, l1b, l2w, l2b]
        for t_ in tens:
            if not t_.is_cuda or t_.dtype != torch.float32:
                raise _lib.RegtError("zero-hidden cell needs float32 CUDA/HIP tensors: there is no CPU path in this package")
        a_z, a_h, gz, gh, cz, ch, att, l1w, l1b, l2w, l2b = [t_.contiguous() for t_ in tens]
        M, kz = a_z.shape
        kh = a_h.shape[1]
        T = att.numel()
        Cdim, O, H1 = gz.shape[0], l2w.shape[0], l1w.shape[0]
        if M != num_nodes * T or a_h.shape[0] != M or tuple(gz.shape) != (Cdim, kz) or tuple(gh.shape) != (Cdim, kh):
            raise ValueError("zero-hidden cell: inconsistent shapes")
        dims = _lib.Dims(num_nodes, T, max(kz, kh), Cdim, 1, O, H1, 0, 0.0)
        args = _lib.Cell0Args(a_z.data_ptr(), a_h.data_ptr(), kz, kh, gz.data_ptr(), gh.data_ptr(), cz.data_ptr(), ch.data_ptr(),
                              att.data_ptr(), l1w.data_ptr(), l1b.data_ptr(), l2w.data_ptr(), l2b.data_ptr())
        wsb = _workspace_bytes("regt_cell0_workspace_bytes", C.byref(dims), kz, kh)
        handle = _WsHandle(wsb, a_z.device)
        pred = torch.empty(num_nodes, O, dtype=torch.float32, device=a_z.device)
        hidden = torch.empty(num_nodes, Cdim, dtype=torch.float32, device=a_z.device)
        _lib.check(lib.regt_cell0_forward(C.byref(dims), C.byref(args), _lib.ptr(pred), _lib.ptr(hidden), _lib.ptr(handle.ws), wsb,
                                          _stream()), "regt_cell0_forward")
        ctx.dims, ctx.args, ctx.ws_handle, ctx.wsb = dims, args, handle, wsb
        ctx.save_for_backward(hidden, a_z, a_h, gz, gh, cz, ch, att, l1w, l1b, l2w, l2b)
        ctx.set_materialize_grads(False)         # an unused output (hidden) arrives as None in backward, not as zeros
        return pred, hidden

    @staticmethod
    def backward(ctx, dpred, dhidden):
        lib = _lib.load()
        hidden, a_z, a_h, gz, gh, cz, ch, att, l1w, l1b, l2w, l2b = ctx.saved_tensors
        dims = ctx.dims
        dpred, dhid = _upstream_grads(dpred, dhidden, dims, hidden.device)
        need_az, need_ah = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d_az = torch.empty_like(a_z) if need_az else None
        d_ah = torch.empty_like(a_h) if need_ah else None
        g = [torch.empty_like(t_) for t_ in (gz, gh, cz, ch, att, l1w, l1b, l2w, l2b)]
        gr = _lib.Cell0Grads(_lib.ptr(d_az), _lib.ptr(d_ah), *[t_.data_ptr() for t_ in g])
        _lib.check(lib.regt_cell0_backward(C.byref(dims), C.byref(ctx.args), C.byref(gr), _lib.ptr(dpred), _lib.ptr(dhid),
                                           _lib.ptr(hidden), _lib.ptr(ctx.ws_handle.ws), ctx.wsb, _stream()), "regt_cell0_backward")
        return (d_az, d_ah, *g, None)


class GatAggregateFunction(torch.autograd.Function):
    """out (N,T,F) = attention-weighted neighbour sum of GATConv on packed input rows (regt_gat_forward); the backward returns
    the gradients of the two score vectors u_src, u_dst (F) -- the input rows are data."""

    @staticmethod
    def forward(ctx, xp, u_src, u_dst, pattern, slope: float):
        from . import ops
        out, stats = ops.gat_forward(pattern.rowptr, pattern.col, xp, u_src, u_dst, slope)
        ctx.pattern, ctx.slope = pattern, slope
        ctx.save_for_backward(xp, u_src.contiguous(), stats)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import ops
        xp, u_src, stats = ctx.saved_tensors
        p = ctx.pattern
        n, t, f = xp.shape
        dsd = ops.gat_backward(p.rowptr, p.col, p.t_rowptr, p.t_col, xp, u_src, dout.contiguous(), stats, ctx.slope)
        du, _ = ops.wgrad(dsd, xp.view(n * t, f), with_bias=False)          # (2, F) = dsd^T x
        return None, du[0].contiguous(), du[1].contiguous(), None, None


class SpatialEmbedFunction(torch.autograd.Function):
    """(x_packed, lx_packed (N,T,F) data, W0, W1 (64,F), b (64), keep (N*T,2) int32 | None) -> S (N,64) = sum_t dropout(relu(ChebConv_t))
    (regt_spatial_embed_forward / regt_spatial_embed_backward: the backward recomputes the pre-activation; x is data, no dx)."""

    @staticmethod
    def forward(ctx, xp, lxp, w0, w1, b, keep):
        from . import ops
        ctx.save_for_backward(xp, lxp, w0, w1, b)
        ctx.keep = keep
        return ops.spatial_embed_forward(xp, lxp, w0, w1, b, keep)

    @staticmethod
    def backward(ctx, ds):
        from . import ops
        xp, lxp, w0, w1, b = ctx.saved_tensors
        dw0, dw1, db = ops.spatial_embed_backward(xp, lxp, w0, w1, b, ctx.keep, ds.contiguous())
        return None, None, dw0, dw1, db, None


class STNormFunction(torch.autograd.Function):
    """(x (B, L, N, C_in), dims, running, *params) -> out (B, O, N, L_out): the whole STNorm forward and backward in HIP
    (regt_stnorm_forward / regt_stnorm_backward; ``params`` in their table order, None where TNorm / SNorm is off).  The forward
    keeps the layer inputs and SNorm statistics in its workspace for the backward, which allocates its own scratch and recomputes
    the rest; in training mode the
    forward updates ``running`` in place.  x is data: no dx.  Honours :func:`set_grad_accumulation_in_backward`."""

    @staticmethod
    def forward(ctx, x, dims, running, *params):
        from . import ops
        out, ws = ops.stnorm_forward(dims, x, params, running)
        ctx.dims, ctx.running, ctx.ws = dims, running, ws
        ctx.leaf_params = params
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import ops
        (x,) = ctx.saved_tensors
        params = ctx.leaf_params
        grads = ops.stnorm_backward(ctx.dims, x, [None if p is None else p.detach() for p in params], ctx.running,
                                    dout.contiguous(), ctx.ws)
        ctx.ws = None
        # the last layer's residual conv feeds nothing: None, as autograd gives the reference module (no weight decay step either)
        last = ops.STNORM_HEAD + ops.STNORM_PER_LAYER * (ctx.dims.blocks * ctx.dims.layers - 1)
        grads[last + 4] = grads[last + 5] = None
        return (None, None, None) + _deliver_grads(params, grads)


class STIDFunction(torch.autograd.Function):
    """(x (B, L, N, C), dims, keep, *params) -> out (B, output_len, N, 1): the whole STID forward and backward in HIP
    (regt_stid_forward / regt_stid_backward; ``params`` in state_dict order, None for node_emb when if_node is off; ``keep`` the
    int32 keep bits or None).  When a gradient is wanted the forward leaves the block inputs and activations in a workspace that
    the backward reads.  x is data: no dx.  Honours :func:`set_grad_accumulation_in_backward`."""

    @staticmethod
    def forward(ctx, x, dims, keep, *params):
        from . import ops
        save = any(ctx.needs_input_grad[3:])
        out, ws = ops.stid_forward(dims, x, params, keep, save=save)
        ctx.dims, ctx.keep, ctx.ws = dims, keep, ws
        ctx.leaf_params = params
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import ops
        (x,) = ctx.saved_tensors
        params = ctx.leaf_params
        grads = ops.stid_backward(ctx.dims, x, [None if p is None else p.detach() for p in params], ctx.keep, dout.contiguous(), ctx.ws)
        ctx.ws = None
        return (None, None, None) + _deliver_grads(params, grads)


class GRUFunction(torch.autograd.Function):
    """(x (seq_len, rows, T), h0 (1, rows, 256) | None, want_out, want_last, weight_ih, weight_hh, bias_ih, bias_hh) ->
    (out (seq_len, rows, 256) | None, h_last (1, rows, 256) | None): one torch.nn.GRU layer in HIP (regt_gru_forward /
    regt_gru_backward).  When a gradient is wanted the forward leaves every step's state and gates in a workspace that the reverse
    pass reads.  x is data: no dx; h0 receives its gradient.  Honours :func:`set_grad_accumulation_in_backward`."""

    @staticmethod
    def forward(ctx, x, h0, want_out, want_last, *weights):
        from . import ops
        ctx.set_materialize_grads(False)
        save = any(ctx.needs_input_grad[4:]) or ctx.needs_input_grad[1]
        out, last, dims, ws = ops.gru_forward(x, [w.detach() for w in weights], h0, want_out, want_last, save=save)
        ctx.dims, ctx.ws, ctx.x = dims, ws if save else None, x
        ctx.leaf_params = weights
        ctx.want_dh0 = h0 is not None and ctx.needs_input_grad[1]
        return out, last

    @staticmethod
    def backward(ctx, dout, dlast):
        from . import ops
        weights = ctx.leaf_params
        grads, dh0 = ops.gru_backward(ctx.dims, ctx.x, [w.detach() for w in weights], dout, dlast, ctx.ws, ctx.want_dh0)
        ctx.ws = None
        return (None, dh0, None, None) + _deliver_grads(weights, grads)


class MLPHeadFunction(torch.autograd.Function):
    """(a (M, K), w1 (H1, K), b1, w2 (O, H1), b2) -> relu(a w1^T + b1) w2^T + b2 on the dense entry points (regt_linear, regt_wgrad,
    regt_relu_backward): StackedGRU's linear1 / relu / linear2.  Honours :func:`set_grad_accumulation_in_backward`."""

    @staticmethod
    def forward(ctx, a, w1, b1, w2, b2):
        from . import ops
        y1 = ops.linear(a, w1, b1, 2)
        ctx.save_for_backward(a, y1)
        ctx.leaf_params = (w1, b1, w2, b2)
        ctx.need_da = ctx.needs_input_grad[0]
        return ops.linear(y1, w2, b2, 0)

    @staticmethod
    def backward(ctx, dy):
        from . import ops
        a, y1 = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.leaf_params
        dy = dy.contiguous()
        dw2, db2 = ops.wgrad(dy, y1)
        d1 = ops.relu_backward_(y1, ops.linear(dy, w2.detach().t().contiguous(), None, 0))
        dw1, db1 = ops.wgrad(d1, a)
        da = ops.linear(d1, w1.detach().t().contiguous(), None, 0) if ctx.need_da else None
        return (da,) + _deliver_grads((w1, b1, w2, b2), (dw1, db1, dw2, db2))


class STAEAttentionFunction(torch.autograd.Function):
    """(q, k, v (M, 32 heads) views with one row stride, batch, in_steps, num_nodes, heads, axis) -> softmax(Q K^T / sqrt(32)) V per
    head along ``axis`` (regt_stae_attention_train / regt_stae_attention_backward).  When a gradient is wanted the forward keeps its
    output and each (row, head)'s log-sum-exp; otherwise it is the inference kernel and nothing is saved.  dq, dk, dv come back as
    the three column windows of one (M, 3 * 32 heads) buffer."""

    @staticmethod
    def forward(ctx, q, k, v, batch, in_steps, num_nodes, heads, axis):
        from . import ops
        ctx.shape = (batch, in_steps, num_nodes, heads, axis)
        if not any(ctx.needs_input_grad[:3]):
            return ops.stae_attention(q, k, v, batch, in_steps, num_nodes, heads, axis)
        out, lse = ops.stae_attention_train(q, k, v, batch, in_steps, num_nodes, heads, axis)
        ctx.save_for_backward(q, k, v, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import ops
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = ops.stae_attention_backward(q, k, v, out, dout.contiguous(), lse, *ctx.shape)
        need = ctx.needs_input_grad
        return (dq if need[0] else None, dk if need[1] else None, dv if need[2] else None, None, None, None, None, None)


class STAEPackedAttentionFunction(torch.autograd.Function):
    """:class:`STAEAttentionFunction` on one (M, 3 * 32 heads) buffer Q|K|V, as a fused projection writes it: the gradient is the
    backward's own (M, 3 * 32 heads) buffer, handed on whole (three separate window gradients would be re-assembled by autograd
    with three zero-filled copies of it)."""

    @staticmethod
    def forward(ctx, qkv, batch, in_steps, num_nodes, heads, axis):
        from . import ops
        d = heads * ops.STAE_HEAD_DIM
        q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        ctx.shape = (batch, in_steps, num_nodes, heads, axis)
        if not ctx.needs_input_grad[0]:
            return ops.stae_attention(q, k, v, batch, in_steps, num_nodes, heads, axis)
        out, lse = ops.stae_attention_train(q, k, v, batch, in_steps, num_nodes, heads, axis)
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import ops
        qkv, out, lse = ctx.saved_tensors
        d = out.shape[1]
        grads = torch.empty_like(qkv)
        ops.stae_attention_backward(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], out, dout.contiguous(), lse, *ctx.shape, grads=grads)
        return grads, None, None, None, None, None


class STAEAddLayerNormFunction(torch.autograd.Function):
    """(residual (M, D), y (M, D), gamma, beta, eps) -> LayerNorm(residual + y) gamma + beta (regt_stae_add_layernorm /
    regt_stae_add_layernorm_backward).  The backward recomputes the row statistics from residual and y, which is all the forward
    keeps; residual and y receive the same gradient.  Honours :func:`set_grad_accumulation_in_backward`."""

    @staticmethod
    def forward(ctx, residual, y, gamma, beta, eps):
        from . import ops
        out = ops.stae_add_layernorm(residual, y, gamma.detach(), beta.detach(), eps)
        if any(ctx.needs_input_grad[:4]):
            ctx.save_for_backward(residual, y)
            ctx.leaf_params = (gamma, beta)
            ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import ops
        residual, y = ctx.saved_tensors
        gamma, beta = ctx.leaf_params
        dz, dgamma, dbeta = ops.stae_add_layernorm_backward(residual, y, gamma.detach(), dout, ctx.eps)
        need = ctx.needs_input_grad
        return (dz if need[0] else None, dz if need[1] else None) + \
            _deliver_grads((gamma if need[2] else None, beta if need[3] else None), (dgamma, dbeta)) + (None,)


class ZeroGradAnchor(torch.autograd.Function):
    """Identity on ``(pred, hidden)`` that gives ``dead`` parameters an all-zero gradient: in the reference's GraphSAGE / GAT models
    the reset gate is computed and multiplied by the zero hidden state, so autograd hands its parameters zeros, not None --
    whichever of the two outputs the loss is built from."""

    @staticmethod
    def forward(ctx, pred, hidden, *dead):
        ctx.shapes = [(d.shape, d.device) for d in dead]
        ctx.set_materialize_grads(False)         # the unused output's gradient stays None on its way to the cell's backward
        return pred.view_as(pred), hidden.view_as(hidden)

    @staticmethod
    def backward(ctx, g_pred, g_hidden):
        return (g_pred, g_hidden, *[torch.zeros(s, dtype=torch.float32, device=dv) for s, dv in ctx.shapes])


def regt_gcn_forward(x, graph: PreparedGraph, params: Dict[str, torch.Tensor], regional: bool = True, slope: float = 0.01):
    """Functional entry: ``params`` keyed by the reference's state_dict names.  Like the modules it takes the forward-only call
    where no gradient can be asked for (:func:`regt_run`)."""
    names = param_names(regional)
    return regt_run(x, graph, regional, slope, False, *[params[n] for n in names])


# ---- STAEformer, the whole model (nn.STAEformerTrainable) ----------------------------------------------------------------------------

class STAEEmbedFunction(torch.autograd.Function):
    """(x (B, T, N, F), dims, node_emb, adaptive_embedding, input_proj.weight, .bias, tod_embedding.weight, dow_embedding.weight -- None
    where an embedding is off) -> layer 0's input (M, model_dim) (regt_stae_embed / regt_stae_embed_backward).  x gets no gradient
    (the reference's .long() indices and data have none to give).  Honours :func:`set_grad_accumulation_in_backward`."""

    @staticmethod
    def forward(ctx, x, dims, *params):
        from . import ops
        out = ops.stae_embed(dims, x, [None if p is None else p.detach() for p in params])
        if any(ctx.needs_input_grad[2:]):
            ctx.save_for_backward(x)
            ctx.dims, ctx.leaf_params = dims, params
        return out

    @staticmethod
    def backward(ctx, dx0):
        from . import ops
        need = ctx.needs_input_grad[2:]
        if not any(need):                        # only x asked (every parameter frozen): it has no gradient, nothing was kept
            return (None,) * (2 + len(need))
        x, = ctx.saved_tensors
        grads = ops.stae_embed_backward(ctx.dims, x, dx0)
        params = [p if n_ else None for p, n_ in zip(ctx.leaf_params, need)]
        return (None, None) + _deliver_grads(params, [g if n_ else None for g, n_ in zip(grads, need)])


class STAEOutputProjFunction(torch.autograd.Function):
    """(x (M, model_dim), dims, output_proj.weight, .bias) -> (B, out_steps, N, output_dim), the use_mixed_proj tail
    (regt_stae_output_proj / regt_stae_output_proj_backward).  The upstream gradient is read in place through its strides.  Honours
    :func:`set_grad_accumulation_in_backward`."""

    @staticmethod
    def forward(ctx, x, dims, w, b):
        from . import ops
        out = ops.stae_output_proj(dims, x, w.detach(), b.detach())
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x)
            ctx.dims, ctx.leaf_params = dims, (w, b)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import ops
        x, = ctx.saved_tensors
        w, b = ctx.leaf_params
        need = ctx.needs_input_grad
        dx, dw, db = ops.stae_output_proj_backward(ctx.dims, x, w.detach(), dout, need_dx=need[0])
        return (dx, None) + _deliver_grads((w if need[2] else None, b if need[3] else None), (dw, db))


class STAEDropAddLayerNormFunction(torch.autograd.Function):
    """(residual (M, D), y (M, D), keep int32 (M, D / 32) or None, p, gamma, beta, eps) -> LayerNorm(residual + keep y / (1 - p)) gamma +
    beta (regt_stae_drop_add_layernorm / _backward): the reference's ``ln(residual + dropout(out))``.  The backward recomputes the row
    statistics from residual, y and keep, which is all the forward keeps, and writes both gradients in one pass.  ``keep=None`` is
    :class:`STAEAddLayerNormFunction`'s arithmetic.  Honours :func:`set_grad_accumulation_in_backward`."""

    @staticmethod
    def forward(ctx, residual, y, keep, p, gamma, beta, eps):
        from . import ops
        out = ops.stae_drop_add_layernorm(residual, y, keep, p, gamma.detach(), beta.detach(), eps)
        need = ctx.needs_input_grad
        if need[0] or need[1] or need[4] or need[5]:
            ctx.save_for_backward(residual, y)
            ctx.keep, ctx.p, ctx.eps, ctx.leaf_params = keep, p, eps, (gamma, beta)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import ops
        residual, y = ctx.saved_tensors
        gamma, beta = ctx.leaf_params
        dz, dy, dgamma, dbeta = ops.stae_drop_add_layernorm_backward(residual, y, ctx.keep, ctx.p, gamma.detach(), dout, ctx.eps)
        need = ctx.needs_input_grad
        return (dz if need[0] else None, dy if need[1] else None, None, None) + \
            _deliver_grads((gamma if need[4] else None, beta if need[5] else None), (dgamma, dbeta)) + (None,)
