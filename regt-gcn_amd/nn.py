"""Drop-in ``nn.Module`` surface of the RegT-GCN hot path.

Same constructor / ``forward()`` signatures, parameter names and ``state_dict`` layout as the
reference classes, so the reference's ``run.py`` / ``predict.py`` and its shipped checkpoints work
unchanged:

* :class:`RegionalTemporalGCN`  <-> models/RegionalTemporalGCN.py:9-39  (+ RegionalA3TGCN :42-149)
* :class:`TemporalGCN`          <-> models/TemporalGCN.py:7-32          (+ A3TGCN :35-91)
* :class:`ConvStackedTemporalGCN` <-> models/ConvStackedTemporalGCN.py:8-33 (+ ConvStackedA3TGCN :35-126)
* :class:`TGCN`                 <-> models/utils.py:69-203 (the GRU cell: ``forward(X, edge_index, edge_weight, H)``, differentiable in X and H)
* :class:`A3TGCN`, :class:`RegionalA3TGCN` <-> the inner modules above, callable on their own (``model.tgnn(...)`` -> hidden)
* :class:`SpatialGCN`           <-> models/SpatialGCN.py:8-49
* :class:`STNorm`               <-> models/STNorm.py:6-185
* :class:`STID`                 <-> models/STID.py:5-157
* :class:`StackedGRU`           <-> models/StackedGRU.py:4-30
* :class:`STAEformer`           <-> models/STAEformer.py:110-255 (inference only)
* :class:`SelfAttentionLayer`   <-> models/STAEformer.py:76-107 (trainable)
* :class:`STAEformerTrainable`  <-> models/STAEformer.py:110-255 (trainable, keep-bit dropout)

The modules only *hold* parameters; all arithmetic runs in libregtgcn_hip.so through
:class:`regt-gcn_amd.functional.RegTGCNFunction`.  There is no CPU implementation here: calling
``forward`` with CPU tensors raises.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib
from . import ops
from .functional import (HEAD_HIDDEN, PARAM_NAMES_CELL, AggregateFunction, Cell0Function, CellFunction, GatAggregateFunction,
                         GRUFunction, LinearFunction, MLPHeadFunction, RegTGCNFunction, SpatialEmbedFunction, STAEAddLayerNormFunction,
                         STAEDropAddLayerNormFunction, STAEEmbedFunction, STAEOutputProjFunction, STAEPackedAttentionFunction, STIDFunction, STNormFunction, ZeroGradAnchor, _regt_forward_call, cell_run, param_names,
                         regt_period_gradients, regt_run, tgcn_run)
from .graph import (AttentionPattern, GcnOperator, MeanOperator, PreparedGraph, fingerprint, prepare_attention_pattern,
                    prepare_cheb_operator, prepare_gcn_operator, prepare_graph, prepare_mean_operator)

HIDDEN = 256          # out_channels=256, models/RegionalTemporalGCN.py:14 / models/TemporalGCN.py:12
LEAKY_SLOPE = 0.01    # F.leaky_relu default, models/RegionalTemporalGCN.py:143


class _PygLinear(nn.Module):
    """Linear parameter holder named like torch_geometric's Linear (``.weight`` (out,in) glorot; optional zero ``.bias``)."""

    def __init__(self, in_channels: int, out_channels: int, bias: bool = False):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        a = math.sqrt(6.0 / (in_channels + out_channels))
        nn.init.uniform_(self.weight, -a, a)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))


class _GCNConvParams(nn.Module):
    """Parameters of a PyG GCNConv: ``bias`` (C,) zero-init and ``lin.weight`` (C,F)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.lin = _PygLinear(in_channels, out_channels)


class _ChebConvParams(nn.Module):
    """Parameters of a PyG ChebConv(K=2): ``bias`` and ``lins.{0,1}.weight``."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.lins = nn.ModuleList([_PygLinear(in_channels, out_channels) for _ in range(2)])


class _SAGEConvParams(nn.Module):
    """Parameters of a PyG SAGEConv(aggr='mean', root_weight=True): ``lin_l.weight/.bias`` (neighbour mean) and ``lin_r.weight``."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.lin_l = _PygLinear(in_channels, out_channels, bias=True)
        self.lin_r = _PygLinear(in_channels, out_channels)


class _GATConvParams(nn.Module):
    """Parameters of a PyG GATConv(heads=1): ``att_src``, ``att_dst`` (1,1,C), ``bias`` (C), ``lin.weight`` (C,F) -- the layout
    of PyG >= 2.5, where an int ``in_channels`` shares one projection ``lin`` (2.0-2.4 call it lin_src / lin_dst)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        a = math.sqrt(6.0 / (1 + out_channels))
        self.att_src = nn.Parameter(torch.empty(1, 1, out_channels).uniform_(-a, a))
        self.att_dst = nn.Parameter(torch.empty(1, 1, out_channels).uniform_(-a, a))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.lin = _PygLinear(in_channels, out_channels)


class TGCN(nn.Module):
    """Parameter layout of the reference's T-GCN GRU cell (models/utils.py:75-161) for its three base blocks: 'gcn'
    (GCNConv, the hot path), 'graphsage' (SAGEConv) and 'gat' (GATConv) (:93-100)."""

    def __init__(self, in_channels: int, out_channels: int, baseblock: str = "gcn", improved: bool = False,
                 cached: bool = False, add_self_loops: bool = True):
        super().__init__()
        if improved or not add_self_loops:
            raise NotImplementedError("only improved=False, add_self_loops=True is on the hot path")
        blocks = {"gcn": _GCNConvParams, "graphsage": _SAGEConvParams, "gat": _GATConvParams}
        if baseblock not in blocks:
            raise NotImplementedError("Current baseblock %s is not supported." % (baseblock))     # models/utils.py:102
        conv = blocks[baseblock]
        self.in_channels, self.out_channels, self.baseblock = in_channels, out_channels, baseblock
        self.conv_z = conv(in_channels, out_channels)
        self.linear_z = nn.Linear(2 * out_channels, out_channels)
        self.conv_r = conv(in_channels, out_channels)
        self.linear_r = nn.Linear(2 * out_channels, out_channels)
        self.conv_h = conv(in_channels, out_channels)
        self.linear_h = nn.Linear(2 * out_channels, out_channels)
        self._graphs = _GraphCache()

    def _cell_params(self) -> List[torch.Tensor]:
        """The twelve tensors in functional.PARAM_NAMES_TGCN order."""
        convs, lins = (self.conv_z, self.conv_r, self.conv_h), (self.linear_z, self.linear_r, self.linear_h)
        return [c.lin.weight for c in convs] + [c.bias for c in convs] + [m.weight for m in lins] + [m.bias for m in lins]

    def _gcn_only(self):
        if self.baseblock != "gcn":
            raise NotImplementedError(f"TGCN.forward runs baseblock='gcn'; the '{self.baseblock}' block runs inside "
                                      "GraphSAGETemporalGCN / GATTemporal (zero hidden state, all periods at once)")

    def forward_prepared(self, X: torch.Tensor, op: GcnOperator, H: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One cell step on a prepared operator (:func:`prepare_gcn_operator`): H' (N, C).  Differentiable in the parameters, in ``X``
        and in ``H`` (regt_tgcn_forward / regt_tgcn_backward); ``X`` may be a strided view such as ``X[:, :, period]``."""
        self._gcn_only()
        _need_cuda(X)
        return tgcn_run(X, H, op, *self._cell_params())

    def forward(self, X: torch.Tensor, edge_index: torch.Tensor, edge_weight: Optional[torch.Tensor] = None,
                H: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The reference's ``TGCN.forward(X, edge_index, edge_weight, H)`` (models/utils.py:190-203): X (N, F), H (N, C) or None = zeros."""
        self._gcn_only()
        _need_cuda(X)
        n = X.shape[0]
        op = self._graphs.get([edge_index, edge_weight], n, lambda: prepare_gcn_operator(edge_index, edge_weight, n))
        return self.forward_prepared(X, op, H)


class _GraphCache:
    """Prepared graphs keyed first by tensor identity (free), then by content fingerprint (one 8-byte readback).

    An identity entry keeps strong references to its key tensors: while the entry lives their storage cannot be freed and
    handed to a new tensor with other edges at the same address, so (data_ptr, shape, _version) really identifies the
    content (an in-place edit bumps ``_version``).  The identity table is small (a loader that builds a fresh ``edge_index``
    per snapshot, run.py:172, goes through the fingerprint every time) so that it pins at most a few edge lists."""

    MAX_IDENT = 8

    def __init__(self):
        self._by_id: Dict[tuple, tuple] = {}            # key -> (graph, key tensors)
        self._by_hash: Dict[tuple, PreparedGraph] = {}

    @staticmethod
    def _ident(tensors):
        return tuple((t.data_ptr(), tuple(t.shape), t._version) if t is not None else None for t in tensors)

    def get(self, tensors: Sequence[Optional[torch.Tensor]], num_nodes: int, build):
        key = (num_nodes,) + self._ident(tensors)
        hit = self._by_id.get(key)
        if hit is not None and all(a is b for a, b in zip(hit[1], tensors)):
            return hit[0]
        hkey = (num_nodes, fingerprint(tensors))
        g = self._by_hash.get(hkey)
        if g is None:
            g = build()
            self._by_hash[hkey] = g
        if len(self._by_id) >= self.MAX_IDENT:
            self._by_id.clear()
        self._by_id[key] = (g, tuple(tensors))
        return g


def _need_cuda(x: torch.Tensor):
    if not x.is_cuda:
        raise _lib.RegtError("this package only runs on an MI355X through libregtgcn_hip.so; got a CPU tensor "
                             "(use oracle/ for CPU checks)")


def _inner_hidden(mod: nn.Module, regional: bool, x: torch.Tensor, graph: PreparedGraph) -> torch.Tensor:
    """``hidden`` (N, C) of an inner module (A3TGCN / RegionalA3TGCN) called on its own: the whole-model entry points without the head
    (DIMS_NO_HEAD) -- the bits the owning model returns as ``hidden``.  The head tensors the parameter structs name are stand-ins that
    the library neither reads nor writes under that flag."""
    _need_cuda(x)
    named = dict(mod.named_parameters())
    names = param_names(regional)
    dev = named["_attention"].device
    head = mod.__dict__.get("_no_head_tensors")
    if head is None or head[0].device != dev:
        c = mod.out_channels
        head = mod.__dict__["_no_head_tensors"] = [torch.zeros(s, dtype=torch.float32, device=dev) for s in ((4, c), (4,), (1, 4), (1,))]
    params = [named[n_[len("tgnn."):]] for n_ in names[:-4]] + head
    return regt_run(x, graph, regional, LEAKY_SLOPE, (False, _lib.arith_code(getattr(mod, "arithmetic", None)), _lib.DIMS_NO_HEAD), *params)[1]


class RegionalA3TGCN(nn.Module):
    """models/RegionalTemporalGCN.py:42-149 (attention over periods + regional ChebConv + TGCN): the parameter layout, and ``forward``
    with the reference's argument list, returning the attention-weighted hidden state (N, C)."""

    def __init__(self, in_channels: int, out_channels: int, num_nodes: int, periods: int, improved: bool = False,
                 cached: bool = False, add_self_loops: bool = True, num_regions: int = 5):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.num_nodes, self.periods, self.num_regions = num_nodes, periods, num_regions
        self._attention = nn.Parameter(torch.empty(periods))
        # registered-but-unused parameters of the reference's dead attention() (:84-87, :91-111)
        self._weight_att1 = nn.Parameter(torch.normal(0.0, 0.1, size=(out_channels, 1)))
        self._weight_att2 = nn.Parameter(torch.normal(0.0, 0.1, size=(num_nodes, 1)))
        self._bias_att1 = nn.Parameter(torch.normal(0.0, 1.0, size=(1, 1)))
        self._bias_att2 = nn.Parameter(torch.normal(0.0, 1.0, size=(1, 1)))
        self._base_tgcn = TGCN(in_channels, out_channels, improved=improved, cached=cached, add_self_loops=add_self_loops)
        self.conv = _ChebConvParams(in_channels, out_channels)
        self.linear = nn.Linear(out_channels * num_regions, out_channels)
        nn.init.uniform_(self._attention)
        self._graphs = _GraphCache()

    def forward(self, X: torch.Tensor, edge_index: torch.Tensor, *regions, edge_weight: Optional[torch.Tensor] = None,
                H: Optional[torch.Tensor] = None, C: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``forward(X, edge_index, idx_1..idx_R, weight_1..weight_R, edge_weight=None, H=None, C=None)`` -> hidden (N, C)
        (models/RegionalTemporalGCN.py:114-149; ``edge_weight``, ``H``, ``C`` may also follow positionally).  ``H`` and ``C`` are
        accepted and ignored, as the reference ignores them: every period's cell starts from the regional embedding."""
        r = self.num_regions
        extra = list(regions[2 * r:])
        if len(regions) < 2 * r or len(extra) > 3:
            raise TypeError(f"forward() expects {r} regional edge_index tensors followed by {r} edge weight tensors "
                            f"(then optionally edge_weight, H, C), got {len(regions)} tensors")
        if extra:
            edge_weight = extra[0]
        idx, attr = list(regions[:r]), list(regions[r:2 * r])
        _need_cuda(X)
        n = X.shape[0]
        flat: List[Optional[torch.Tensor]] = [edge_index, edge_weight]
        for i, a in zip(idx, attr):
            flat += [i, a]
        graph = self._graphs.get(flat, n, lambda: prepare_graph(edge_index, edge_weight, idx, attr, n))
        return _inner_hidden(self, True, X, graph)


class A3TGCN(nn.Module):
    """Parameter layout of models/TemporalGCN.py:35-73 (incl. its dead ``linear`` (64 -> C), :70)."""

    def __init__(self, in_channels: int, out_channels: int, periods: int, improved: bool = False, cached: bool = False,
                 add_self_loops: bool = True):
        super().__init__()
        self.in_channels, self.out_channels, self.periods = in_channels, out_channels, periods
        self._base_tgcn = TGCN(in_channels, out_channels)
        self.conv = _ChebConvParams(in_channels, out_channels)
        self.linear = nn.Linear(64, out_channels)
        self._attention = nn.Parameter(torch.empty(periods))
        nn.init.uniform_(self._attention)
        self._graphs = _GraphCache()

    def forward(self, X: torch.Tensor, edge_index: torch.Tensor, edge_weight: Optional[torch.Tensor] = None,
                H: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``forward(X (N, F, T), edge_index, edge_weight, H)`` -> hidden (N, C) (models/TemporalGCN.py:75-91).  ``H`` is accepted and
        ignored, as the reference ignores it: every period's cell starts from the Chebyshev embedding."""
        _need_cuda(X)
        n = X.shape[0]
        graph = self._graphs.get([edge_index, edge_weight], n,
                                 lambda: prepare_graph(edge_index, edge_weight, [edge_index], [edge_weight], n))
        return _inner_hidden(self, False, X, graph)


class _FusedModel(nn.Module):
    regional: bool

    def _params_in_order(self) -> List[torch.Tensor]:
        # walking named_parameters() costs ~70 us per call -- a fifth of a TPIMS-scale step's host time; the Parameter
        # objects are stable (load_state_dict / .to() / optimisers update them in place), so look them up once
        cached = self.__dict__.get("_ordered_params")
        if cached is None or any(p is not q for p, q in zip(cached[0], cached[1]())):
            named = dict(self.named_parameters())
            plist = [named[n] for n in param_names(self.regional)]
            owners = [self._owner_of(n) for n in param_names(self.regional)]
            getter = lambda: [m._parameters[k] for m, k in owners]      # noqa: E731  (catches a replaced Parameter object)
            cached = (plist, getter)
            self.__dict__["_ordered_params"] = cached
        return cached[0]

    def _owner_of(self, name: str):
        mod = self
        *path, leaf = name.split(".")
        for part in path:
            mod = mod._modules[part]
        return mod, leaf

    # GEMM arithmetic of THIS model's calls (regt_dims.arith): None = the process default (regt_set_gemm_mode / REGT_GEMM_MODE),
    # "fp32", "bf16x3" (exact split) or "bf16" (reduced precision, BASELINE configs[4]).  Per call, no process state: two models
    # of one process may differ.
    arithmetic = None
    call_flags = 0        # regt_dims.flags of this model's calls: _lib.DIMS_NO_BF16_ROWS | DIMS_NO_FUSED_BWD | DIMS_NO_SIDE_STREAM (A/B switches)

    def _run(self, x: torch.Tensor, graph: PreparedGraph, packed: bool = False):
        arith, flags = _lib.arith_code(self.arithmetic), int(self.call_flags)
        # (regt_run: RegTGCNFunction.apply, or the forward-only library call when no gradient can be asked for -- decided here,
        # before apply: inside Function.forward grad mode is always off)
        return regt_run(x, graph, self.regional, LEAKY_SLOPE, (packed, arith, flags) if (arith or flags) else packed,
                        *self._params_in_order())

    @torch.no_grad()
    def period_outputs(self, x_steps: torch.Tensor, graph: PreparedGraph, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The cell's output S (B, N, C) of B raw time steps ``x_steps`` (B, N, F); ``graph`` prepared with ``copies=B`` (a plain prepared
        graph for B = 1).  The reference calls the cell with H = None in every period, so S of a time step does not depend on the window
        it is read through: ``hidden(window i) = sum_p softmax(_attention)_p S_{i+p}`` (serve.StreamingPredictor, ops.window_forward).
        One forward-only library call at T = 1 on (B N, F, 1) with a one-element attention tensor in place of ``_attention``: a single
        logit has probability exactly 1, so that call's ``hidden`` IS the cell output (its ``pred`` is dropped).  Never differentiable.
        ``out``: a contiguous float32 (B, N, C) tensor the library writes S into (a ring slab, a stretch of a timeline) and that is
        returned, instead of a fresh one.
        fp32-storage arithmetics only ("fp32", "bf16x3")."""
        _need_cuda(x_steps)
        if x_steps.dim() != 3 or x_steps.dtype != torch.float32:
            raise ValueError(f"x_steps must be float32 (B, N, F), got {x_steps.dtype} {tuple(x_steps.shape)}")
        arith = _lib.arith_code(self.arithmetic)
        if arith == _lib.ARITH_BF16 or (arith == _lib.ARITH_DEFAULT and _lib.gemm_mode() == 2):
            raise NotImplementedError("period_outputs / streaming inference covers the fp32-storage arithmetics (fp32, bf16x3); the bf16 "
                                      "arithmetic rounds per window and is out of scope (DESIGN.md 4b)")
        b, n, f = x_steps.shape
        if b * n != graph.num_nodes:
            raise ValueError(f"x_steps holds {b} steps of {n} nodes but the prepared graph has {graph.num_nodes} nodes (prepare it with copies={b})")
        params = [p.detach() for p in self._params_in_order()]
        params[0] = self._one_logit()                          # tgnn._attention -> one logit: softmax = [1.0]
        flags = int(self.call_flags) | _lib.DIMS_NO_HEAD       # the head's pred of a single step would be dropped: not computed
        if out is not None and (out.dim() != 3 or tuple(out.shape[:2]) != (b, n) or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous ({b}, {n}, C) tensor, got {tuple(out.shape)} strides {out.stride()}")
        _, s, _ = _regt_forward_call(x_steps.reshape(b * n, f, 1), graph, self.regional, LEAKY_SLOPE, (False, arith, flags), params, True,
                                     hidden_out=None if out is None else out.view(b * n, out.shape[2]))
        return s.view(b, n, -1) if out is None else out

    def _one_logit(self) -> torch.Tensor:
        """A one-element zero tensor on the model's device, kept: the library's call plans are keyed by the parameters' addresses."""
        dev = self._params_in_order()[0].device
        t = self.__dict__.get("_one_logit_tensor")
        if t is None or t.device != dev:
            t = self.__dict__["_one_logit_tensor"] = torch.zeros(1, dtype=torch.float32, device=dev)
        return t

    def _refuse_bf16(self, what: str) -> int:
        arith = _lib.arith_code(self.arithmetic)
        if arith == _lib.ARITH_BF16 or (arith == _lib.ARITH_DEFAULT and _lib.gemm_mode() == 2):
            raise NotImplementedError(f"{what} covers the fp32-storage arithmetics (fp32, bf16x3); the bf16 arithmetic rounds per window "
                                      "and is out of scope (DESIGN.md 4b, 4c)")
        return arith

    def period_gradients(self, x_steps: torch.Tensor, graph: PreparedGraph, d_s: torch.Tensor) -> None:
        """Streamed training: adds to ``.grad`` of the cell and embedding parameters what the cell outputs S (B, N, C) of
        the B raw time steps ``x_steps`` (B, N, F) pass back from ``d_s`` = dL/dS (B, N, C, contiguous); ``graph`` prepared with
        ``copies=B``.  One training-layout T = 1 forward without the head (the recompute of :meth:`period_outputs`' S) followed by the
        library's backward with ``d_s`` as the whole upstream gradient, on a one-element attention tensor whose dummy gradient is dropped.
        ``tgnn._attention``, ``linear1.*`` and ``linear2.*`` are left alone: their gradients come from ``ops.window_backward``.
        fp32-storage arithmetics only."""
        _need_cuda(x_steps)
        if x_steps.dim() != 3 or x_steps.dtype != torch.float32:
            raise ValueError(f"x_steps must be float32 (B, N, F), got {x_steps.dtype} {tuple(x_steps.shape)}")
        arith = self._refuse_bf16("period_gradients / streamed training")
        b, n, f = x_steps.shape
        if b * n != graph.num_nodes:
            raise ValueError(f"x_steps holds {b} steps of {n} nodes but the prepared graph has {graph.num_nodes} nodes (prepare it with copies={b})")
        if d_s.dim() != 3 or tuple(d_s.shape[:2]) != (b, n) or not d_s.is_contiguous():
            raise ValueError(f"d_s must be a contiguous ({b}, {n}, C) tensor, got {tuple(d_s.shape)} strides {d_s.stride()}")
        params = list(self._params_in_order())
        params[0] = self._one_logit()
        regt_period_gradients(x_steps.reshape(b * n, f, 1), graph, self.regional, LEAKY_SLOPE, arith, int(self.call_flags), params,
                              d_s.view(b * n, d_s.shape[2]))

    def forward_packed(self, x_packed_ext: torch.Tensor, graph: PreparedGraph):
        """Region-sharded entry: ``x_packed_ext`` (x_rows, T, F) = own packed rows + gathered halo rows (dist.py)."""
        _need_cuda(x_packed_ext)
        return self._run(x_packed_ext, graph, packed=True)


class RegionalTemporalGCN(_FusedModel):
    """RegT-GCN.  ``forward`` keeps the reference's 12-positional-argument form (5 named regions,
    models/RegionalTemporalGCN.py:25-26) and also accepts any number R of regions as
    ``forward(x, edge_index, idx_1..idx_R, attr_1..attr_R)`` or ``forward(x, edge_index, [idx...], [attr...])``.
    Returns ``(prediction (N, output_dim), hidden (N, 256))``."""

    regional = True

    def __init__(self, node_features: int, num_nodes: int, periods: int, output_dim: int, num_regions: int = 5,
                 hidden_channels: int = HIDDEN):
        super().__init__()
        self.tgnn = RegionalA3TGCN(in_channels=node_features, out_channels=hidden_channels, num_nodes=num_nodes,
                                   periods=periods, num_regions=num_regions)
        self.output_dim = output_dim
        self.linear1 = nn.Linear(hidden_channels, HEAD_HIDDEN)
        self.linear2 = nn.Linear(HEAD_HIDDEN, output_dim)
        self.relu = nn.ReLU()
        self.num_nodes, self.num_regions = num_nodes, num_regions
        self._graphs = _GraphCache()

    def prepare_graph(self, edge_index, region_index: Sequence[torch.Tensor], region_attr: Sequence[torch.Tensor],
                      num_nodes: Optional[int] = None, copies: int = 1) -> PreparedGraph:
        """Normalise + sort the static graph once; pass the result to :meth:`forward_prepared`.  ``copies`` = B builds the
        block-diagonal graph of B snapshots (train.train_epoch_batched): forward_prepared then takes x of shape (B*N, F, T)."""
        n = self.num_nodes if num_nodes is None else num_nodes
        return prepare_graph(edge_index, None, list(region_index), list(region_attr), n, copies)

    def forward_prepared(self, x: torch.Tensor, graph: PreparedGraph):
        _need_cuda(x)
        return self._run(x, graph)

    # the reference's parameter names, in its order (models/RegionalTemporalGCN.py:25-26): accepted as keywords too
    REF_KEYWORDS = ("IAedge_index", "KSedge_index", "KYedge_index", "OHedge_index", "WIedge_index",
                    "IAedge_attr", "KSedge_attr", "KYedge_attr", "OHedge_attr", "WIedge_attr")

    def forward(self, x, edge_index, *regions, **named):
        if named:
            # keyword call with the reference's names (any prefix of the ten may still be positional, as in Python's own binding)
            unknown = [k for k in named if k not in self.REF_KEYWORDS]
            if unknown:
                raise TypeError(f"forward() got an unexpected keyword argument '{unknown[0]}'")
            if self.num_regions != 5:
                raise TypeError("the reference's keyword names cover its 5 regions; this model was built for "
                                f"{self.num_regions} -- pass the region tensors positionally or as two lists")
            if len(regions) > len(self.REF_KEYWORDS) or (len(regions) == 2 and isinstance(regions[0], (list, tuple))):
                raise TypeError("forward(): keyword region arguments cannot be mixed with the list form")
            bound = list(regions)
            for k in self.REF_KEYWORDS[len(regions):]:
                if k not in named:
                    raise TypeError(f"forward() missing 1 required positional argument: '{k}'")
                bound.append(named[k])
            for k in self.REF_KEYWORDS[:len(regions)]:
                if k in named:
                    raise TypeError(f"forward() got multiple values for argument '{k}'")
            regions = tuple(bound)
        _need_cuda(x)
        if len(regions) == 2 and isinstance(regions[0], (list, tuple)):
            idx, attr = list(regions[0]), list(regions[1])
        else:
            if len(regions) != 2 * self.num_regions:
                raise TypeError(f"forward() expects {self.num_regions} regional edge_index tensors followed by "
                                f"{self.num_regions} edge_attr tensors, got {len(regions)} tensors")
            idx, attr = list(regions[:self.num_regions]), list(regions[self.num_regions:])
        if len(idx) != self.num_regions:
            raise TypeError(f"model was built for {self.num_regions} regions, got {len(idx)}")
        n = x.shape[0]
        flat: List[Optional[torch.Tensor]] = [edge_index, None]
        for i, a in zip(idx, attr):
            flat += [i, a]
        graph = self._graphs.get(flat, n, lambda: prepare_graph(edge_index, None, idx, attr, n))
        return self._run(x, graph)


class TemporalGCN(_FusedModel):
    """A3T-GCN baseline sharing the cell.  ``forward(x, edge_index, edge_attr)`` (models/TemporalGCN.py:21)."""

    regional = False

    def __init__(self, node_features: int, periods: int, output_dim: int, hidden_channels: int = HIDDEN):
        super().__init__()
        self.tgnn = A3TGCN(in_channels=node_features, out_channels=hidden_channels, periods=periods)
        self.output_dim = output_dim
        self.linear1 = nn.Linear(hidden_channels, HEAD_HIDDEN)
        self.linear2 = nn.Linear(HEAD_HIDDEN, output_dim)
        self.relu = nn.ReLU()
        self._graphs = _GraphCache()

    def prepare_graph(self, edge_index, edge_attr, num_nodes: int, copies: int = 1) -> PreparedGraph:
        return prepare_graph(edge_index, edge_attr, [edge_index], [edge_attr], num_nodes, copies)

    def forward_prepared(self, x: torch.Tensor, graph: PreparedGraph):
        _need_cuda(x)
        return self._run(x, graph)

    def forward(self, x, edge_index, edge_attr):
        _need_cuda(x)
        n = x.shape[0]
        graph = self._graphs.get([edge_index, edge_attr], n, lambda: prepare_graph(edge_index, edge_attr, [edge_index], [edge_attr], n))
        return self._run(x, graph)


class ConvStackedA3TGCN(nn.Module):
    """Parameter layout of models/ConvStackedTemporalGCN.py:35-103: TGCN cell, five GCNConv, a never-called
    ``linear`` (512*5 -> 512, :100) and the attention over periods."""

    def __init__(self, in_channels: int, out_channels: int, periods: int, improved: bool = False, cached: bool = False,
                 add_self_loops: bool = True):
        super().__init__()
        if improved or not add_self_loops:
            raise NotImplementedError("only improved=False, add_self_loops=True is on the hot path")
        self.in_channels, self.out_channels, self.periods = in_channels, out_channels, periods
        self._base_tgcn = TGCN(in_channels=in_channels, out_channels=out_channels)
        self.conv1 = _GCNConvParams(in_channels, out_channels)
        self.conv2 = _GCNConvParams(out_channels, out_channels)
        self.conv3 = _GCNConvParams(out_channels, out_channels)
        self.conv4 = _GCNConvParams(out_channels, out_channels)
        self.conv5 = _GCNConvParams(out_channels, out_channels)
        self.linear = nn.Linear(out_channels * 5, out_channels)      # dead layer of the reference, kept for state_dict parity
        self._attention = nn.Parameter(torch.empty(periods))
        nn.init.uniform_(self._attention)


class ConvStackedTemporalGCN(nn.Module):
    """Stacked-GCNConv baseline.  ``forward(x, edge_index, edge_attr)`` ->
    ``(prediction (N, output_dim), hidden (N, 512))`` (models/ConvStackedTemporalGCN.py:21-33).

    Per period the reference runs conv1..conv5 = A_hat (h W^T) + b without activation and feeds the result to the TGCN
    cell as its hidden input.  Here all periods go through each layer at once on node-major rows (node*T + t):
    layer 1 aggregates the *input* (width T*F, no sparse backward), layers 2-5 aggregate the learned hidden state at
    width T*512 with the CSR of A_hat forward and of A_hat^T backward; the dense parts are fp32-MFMA GEMMs and the
    cell + attention + head is ``regt_cell_forward`` / ``regt_cell_backward``."""

    HIDDEN = 512          # models/ConvStackedTemporalGCN.py:13
    HEAD = 256            # :16

    def __init__(self, node_features: int, periods: int, output_dim: int):
        super().__init__()
        self.tgnn = ConvStackedA3TGCN(in_channels=node_features, out_channels=self.HIDDEN, periods=periods)
        self.linear1 = nn.Linear(self.HIDDEN, self.HEAD)
        self.linear2 = nn.Linear(self.HEAD, output_dim)
        self.relu = nn.ReLU()
        self.output_dim = output_dim
        self._graphs = _GraphCache()

    def prepare_graph(self, edge_index, edge_attr, num_nodes: int, copies: int = 1) -> GcnOperator:
        return prepare_gcn_operator(edge_index, edge_attr, num_nodes, copies)

    # conv1 .. conv5 are applied WITHOUT an activation in between (models/ConvStackedTemporalGCN.py:116-120), and the aggregation
    # (acts on the node axis) commutes with the linear maps (act on the feature axis), so the five layers collapse exactly:
    #     h5 = (A^5 x) (W5 W4 W3 W2 W1)^T + sum_k (A^(5-k) 1) (W5 .. W_(k+1) b_k)^T,        A = A_hat
    # -- five aggregations of the INPUT at width T*F (no sparse backward: x is data) and of the all-ones vector (once per graph),
    # ONE (M x 512) GEMM with K = F + 8 on the rows [A^5 x | A^0 1 .. A^4 1], and a chain of 512 x 512 weight products that
    # autograd differentiates (LinearFunction: regt_linear / regt_wgrad).  The reference-faithful layer-by-layer form -- four
    # aggregations of the learned hidden state at width T*512 forward (A_hat) and backward (A_hat^T), 27 GB of gathered rows
    # each at the cfg-3 shape -- stays available as ``collapse = False`` / :meth:`forward_layerwise` (and is what pins the wide
    # aggregation kernels in tests/test_gpu_convstack.py); same parameters, same gradients up to fp32 reassociation.
    collapse = True

    def forward_prepared(self, x: torch.Tensor, op: GcnOperator):
        _need_cuda(x)
        if not self.collapse:
            return self.forward_layerwise(x, op)
        n, f, t = x.shape
        sd = dict(self.named_parameters())
        u = ops.pack_x(x).view(n, t * f)                                        # (N, T*F)
        for _ in range(5):
            u = ops.spmm_csr(op.rowptr, op.col, op.val, u)                      # A^5 x: input data, no backward
        chain = op.__dict__.get("_ones_chain")
        if chain is None:                                                       # [A^0 1 .. A^4 1 | 0 0 0] per node, once per graph
            cols, a = [], torch.ones(n, 4, device=x.device)
            for _ in range(5):
                cols.append(a[:, :1])
                a = ops.spmm_csr(op.rowptr, op.col, op.val, a)
            chain = torch.cat(cols + [torch.zeros(n, 3, device=x.device)], dim=1).contiguous()
            op.__dict__["_ones_chain"] = chain
        feat = torch.cat([u.view(n, t, f), chain[:, None, :].expand(n, t, 8)], dim=2).reshape(n * t, f + 8)
        # P_k = W5 .. W_(k+1),  c_k = P_k b_k  (k = 5 .. 1),  W_all = P_1 W1
        P = sd["tgnn.conv5.lin.weight"]
        cs = [sd["tgnn.conv5.bias"].view(1, -1)]                                # c_5 = b_5
        for k in (4, 3, 2, 1):
            cs.append(LinearFunction.apply(sd[f"tgnn.conv{k}.bias"].view(1, -1), P, None))          # (P b_k)^T as a row
            wk = sd[f"tgnn.conv{k}.lin.weight"]
            P = _compose(P, wk)                                                 # P @ W_k
        zero = torch.zeros(3, self.HIDDEN, device=x.device)
        wcat = torch.cat([P.t()] + cs + [zero], dim=0).t().contiguous()         # (512, F + 8): [W_all | c_5 c_4 c_3 c_2 c_1 | 0 0 0]
        h = LinearFunction.apply(feat, wcat, None)                              # (M, 512)
        return cell_run(x, h, op, *[sd[k] for k in PARAM_NAMES_CELL])      # (CellFunction, or forward-only without a gradient)

    def forward_layerwise(self, x: torch.Tensor, op: GcnOperator):
        """The reference's evaluation order: every layer aggregates its (learned) input at width T*512."""
        _need_cuda(x)
        n, f, t = x.shape
        c = self.HIDDEN
        sd = dict(self.named_parameters())
        xp = ops.pack_x(x)                                                      # (N, T, F)
        ax = ops.spmm_csr(op.rowptr, op.col, op.val, xp.view(n, t * f))          # A_hat x: input data, no backward
        h = LinearFunction.apply(ax.view(n * t, f), sd["tgnn.conv1.lin.weight"], sd["tgnn.conv1.bias"])
        for layer in range(2, 6):
            s = AggregateFunction.apply(h.view(n, t * c), op)
            h = LinearFunction.apply(s.view(n * t, c), sd[f"tgnn.conv{layer}.lin.weight"], sd[f"tgnn.conv{layer}.bias"])
        return cell_run(x, h, op, *[sd[k] for k in PARAM_NAMES_CELL])      # (CellFunction, or forward-only without a gradient)

    def forward(self, x, edge_index, edge_attr):
        _need_cuda(x)
        n = x.shape[0]
        op = self._graphs.get([edge_index, edge_attr], n, lambda: prepare_gcn_operator(edge_index, edge_attr, n))
        return self.forward_prepared(x, op)


# ---- GraphSAGE / GAT base blocks of the cell (second half) ---------------------------------------------
# Both reference models call ``self._base_tgcn(X[:, :, period], edge_index, H)``: TGCN.forward's third positional parameter is
# ``edge_weight``, so H stays None and the cell starts from zeros in every period (models/utils.py:163-166).  With H = 0 the
# reset gate only multiplies zeros: Z = sigmoid(U_z1 conv_z(x) + u_z), H~ = tanh(U_h1 conv_h(x) + u_h), H' = (1 - Z) H~
# -- every contraction has K = F (or 2F), the sparse operators act on the input, and the whole model is one aggregation, two
# skinny MFMA GEMMs with sigmoid / tanh epilogues, a blend + attention sum and the head (regt_cell0_forward).

def _compose(u1: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """U1 (C,C) @ W (C,K) on the matrix cores with autograd (regt_linear / regt_wgrad)."""
    return LinearFunction.apply(u1, w.t().contiguous(), None)


def _compose_bias(u1: torch.Tensor, b: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """U1 b + u."""
    return LinearFunction.apply(b.view(1, -1), u1, None).view(-1) + u


class GraphSAGE(nn.Module):
    """Parameter layout of models/GraphSAGETemporalGCN.py:46-72: TGCN cell with SAGEConv gates, a never-called GCNConv
    ``conv`` (:61-64), the attention over periods and the dead ``_weight_att*`` / ``_bias_att*`` of the A3T-GCN template."""

    def __init__(self, in_channels: int, out_channels: int, num_nodes: int, periods: int):
        super().__init__()
        self.in_channels, self.out_channels, self.num_nodes, self.periods = in_channels, out_channels, num_nodes, periods
        self._attention = nn.Parameter(torch.empty(periods))
        self._weight_att1 = nn.Parameter(torch.normal(0.0, 0.1, size=(out_channels, 1)))
        self._weight_att2 = nn.Parameter(torch.normal(0.0, 0.1, size=(num_nodes, 1)))
        self._bias_att1 = nn.Parameter(torch.normal(0.0, 1.0, size=(1, 1)))
        self._bias_att2 = nn.Parameter(torch.normal(0.0, 1.0, size=(1, 1)))
        self._base_tgcn = TGCN(in_channels, out_channels, baseblock="graphsage")
        self.conv = _GCNConvParams(in_channels, out_channels)
        nn.init.uniform_(self._attention)


class GAT(nn.Module):
    """Parameter layout of models/GATTemporal.py:37-64: TGCN cell with GATConv gates and the attention over periods."""

    def __init__(self, in_channels: int, out_channels: int, num_nodes: int, periods: int):
        super().__init__()
        self.in_channels, self.out_channels, self.num_nodes, self.periods = in_channels, out_channels, num_nodes, periods
        self._attention = nn.Parameter(torch.empty(periods))
        self._base_tgcn = TGCN(in_channels, out_channels, baseblock="gat")
        self.relu = nn.ReLU()
        nn.init.uniform_(self._attention)


def _pad_features(x: torch.Tensor):
    """(N, F, T) -> the same with F rounded up to a multiple of 4 by zero feature rows, and the number of rows added.  Any node
    feature width is accepted, as in the reference; zero features under zero weight columns change nothing, and autograd slices
    the gradients of the padded weights back."""
    fpad = (-x.shape[1]) % 4
    return (torch.nn.functional.pad(x, (0, 0, 0, fpad)).contiguous() if fpad else x), fpad


def _pad_cols(w: torch.Tensor, fpad: int) -> torch.Tensor:
    return torch.nn.functional.pad(w, (0, fpad)) if fpad else w


class _ZeroHiddenModel(nn.Module):
    cell_attr: str

    def _cell(self) -> TGCN:
        return getattr(self, self.cell_attr)._base_tgcn

    def _run_cell0(self, a_z, a_h, gz, gh, cz, ch, num_nodes: int):
        inner = getattr(self, self.cell_attr)
        pred, hidden = Cell0Function.apply(a_z, a_h, gz, gh, cz, ch, inner._attention, self.linear1.weight, self.linear1.bias,
                                           self.linear2.weight, self.linear2.bias, num_nodes)
        cell = self._cell()
        dead = list(cell.conv_r.parameters()) + list(cell.linear_r.parameters())     # reset gate: multiplied by H = 0
        return ZeroGradAnchor.apply(pred, hidden, *dead)


class GraphSAGETemporalGCN(_ZeroHiddenModel):
    """GraphSAGE baseline (models/GraphSAGETemporalGCN.py:8-43).  ``forward(x, edge_index, edge_attr)`` ->
    ``(prediction (N, output_dim), hidden (N, 256))``; ``edge_attr`` is accepted and ignored, as in the reference (:93-95)."""

    cell_attr = "tgnn"

    def __init__(self, node_features: int, num_nodes: int, periods: int, output_dim: int, hidden_channels: int = HIDDEN):
        super().__init__()
        self.tgnn = GraphSAGE(node_features, hidden_channels, num_nodes, periods)
        self.output_dim = output_dim
        self.linear1 = nn.Linear(hidden_channels, HEAD_HIDDEN)
        self.linear2 = nn.Linear(HEAD_HIDDEN, output_dim)
        self.relu = nn.ReLU()
        self._graphs = _GraphCache()

    def prepare_graph(self, edge_index, num_nodes: int, copies: int = 1) -> MeanOperator:
        return prepare_mean_operator(edge_index, num_nodes, copies)

    def forward_prepared(self, x: torch.Tensor, op: MeanOperator):
        _need_cuda(x)
        x, fpad = _pad_features(x)            # the kernels read 16-byte feature rows: zero columns for x and for the weights
        n, f, t = x.shape
        c = self.tgnn.out_channels
        cell = self.tgnn._base_tgcn
        xp = ops.pack_x(x)                                                        # (N, T, F)
        ax = ops.spmm_csr(op.rowptr, op.col, op.val, xp.view(n, t * f))           # mean over in-neighbours: input data, no backward
        a = torch.cat([ax.view(n * t, f), xp.view(n * t, f)], dim=1)              # [mean-neighbour x | x]  (M, 2F)
        gs, cs = [], []
        for conv, lin in ((cell.conv_z, cell.linear_z), (cell.conv_h, cell.linear_h)):
            u1 = lin.weight[:, :c].contiguous()
            gs.append(torch.cat([_compose(u1, _pad_cols(conv.lin_l.weight, fpad)), _compose(u1, _pad_cols(conv.lin_r.weight, fpad))], dim=1))
            cs.append(_compose_bias(u1, conv.lin_l.bias, lin.bias))
        return self._run_cell0(a, a, gs[0], gs[1], cs[0], cs[1], n)

    def forward(self, x, edge_index, edge_attr=None):
        _need_cuda(x)
        n = x.shape[0]
        op = self._graphs.get([edge_index, None], n, lambda: prepare_mean_operator(edge_index, n))
        return self.forward_prepared(x, op)


class GATTemporal(_ZeroHiddenModel):
    """GAT baseline (models/GATTemporal.py:7-34).  ``forward(x, edge_index, edge_attr)`` -> ``(prediction, hidden (N, 256))``;
    ``edge_attr`` is accepted and ignored, as in the reference (:78-80)."""

    cell_attr = "gat"
    NEGATIVE_SLOPE = 0.2          # GATConv default

    def __init__(self, node_features: int, num_nodes: int, periods: int, output_dim: int, hidden_channels: int = HIDDEN):
        super().__init__()
        self.gat = GAT(node_features, hidden_channels, num_nodes, periods)
        self.output_dim = output_dim
        self.linear1 = nn.Linear(hidden_channels, HEAD_HIDDEN)
        self.linear2 = nn.Linear(HEAD_HIDDEN, output_dim)
        self.relu = nn.ReLU()
        self._graphs = _GraphCache()

    def prepare_graph(self, edge_index, num_nodes: int, copies: int = 1) -> AttentionPattern:
        return prepare_attention_pattern(edge_index, num_nodes, copies)

    def forward_prepared(self, x: torch.Tensor, pat: AttentionPattern):
        _need_cuda(x)
        x, fpad = _pad_features(x)
        n, f, t = x.shape
        c = self.gat.out_channels
        cell = self.gat._base_tgcn
        xp = ops.pack_x(x)
        ins, gs, cs = [], [], []
        for conv, lin in ((cell.conv_z, cell.linear_z), (cell.conv_h, cell.linear_h)):
            w = _pad_cols(conv.lin.weight, fpad)                                   # (C, F)
            u_src = LinearFunction.apply(conv.att_src.view(1, c), w.t().contiguous(), None).view(f)      # W^T att_src
            u_dst = LinearFunction.apply(conv.att_dst.view(1, c), w.t().contiguous(), None).view(f)
            ins.append(GatAggregateFunction.apply(xp, u_src, u_dst, pat, self.NEGATIVE_SLOPE).view(n * t, f))
            u1 = lin.weight[:, :c].contiguous()
            gs.append(_compose(u1, w))
            cs.append(_compose_bias(u1, conv.bias, lin.bias))
        return self._run_cell0(ins[0], ins[1], gs[0], gs[1], cs[0], cs[1], n)

    def forward(self, x, edge_index, edge_attr=None):
        _need_cuda(x)
        n = x.shape[0]
        pat = self._graphs.get([edge_index, None], n, lambda: prepare_attention_pattern(edge_index, n))
        return self.forward_prepared(x, pat)


# ---- SpatialGCN (models/SpatialGCN.py) ---------------------------------------------------------------------------------------

def draw_keep_mask(rows: int, device) -> torch.Tensor:
    """F.dropout(p = 0.5) keep bits for ``rows`` (node*T + t) rows of 64 channels: (rows, 2) int32, bit j of word w keeps channel
    32w + j.  Random bytes viewed as int32 (``int32.random_()`` never sets the top bit, which would always drop channel 31 of a word)."""
    return torch.randint(0, 256, (rows, 8), dtype=torch.uint8, device=device).view(torch.int32)


class SpatialGCN(nn.Module):
    """Two ChebConv(K=2) layers with ReLU and dropout between them, summed over the periods, and a 256 -> 128 -> O head
    (models/SpatialGCN.py:8-49).  ``forward(x, edge_index, edge_attr)`` -> ``(prediction (N, output_dim), H (N, 256))``, H being
    the period sum itself (the reference's ``relu(H_accum)`` on :45 is never used).

    gcn2 is linear and its outputs are summed over the periods, so H = S V0^T + (L~ S) V1^T + T c with S = sum_t dropout(relu(
    gcn(x_t))) (N, 64): the first layer is one kernel pair (regt_spatial_embed_forward / _backward, which folds ReLU, the dropout
    mask and the period sum), the second is one aggregation at width 64 and one (N x 128) . (128 x 256) GEMM.  Dropout follows
    ``self.training``: in training mode one fresh mask is drawn on the device per call, unless ``forward_prepared`` is given
    ``keep`` ((N*T, 2) int32 mask bits, see :func:`draw_keep_mask`)."""

    CHANNELS = 64         # models/SpatialGCN.py:14
    HIDDEN = 256          # :19
    DROPOUT = 0.5         # F.dropout default, :41

    def __init__(self, node_features: int, periods: int, output_dim: int):
        super().__init__()
        self.gcn = _ChebConvParams(node_features, self.CHANNELS)
        self.gcn2 = _ChebConvParams(self.CHANNELS, self.HIDDEN)
        self.periods = periods
        self.output_dim = output_dim
        self.linear1 = nn.Linear(self.HIDDEN, HEAD_HIDDEN)
        self.linear2 = nn.Linear(HEAD_HIDDEN, output_dim)
        self.relu = nn.ReLU()
        self.leakyRelu = nn.LeakyReLU()
        self._graphs = _GraphCache()

    def prepare_graph(self, edge_index, edge_attr, num_nodes: int, copies: int = 1) -> GcnOperator:
        return prepare_cheb_operator(edge_index, edge_attr, num_nodes, copies)

    def forward_prepared(self, x: torch.Tensor, op: GcnOperator, keep: Optional[torch.Tensor] = None):
        _need_cuda(x)
        if x.shape[2] != self.periods:
            raise ValueError(f"x has {x.shape[2]} periods, the model {self.periods}")
        x, fpad = _pad_features(x)            # the kernels read 16-byte feature rows: zero columns for x and for the weights
        n, f, t = x.shape
        if self.training:
            keep = draw_keep_mask(n * t, x.device) if keep is None else keep
        else:
            keep = None                       # F.dropout(training=False) is the identity
        xp = ops.pack_x(x)                                                              # (N, T, F)
        lxp = ops.spmm_csr(op.rowptr, op.col, op.val, xp.view(n, t * f)).view(n, t, f)  # L~ x: input data, no backward
        s = SpatialEmbedFunction.apply(xp, lxp, _pad_cols(self.gcn.lins[0].weight, fpad), _pad_cols(self.gcn.lins[1].weight, fpad),
                                       self.gcn.bias, keep)                            # (N, 64)
        ls = AggregateFunction.apply(s, op)                                             # L~ S
        v = torch.cat([self.gcn2.lins[0].weight, self.gcn2.lins[1].weight], dim=1)     # (256, 128)
        h = LinearFunction.apply(torch.cat([s, ls], dim=1), v, self.gcn2.bias * t)     # H = S V0^T + (L~ S) V1^T + T c
        z = torch.relu(LinearFunction.apply(h, self.linear1.weight, self.linear1.bias))
        return LinearFunction.apply(z, self.linear2.weight, self.linear2.bias), h

    def forward(self, x, edge_index, edge_attr):
        _need_cuda(x)
        n = x.shape[0]
        op = self._graphs.get([edge_index, edge_attr], n, lambda: prepare_cheb_operator(edge_index, edge_attr, n))
        return self.forward_prepared(x, op)


# ---- STNorm (models/STNorm.py) ---------------------------------------------------------------------------------------------------------

class _SNormParams(nn.Module):
    """SNorm's parameters (models/STNorm.py:6-19): beta, gamma (channels,)."""

    def __init__(self, channels: int):
        super().__init__()
        self.beta = nn.Parameter(torch.zeros(channels))
        self.gamma = nn.Parameter(torch.ones(channels))


class _TNormParams(nn.Module):
    """TNorm's parameters and running statistics (models/STNorm.py:22-57): beta, gamma, running_mean, running_var (1, C, N, 1)."""

    def __init__(self, num_nodes: int, channels: int, momentum: float = 0.1):
        super().__init__()
        self.beta = nn.Parameter(torch.zeros(1, channels, num_nodes, 1))
        self.gamma = nn.Parameter(torch.ones(1, channels, num_nodes, 1))
        self.register_buffer("running_mean", torch.zeros(1, channels, num_nodes, 1))
        self.register_buffer("running_var", torch.ones(1, channels, num_nodes, 1))
        self.momentum = momentum


class STNorm(nn.Module):
    """STNorm (models/STNorm.py:60-185): the reference's constructor, ``forward(input (B, L, N, C_in)) -> (B, out_dim, N, L_out)`` and
    state_dict.  All arithmetic runs in regt_stnorm_forward / regt_stnorm_backward; ``nn.Conv2d`` modules only hold the weights, and
    are created in the reference's order so that a seeded construction draws the same initial values.

    ``tnorm_group`` (forward keyword): TNorm pools its statistics over groups of that many consecutive batch elements.  The default,
    the whole batch, is the reference's semantics; ``tnorm_group=1`` makes a batch of B snapshots equal to B sequential calls with
    B = 1 (the running buffers are updated once per snapshot, in order) -- what snapshot batching in ``train.py`` uses."""

    def __init__(self, num_nodes, tnorm_bool=True, snorm_bool=True, in_dim=1, out_dim=12, channels=16, kernel_size=2, blocks=4, layers=2):
        super().__init__()
        if channels != ops.STNORM_CHANNELS or kernel_size != 2:
            raise ValueError(f"STNorm runs with channels={ops.STNORM_CHANNELS} and kernel_size=2 only, got {channels}, {kernel_size}")
        if not 1 <= in_dim <= ops.STNORM_MAX_DIM or not 1 <= out_dim <= ops.STNORM_MAX_DIM:
            raise ValueError(f"STNorm runs with 1 <= in_dim, out_dim <= {ops.STNORM_MAX_DIM}, got {in_dim}, {out_dim}")
        self.num_nodes, self.in_dim, self.out_dim = num_nodes, in_dim, out_dim
        self.blocks, self.layers = blocks, layers
        self.snorm_bool, self.tnorm_bool = snorm_bool, tnorm_bool
        self.filter_convs = nn.ModuleList()
        self.gate_convs = nn.ModuleList()
        self.residual_convs = nn.ModuleList()
        self.skip_convs = nn.ModuleList()
        if snorm_bool:
            self.sn = nn.ModuleList()
        if tnorm_bool:
            self.tn = nn.ModuleList()
        wide = (1 + int(tnorm_bool) + int(snorm_bool)) * channels
        self.start_conv = nn.Conv2d(in_dim, channels, kernel_size=(1, 1))
        rf = 1
        for _ in range(blocks):
            scope, dilation = kernel_size - 1, 1
            for _ in range(layers):
                if tnorm_bool:
                    self.tn.append(_TNormParams(num_nodes, channels))
                if snorm_bool:
                    self.sn.append(_SNormParams(channels))
                self.filter_convs.append(nn.Conv2d(wide, channels, kernel_size=(1, kernel_size), dilation=dilation))
                self.gate_convs.append(nn.Conv2d(wide, channels, kernel_size=(1, kernel_size), dilation=dilation))
                self.residual_convs.append(nn.Conv2d(channels, channels, kernel_size=(1, 1)))
                self.skip_convs.append(nn.Conv2d(channels, channels, kernel_size=(1, 1)))
                dilation *= 2
                rf += scope
                scope *= 2
        self.end_conv_1 = nn.Conv2d(channels, channels, kernel_size=(1, 1), bias=True)
        self.end_conv_2 = nn.Conv2d(channels, out_dim, kernel_size=(1, 1), bias=True)
        self.receptive_field = rf

    def param_table(self):
        """The parameters in the table order of regt_stnorm_forward (None where TNorm / SNorm is off)."""
        t = [self.start_conv.weight, self.start_conv.bias, self.end_conv_1.weight, self.end_conv_1.bias, self.end_conv_2.weight,
             self.end_conv_2.bias]
        for i in range(self.blocks * self.layers):
            t += [self.filter_convs[i].weight, self.filter_convs[i].bias, self.gate_convs[i].weight, self.gate_convs[i].bias,
                  self.residual_convs[i].weight, self.residual_convs[i].bias, self.skip_convs[i].weight, self.skip_convs[i].bias]
            t += [self.tn[i].gamma, self.tn[i].beta] if self.tnorm_bool else [None, None]
            t += [self.sn[i].gamma, self.sn[i].beta] if self.snorm_bool else [None, None]
        return t

    def running_table(self):
        r = []
        if self.tnorm_bool:
            for m in self.tn:
                r += [m.running_mean, m.running_var]
        return r

    def forward(self, input: torch.Tensor, tnorm_group: Optional[int] = None) -> torch.Tensor:
        _need_cuda(input)
        if input.dim() != 4 or input.shape[2] != self.num_nodes or input.shape[3] != self.in_dim:
            raise ValueError(f"input must be (B, L, {self.num_nodes}, {self.in_dim}), got {tuple(input.shape)}")
        b, l = input.shape[0], input.shape[1]
        group = b if tnorm_group is None else int(tnorm_group)
        dims = ops.stnorm_dims(self.num_nodes, b, group, l, self.in_dim, self.out_dim, self.blocks, self.layers, self.tnorm_bool,
                               self.snorm_bool, self.training)
        params = self.param_table()
        ops.stnorm_check_tables(dims, input.device, params, self.running_table())   # raw pointers: device, dtype, shape, layout
        if input.dtype != torch.float32:
            raise _lib.RegtError(f"STNorm input must be float32, got {input.dtype}")
        return STNormFunction.apply(input.contiguous(), dims, self.running_table(), *params)


# ---- STID (models/STID.py) -------------------------------------------------------------------------------------------------------------

def draw_stid_keep(num_layer: int, batch: int, num_nodes: int, hidden: int, device, p: float = ops.STID_DROPOUT) -> torch.Tensor:
    """nn.Dropout(p) keep bits for STID's blocks: (num_layer, batch, num_nodes, hidden / 32) int32, bit j of word w keeps channel
    32w + j, every bit an independent Bernoulli(1 - p) draw from torch's generator of ``device``.  The bits are packed bytewise and
    the bytes viewed as int32, so the top bit of a word is as live as the others (see :func:`draw_keep_mask`)."""
    weights = (2 ** torch.arange(8, device=device)).to(torch.uint8)
    out = torch.empty(num_layer, batch, num_nodes, hidden // 32, dtype=torch.int32, device=device)
    for l in range(num_layer):                                    # layer by layer: bounds the transient to 128 bytes per word
        bits = torch.rand(batch, num_nodes, hidden // 8, 8, device=device) >= p
        out[l] = (bits.to(torch.uint8) * weights).sum(-1, dtype=torch.uint8).view(torch.int32)
    return out


class _MLPParams(nn.Module):
    """Parameters of one residual block (models/STID.py:5-15): fc1, fc2 1x1 convolutions."""

    def __init__(self, hidden: int):
        super().__init__()
        self.fc1 = nn.Conv2d(hidden, hidden, kernel_size=(1, 1), bias=True)
        self.fc2 = nn.Conv2d(hidden, hidden, kernel_size=(1, 1), bias=True)


class STID(nn.Module):
    """STID (models/STID.py:32-157) with the reference's constructor, ``forward(history_data (B, L, N, C)) -> (B, output_len, N, 1)``
    and state_dict, for the configuration run.py:134 / predict.py:133 build: ``if_time_in_day=False, if_day_in_week=False``.  All
    arithmetic runs in regt_stid_forward / regt_stid_backward; the ``nn.Conv2d`` modules only hold weights and are created in the
    reference's order, so a seeded construction draws the same initial values.

    Dropout (p = 0.15 inside every block) follows ``self.training``: a training-mode call draws fresh keep bits on the device
    (:func:`draw_stid_keep`) unless ``keep=`` supplies them, and leaves the bits it used in ``self.last_keep``.  Eval mode ignores
    ``keep``.  A strided ``history_data`` (train.py's window view) is made contiguous once here; the kernels gather the first
    ``input_dim`` features of each time step from that tensor themselves."""

    def __init__(self, num_nodes, input_len=12, output_len=12, input_dim=3, embed_dim=32, node_dim=32, temp_dim_tid=32, temp_dim_diw=32,
                 time_of_day_size=288, day_of_week_size=7, if_node=True, if_time_in_day=True, if_day_in_week=True, num_layer=3):
        super().__init__()
        if if_time_in_day or if_day_in_week:
            raise ValueError("STID runs with if_time_in_day=False and if_day_in_week=False only (as run.py and predict.py construct it): "
                             "the time-of-day / day-of-week embeddings index their tables with a dataset-specific feature convention "
                             "(models/STID.py:116-125) that the TPIMS data does not follow")
        if num_nodes < 1:
            raise ValueError(f"STID needs num_nodes >= 1, got num_nodes={num_nodes}")
        ops.stid_limits(input_len, output_len, input_dim, embed_dim, node_dim, num_layer)
        self.num_nodes, self.node_dim, self.input_len, self.input_dim = num_nodes, node_dim, input_len, input_dim
        self.embed_dim, self.output_len, self.num_layer = embed_dim, output_len, num_layer
        self.temp_dim_tid, self.temp_dim_diw = temp_dim_tid, temp_dim_diw
        self.time_of_day_size, self.day_of_week_size = time_of_day_size, day_of_week_size
        self.if_time_in_day, self.if_day_in_week, self.if_spatial = if_time_in_day, if_day_in_week, bool(if_node)
        if self.if_spatial:
            self.node_emb = nn.Parameter(torch.empty(num_nodes, node_dim))
            nn.init.xavier_uniform_(self.node_emb)
        self.time_series_emb_layer = nn.Conv2d(input_dim * input_len, embed_dim, kernel_size=(1, 1), bias=True)
        self.hidden_dim = embed_dim + node_dim * int(self.if_spatial)
        self.encoder = nn.Sequential(*[_MLPParams(self.hidden_dim) for _ in range(num_layer)])
        self.regression_layer = nn.Conv2d(self.hidden_dim, output_len, kernel_size=(1, 1), bias=True)
        self.last_keep = None

    def param_table(self):
        """The parameters in state_dict order, the table order of regt_stid_forward (None for node_emb when if_node is off)."""
        t = [self.node_emb if self.if_spatial else None, self.time_series_emb_layer.weight, self.time_series_emb_layer.bias]
        for m in self.encoder:
            t += [m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias]
        return t + [self.regression_layer.weight, self.regression_layer.bias]

    def forward(self, history_data: torch.Tensor, *, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        _need_cuda(history_data)
        if history_data.dim() != 4 or history_data.shape[1] != self.input_len or history_data.shape[2] != self.num_nodes \
                or history_data.shape[3] < self.input_dim:
            raise ValueError(f"history_data must be (B, {self.input_len}, {self.num_nodes}, C >= {self.input_dim}), got "
                             f"{tuple(history_data.shape)}")
        if history_data.dtype != torch.float32:
            raise _lib.RegtError(f"STID input must be float32, got {history_data.dtype}")
        b, c = history_data.shape[0], history_data.shape[3]
        dims = ops.stid_dims(self.num_nodes, b, self.input_len, c, self.input_dim, self.num_layer, self.output_len, self.if_spatial,
                             self.embed_dim, self.node_dim)
        params = self.param_table()
        ops.stid_check_tables(dims, history_data.device, params)            # raw pointers: device, dtype, shape, layout
        if self.training:
            if keep is None:
                keep = draw_stid_keep(self.num_layer, b, self.num_nodes, self.hidden_dim, history_data.device)
            self.last_keep = keep
        else:
            keep = None
        return STIDFunction.apply(history_data.contiguous(), dims, keep, *params)


# ---- StackedGRU (models/StackedGRU.py) ----------------------------------------------------------------------------------------------

class StackedGRU(nn.Module):
    """StackedGRU (models/StackedGRU.py:4-30) with the reference's constructor, ``forward(x (N, rows, T), edge_index) ->
    (N, rows, output_dim)`` and 12-entry state_dict.  ``nn.GRU`` is sequence-first, so -- exactly as in the reference -- the
    sequence runs over the N nodes, the 8 node features (or 8 B of them for B stacked snapshots) are independent batch rows and
    the T periods are the input vector.  ``gru``'s sequence output is dead in the reference (its relu is overwritten): only its
    final state is computed, as ``gru2``'s initial state.  All arithmetic runs in regt_gru_forward / regt_gru_backward and the
    dense entry points; the ``nn.GRU`` / ``nn.Linear`` modules only hold weights and are created in the reference's order, so a
    seeded construction draws the same initial values.  ``x`` is read in place through its strides."""

    def __init__(self, in_channels, node_features, periods, output_dim):
        super().__init__()
        hidden_dim = ops.GRU_HIDDEN
        ops.gru_limits(in_channels, hidden_dim)
        if output_dim < 1:
            raise ValueError(f"StackedGRU needs output_dim >= 1, got output_dim={output_dim}")
        self.in_channels, self.output_dim, self.periods, self.node_features = in_channels, output_dim, periods, node_features
        self.gru = nn.GRU(input_size=in_channels, hidden_size=hidden_dim)
        self.gru2 = nn.GRU(input_size=in_channels, hidden_size=hidden_dim)
        self.linear1 = nn.Linear(hidden_dim, hidden_dim)
        self.linear2 = nn.Linear(hidden_dim, output_dim)

    @staticmethod
    def _weights(g: nn.GRU):
        return [g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0]

    def forward(self, x: torch.Tensor, edge_index=None) -> torch.Tensor:
        _need_cuda(x)
        if x.dim() != 3 or x.shape[2] != self.in_channels or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"x must be (N, rows, {self.in_channels}), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise _lib.RegtError(f"StackedGRU input must be float32, got {x.dtype}")
        w1, w2 = self._weights(self.gru), self._weights(self.gru2)
        ops.gru_check_weights(self.in_channels, x.device, w1, "StackedGRU.gru")
        ops.gru_check_weights(self.in_channels, x.device, w2, "StackedGRU.gru2")
        _, h = GRUFunction.apply(x, None, False, True, *w1)
        out, _ = GRUFunction.apply(x, h, True, False, *w2)
        y = MLPHeadFunction.apply(out.view(-1, ops.GRU_HIDDEN), self.linear1.weight, self.linear1.bias, self.linear2.weight,
                                  self.linear2.bias)
        return y.view(x.shape[0], x.shape[1], self.output_dim)


# ---- STAEformer, inference only (models/STAEformer.py) ---------------------------------------------------------------------------------

class _STAEAttentionParams(nn.Module):
    """Parameters of one multi-head attention (models/STAEformer.py:20-33): the three projections and out_proj."""

    def __init__(self, model_dim: int):
        super().__init__()
        self.FC_Q = nn.Linear(model_dim, model_dim)
        self.FC_K = nn.Linear(model_dim, model_dim)
        self.FC_V = nn.Linear(model_dim, model_dim)
        self.out_proj = nn.Linear(model_dim, model_dim)


class _STAELayerParams(nn.Module):
    """Parameters of one self-attention layer (models/STAEformer.py:77-91), registered in the reference's order."""

    def __init__(self, model_dim: int, feed_forward_dim: int):
        super().__init__()
        self.attn = _STAEAttentionParams(model_dim)
        self.feed_forward = nn.Sequential(nn.Linear(model_dim, feed_forward_dim), nn.ReLU(inplace=True), nn.Linear(feed_forward_dim, model_dim))
        self.ln1 = nn.LayerNorm(model_dim)
        self.ln2 = nn.LayerNorm(model_dim)

    def table(self):
        a, f = self.attn, self.feed_forward
        return [a.FC_Q.weight, a.FC_Q.bias, a.FC_K.weight, a.FC_K.bias, a.FC_V.weight, a.FC_V.bias, a.out_proj.weight, a.out_proj.bias,
                f[0].weight, f[0].bias, f[2].weight, f[2].bias, self.ln1.weight, self.ln1.bias, self.ln2.weight, self.ln2.bias]


class STAEformer(nn.Module):
    """STAEformer (models/STAEformer.py:110-255) with the reference's constructor, ``forward(x (B, in_steps, N, F)) ->
    (B, out_steps, N, output_dim)`` and state_dict, for INFERENCE: what run.py::test() and predict.py do with the model.  All
    arithmetic runs in regt_stae_forward; the ``nn.Linear`` / ``nn.Embedding`` / ``nn.LayerNorm`` modules only hold weights and are
    created in the reference's order, so a seeded construction draws the same initial values.

    ``forward`` raises NotImplementedError ("inference only") where autograd would record the call (grad mode on and the input or a
    parameter requires grad) and in training mode with ``dropout > 0``: wrap the call in ``torch.no_grad()`` and ``eval()``.
    Constructions outside the kernels' limits (head width 32, ``use_mixed_proj=True``, ...; include/regtgcn.h) raise
    NotImplementedError here: run.py:132 passes ``tod_embedding_dim=0``, which gives model_dim 128 = 4 heads of 32, while the class
    default (model_dim 152, head width 38) is refused.  The day-of-week and time-of-day indices are clamped into their tables."""

    def __init__(self, num_nodes, in_steps=12, out_steps=12, steps_per_day=288, days_per_week=7, input_dim=3, output_dim=1,
                 input_embedding_dim=24, tod_embedding_dim=24, dow_embedding_dim=24, spatial_embedding_dim=0, adaptive_embedding_dim=80,
                 feed_forward_dim=256, num_heads=4, num_layers=3, dropout=0.1, use_mixed_proj=True):
        super().__init__()
        self.num_nodes, self.in_steps, self.out_steps = num_nodes, in_steps, out_steps
        self.steps_per_day, self.days_per_week, self.input_dim, self.output_dim = steps_per_day, days_per_week, input_dim, output_dim
        self.input_embedding_dim, self.tod_embedding_dim, self.dow_embedding_dim = input_embedding_dim, tod_embedding_dim, dow_embedding_dim
        self.spatial_embedding_dim, self.adaptive_embedding_dim = spatial_embedding_dim, adaptive_embedding_dim
        self.model_dim = input_embedding_dim + tod_embedding_dim + dow_embedding_dim + spatial_embedding_dim + adaptive_embedding_dim
        self.feed_forward_dim, self.num_heads, self.num_layers = feed_forward_dim, num_heads, num_layers
        self.dropout, self.use_mixed_proj = float(dropout), use_mixed_proj
        if num_nodes < 1 or input_embedding_dim < 1 or min(tod_embedding_dim, dow_embedding_dim, spatial_embedding_dim, adaptive_embedding_dim) < 0 \
                or steps_per_day < 1 or days_per_week < 1:
            raise ValueError("STAEformer needs num_nodes, input_embedding_dim, steps_per_day, days_per_week >= 1 and embedding widths >= 0")
        ops.stae_limits(in_steps, out_steps, input_dim, output_dim, self.model_dim, num_heads, feed_forward_dim, num_layers, use_mixed_proj)
        self.input_proj = nn.Linear(input_dim, input_embedding_dim)
        if tod_embedding_dim > 0:
            self.tod_embedding = nn.Embedding(steps_per_day, tod_embedding_dim)
        if dow_embedding_dim > 0:
            self.dow_embedding = nn.Embedding(days_per_week, dow_embedding_dim)
        if spatial_embedding_dim > 0:
            self.node_emb = nn.Parameter(torch.empty(num_nodes, spatial_embedding_dim))
            nn.init.xavier_uniform_(self.node_emb)
        if adaptive_embedding_dim > 0:
            self.adaptive_embedding = nn.Parameter(torch.empty(in_steps, num_nodes, adaptive_embedding_dim))
            nn.init.xavier_uniform_(self.adaptive_embedding)
        self.output_proj = nn.Linear(in_steps * self.model_dim, out_steps * output_dim)
        self.attn_layers_t = nn.ModuleList([_STAELayerParams(self.model_dim, feed_forward_dim) for _ in range(num_layers)])
        self.attn_layers_s = nn.ModuleList([_STAELayerParams(self.model_dim, feed_forward_dim) for _ in range(num_layers)])

    def param_table(self):
        """The parameters in state_dict order, the table order of regt_stae_forward (None where an embedding's width is 0)."""
        t = [self.node_emb if self.spatial_embedding_dim > 0 else None, self.adaptive_embedding if self.adaptive_embedding_dim > 0 else None,
             self.input_proj.weight, self.input_proj.bias, self.tod_embedding.weight if self.tod_embedding_dim > 0 else None,
             self.dow_embedding.weight if self.dow_embedding_dim > 0 else None, self.output_proj.weight, self.output_proj.bias]
        for m in list(self.attn_layers_t) + list(self.attn_layers_s):
            t += m.table()
        return t

    def dims(self, batch: int, in_features: int) -> _lib.StaeDims:
        return _lib.StaeDims(batch, self.in_steps, self.num_nodes, in_features, self.input_dim, self.input_embedding_dim,
                             self.tod_embedding_dim, self.dow_embedding_dim, self.spatial_embedding_dim, self.adaptive_embedding_dim,
                             self.steps_per_day, self.days_per_week, self.num_heads, self.feed_forward_dim, self.num_layers, self.out_steps,
                             self.output_dim, int(bool(self.use_mixed_proj)), float(self.attn_layers_t[0].ln1.eps))

    def _check_x(self, x: torch.Tensor):
        _need_cuda(x)
        need = max(self.input_dim, 2 if self.tod_embedding_dim > 0 else 0, 3 if self.dow_embedding_dim > 0 else 0)
        if x.dim() != 4 or x.shape[1] != self.in_steps or x.shape[2] != self.num_nodes or x.shape[3] < need:
            raise ValueError(f"x must be (B, {self.in_steps}, {self.num_nodes}, F >= {need}), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise _lib.RegtError(f"STAEformer input must be float32, got {x.dtype}")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_x(x)
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("STAEformer is inference only here (no backward kernels): call it under torch.no_grad()")
        if self.training and self.dropout > 0:
            raise NotImplementedError(f"STAEformer is inference only here: training mode with dropout={self.dropout} would draw dropout "
                                      "masks; call eval() first")
        dims = self.dims(x.shape[0], x.shape[3])
        params = [None if p is None else p.detach() for p in self.param_table()]
        return ops.stae_forward(dims, x.contiguous(), params)


class SelfAttentionLayer(_STAELayerParams):
    """One self-attention layer of STAEformer (models/STAEformer.py:76-107), TRAINABLE, with the reference's constructor,
    ``forward(x, dim=-2)`` and 16-entry state_dict (attn.FC_Q.weight ... attn.out_proj.bias, feed_forward.0.*, feed_forward.2.*,
    ln1.*, ln2.*).  ``x`` is (B, T, N, model_dim) with attention along ``dim`` 1 / -3 (time) or 2 / -2 (nodes), or (B, L, model_dim)
    with ``dim`` 1 / -2, taken as (B, 1, L, model_dim); nothing is transposed in memory, the kernels read a sequence through its row
    stride.  ``x`` receives its gradient, so layers stack.

    Launches: Q, K, V come from ONE projection GEMM over the concatenated weights (x is read once; its backward is one data-gradient
    GEMM and one weight-gradient call for the three), then attention, out_proj, add+LayerNorm, the two feed-forward GEMMs and the
    second add+LayerNorm.  All arithmetic runs in the HIP library; the ``nn.Linear`` / ``nn.LayerNorm`` modules only hold weights.

    NotImplementedError: head width other than 32, model_dim > 256, a feed_forward_dim outside the dense entry points' use here,
    ``mask=True`` (STAEformer never masks) and training mode with ``dropout > 0`` (keep-bit dropout comes with whole-model training)."""

    def __init__(self, model_dim, feed_forward_dim=2048, num_heads=8, dropout=0, mask=False):
        ops.stae_layer_limits(model_dim, num_heads, feed_forward_dim)
        if mask:
            raise NotImplementedError("SelfAttentionLayer runs without the causal mask only (mask=False): STAEformer never masks")
        super().__init__(model_dim, feed_forward_dim)
        self.model_dim, self.feed_forward_dim, self.num_heads, self.dropout, self.mask = model_dim, feed_forward_dim, num_heads, float(dropout), False

    def forward(self, x: torch.Tensor, dim: int = -2) -> torch.Tensor:
        if self.training and self.dropout > 0:                       # a property of the module: refused whatever the input is
            raise NotImplementedError(f"SelfAttentionLayer in training mode runs with dropout=0 only, got dropout={self.dropout}: call "
                                      "eval() or construct it with dropout=0")
        _need_cuda(x)
        if x.dtype != torch.float32:
            raise _lib.RegtError(f"SelfAttentionLayer input must be float32, got {x.dtype}")
        d = self.model_dim
        if x.dim() == 4 and x.shape[-1] == d and dim in (1, 2, -3, -2):
            b, t, n = x.shape[:3]
            axis = 1 if dim in (1, -3) else 2
        elif x.dim() == 3 and x.shape[-1] == d and dim in (1, -2):
            b, t, n, axis = x.shape[0], 1, x.shape[1], 2
        else:
            raise ValueError(f"x must be (B, T, N, {d}) with dim in (1, 2, -3, -2) or (B, L, {d}) with dim in (1, -2), got "
                             f"{tuple(x.shape)}, dim={dim}")
        if b < 1 or t < 1 or n < 1:
            raise ValueError(f"x must have no empty axis, got {tuple(x.shape)}")
        rows = x.contiguous().view(b * t * n, d)
        return _stae_layer_rows(rows, self.table(), b, t, n, self.num_heads, axis, float(self.ln1.eps), float(self.ln2.eps)).view(x.shape)


def _stae_layer_rows(rows: torch.Tensor, p, b: int, t: int, n: int, heads: int, axis: int, eps1: float, eps2: float,
                     keep1: Optional[torch.Tensor] = None, keep2: Optional[torch.Tensor] = None, drop: float = 0.0) -> torch.Tensor:
    """One self-attention layer on (M, model_dim) rows; ``p`` the layer's 16-entry table (``_STAELayerParams.table``).  ``keep1`` /
    ``keep2``: int32 (M, model_dim / 32) keep words of dropout1 / dropout2 with probability ``drop`` (models/STAEformer.py:98-104), folded
    into the add+LayerNorm that follows; None: no dropout."""
    qkv = LinearFunction.apply(rows, torch.cat([p[0], p[2], p[4]]), torch.cat([p[1], p[3], p[5]]))
    a = STAEPackedAttentionFunction.apply(qkv, b, t, n, heads, axis)
    y = LinearFunction.apply(a, p[6], p[7])
    if keep1 is None:
        h = STAEAddLayerNormFunction.apply(rows, y, p[12], p[13], eps1)
    else:
        h = STAEDropAddLayerNormFunction.apply(rows, y, keep1, drop, p[12], p[13], eps1)
    f = MLPHeadFunction.apply(h, p[8], p[9], p[10], p[11])
    if keep2 is None:
        return STAEAddLayerNormFunction.apply(h, f, p[14], p[15], eps2)
    return STAEDropAddLayerNormFunction.apply(h, f, keep2, drop, p[14], p[15], eps2)


def draw_stae_keep(num_layers: int, rows: int, model_dim: int, device, p: float) -> torch.Tensor:
    """nn.Dropout(p) keep bits for STAEformer: int32 (4 * num_layers, rows, model_dim / 32), one site per dropout call -- the temporal
    layers first, then the spatial ones, within a layer dropout1 before dropout2.  Bit j of word w keeps column 32w + j, every bit an
    independent Bernoulli(1 - p) draw from torch's generator of ``device``.  The bits are packed bytewise and the bytes viewed as
    int32, so the top bit of a word is as live as the others (see :func:`draw_stid_keep`)."""
    weights = (2 ** torch.arange(8, device=device)).to(torch.uint8)
    out = torch.empty(4 * num_layers, rows, model_dim // 32, dtype=torch.int32, device=device)
    for site in range(4 * num_layers):                            # site by site: bounds the transient to 128 bytes per word
        bits = torch.rand(rows, model_dim // 8, 8, device=device) >= p
        out[site] = (bits.to(torch.uint8) * weights).sum(-1, dtype=torch.uint8).view(torch.int32)
    return out


class STAEformerTrainable(STAEformer):
    """:class:`STAEformer`, TRAINABLE: the same constructor, limits, parameter creation order, state_dict and checkpoints, so a
    checkpoint written here loads into :class:`STAEformer` (``evaluate --model STAEformer``) and back.

    ``forward(x, *, keep=None)``.  Where nothing can ask for a gradient (``torch.no_grad()`` or no input requiring grad) and no dropout
    is due (eval mode or ``dropout == 0``) it is the parent's one-call inference path, bit for bit.  Otherwise it composes the op-site
    Functions: embedding, the temporal then the spatial layers (the layer body :class:`SelfAttentionLayer` runs), output projection;
    every hot path is a HIP kernel and every parameter receives its gradient.  Dropout follows ``self.training``: a training-mode
    call with ``dropout > 0`` draws fresh keep bits on the device (:func:`draw_stae_keep`) unless ``keep=`` supplies them -- int32
    (4 * num_layers, B * in_steps * num_nodes, model_dim / 32) -- and leaves the bits it used in ``self.last_keep``; ``dropout == 0``
    and eval mode ignore ``keep``.  The time-of-day / day-of-week indices are clamped into their tables, and a row's gradient goes
    to the table row the forward read.

    Kept per row and layer until the backward runs: 8 model_dim + feed_forward_dim floats (the layer's input, Q|K|V, the attention
    output, out_proj's output, the first LayerNorm's output, the feed-forward hidden and output) plus num_heads floats of softmax
    statistics, and, with dropout, 2 model_dim / 32 keep words."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.last_keep = None

    def forward(self, x: torch.Tensor, *, keep: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check_x(x)
        drop = self.training and self.dropout > 0
        if not drop and not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))):
            return super().forward(x)
        b, t, n, d = x.shape[0], self.in_steps, self.num_nodes, self.model_dim
        m = b * t * n
        dims = self.dims(b, x.shape[3])
        params = self.param_table()
        ops.stae_check_tables(dims, x.device, params, "STAEformerTrainable")     # raw pointers: device, dtype, shape, layout
        if drop:
            shape = (4 * self.num_layers, m, d // 32)
            if keep is None:
                keep = draw_stae_keep(self.num_layers, m, d, x.device, self.dropout)
            elif keep.dtype != torch.int32 or tuple(keep.shape) != shape or keep.device != x.device:
                raise _lib.RegtError(f"keep must be an int32 {shape} tensor on {x.device}, got {keep.dtype} {tuple(keep.shape)} on {keep.device}")
            self.last_keep = keep
        else:
            keep = None
        rows = STAEEmbedFunction.apply(x.contiguous(), dims, *params[:6])
        eps = float(self.attn_layers_t[0].ln1.eps)
        for i, layer in enumerate(list(self.attn_layers_t) + list(self.attn_layers_s)):
            k1, k2 = (None, None) if keep is None else (keep[2 * i].contiguous(), keep[2 * i + 1].contiguous())
            rows = _stae_layer_rows(rows, layer.table(), b, t, n, self.num_heads, 1 if i < self.num_layers else 2, eps, eps, k1, k2,
                                    self.dropout if drop else 0.0)
        return STAEOutputProjFunction.apply(rows, dims, params[6], params[7])
