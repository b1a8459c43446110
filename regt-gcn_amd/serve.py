"""Streaming inference for the models whose cell starts from H = None in every period (RegionalTemporalGCN, TemporalGCN).

The loop body of ``RegionalA3TGCN.forward`` / ``A3TGCN.forward`` is a function of ONE raw time step, the static graph and the weights:

    S_s              = tgcn(X_s, edge_index, edge_weight, h(X_s))            (N, C)
    hidden(window i) = sum_{p < T} softmax(_attention)_p * S_{i+p}
    pred             = head(hidden)

Windows are cut with stride 1, so consecutive windows share T - 1 of their T periods.  :class:`StreamingPredictor` computes every
time step's S once (``model.period_outputs``: one T = 1 forward), keeps the last T of them in a ring and forms each window from the
ring (``ops.window_forward``: one memory-bound pass plus the head).  DESIGN.md section 4b.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib, ops
from .nn import _FusedModel, _need_cuda


STREAMED_MODELS = ("RegionalTemporalGCN", "RandomTemporalGCN", "TemporalGCN")      # the --streamed flag of train.py / evaluate.py
WINDOW_BATCH = 64      # windows per ops.window_forward call of window_outputs


def refuse_streamed(model_name: str) -> None:
    """SystemExit with the reason unless ``--streamed`` covers ``model_name``."""
    if model_name not in STREAMED_MODELS:
        raise SystemExit(f"--streamed covers {' / '.join(STREAMED_MODELS)}: their cell starts from H = None in every period, so a time "
                         f"step's cell output is shared by every window that contains it; {model_name} goes through another entry point")


@torch.no_grad()
def window_outputs(model, node_data: torch.Tensor, t_in: int, build_graph, first: int, count: int, step_batch: int = 64):
    """Yields ``(i, pred (b, N, O), hidden (b, N, C))`` for the ``count`` stride-1 windows ``first .. first + count - 1`` of ``node_data``
    (N, F, steps) as loaded (window i covers steps i .. i + t_in - 1), in batches of at most WINDOW_BATCH windows starting at window i.
    Every raw time step's cell output is computed once -- ``step_batch`` steps per ``period_outputs`` call on ``build_graph(b)``, the
    model's graph prepared with ``copies=b`` --, written straight into a timeline of WINDOW_BATCH + t_in - 1 slabs (N, C) that
    ``ops.window_forward`` reads; the next batch keeps the last t_in - 1 slabs and computes only its own new steps, so the memory does
    not grow with ``count``."""
    if t_in != int(model.tgnn.periods):
        raise ValueError(f"the model was built for {model.tgnn.periods} periods, got t_in={t_in}")
    if count < 1 or first < 0 or first + count + t_in - 1 > node_data.shape[2] or step_batch < 1:
        raise ValueError(f"windows {first} .. {first + count - 1} of {t_in} steps do not fit {node_data.shape[2]} time steps (step_batch={step_batch})")
    dev = model.linear1.weight.device
    n, c = node_data.shape[0], int(model.tgnn.out_channels)
    timeline = torch.empty(min(count, WINDOW_BATCH) + t_in - 1, n, c, dtype=torch.float32, device=dev)
    graphs = {}
    have = 0                                   # slabs at the front of the timeline that the batch at hand inherits
    for i in range(0, count, WINDOW_BATCH):
        b = min(WINDOW_BATCH, count - i)
        need = b + t_in - 1                    # the batch's windows read steps first + i .. first + i + need - 1
        for a in range(have, need, step_batch):
            k = min(step_batch, need - a)
            if k not in graphs:
                graphs[k] = build_graph(k)
            x = node_data[:, :, first + i + a:first + i + a + k].permute(2, 0, 1).to(dev, torch.float32).contiguous()
            model.period_outputs(x, graphs[k], out=timeline[a:a + k])
        pred, hidden = ops.window_forward(timeline[:need], 0, b, model.tgnn._attention, model.linear1.weight, model.linear1.bias,
                                          model.linear2.weight, model.linear2.bias)
        yield first + i, pred, hidden
        have = t_in - 1
        if i + b < count and have:
            timeline[:have].copy_(timeline[b:b + have].clone() if b < have else timeline[b:b + have])


class StreamingPredictor:
    """``push`` one raw time step ``x_t`` (N, F) at a time; once T steps are in, every push returns the model's ``(pred (N, O), hidden
    (N, C))`` for the window that ends at this step -- what ``model.forward_prepared`` returns for the stacked (N, F, T) window, at the
    cost of one period.  ``graph``: the model's prepared graph (``model.prepare_graph``, one copy).

    The ring (T, N, C) holds the cell outputs of the last T steps, step s in slot s % T.  They are only valid for the weights they were
    computed with: a push after any parameter changed (another ``data_ptr`` or ``_version`` than at the oldest cached step) raises
    :class:`RegtError`; call :meth:`reset` and feed the last T steps again."""

    def __init__(self, model, graph):
        if not isinstance(model, _FusedModel):
            raise TypeError("StreamingPredictor serves RegionalTemporalGCN / TemporalGCN (the models whose cell starts from H = None in "
                            f"every period), got {type(model).__name__}")
        self.model, self.graph = model, graph
        self.periods = int(model.tgnn.periods)
        self._ring: Optional[torch.Tensor] = None
        self._seen = 0
        self._weights = None

    @property
    def steps_seen(self) -> int:
        """Time steps pushed since construction or the last :meth:`reset`."""
        return self._seen

    def reset(self) -> None:
        """Forget every cached step (after a weight update, a gap in the feed, another graph)."""
        self._seen = 0
        self._weights = None

    def _weights_now(self):
        return tuple((p.data_ptr(), p._version) for p in self.model._params_in_order())

    @torch.no_grad()
    def push(self, x_t: torch.Tensor) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        _need_cuda(x_t)
        if x_t.dim() != 2 or x_t.dtype != torch.float32:
            raise ValueError(f"x_t must be float32 (N, F), got {x_t.dtype} {tuple(x_t.shape)}")
        now = self._weights_now()
        if self._seen == 0:
            self._weights = now
        elif now != self._weights:
            raise _lib.RegtError("StreamingPredictor: a model parameter changed since the oldest cached time step was computed; the ring "
                                 "would mix outputs of two sets of weights -- call reset() and push the last T steps again")
        t, shape = self.periods, (x_t.shape[0], int(self.model.tgnn.out_channels))
        if self._ring is None or tuple(self._ring.shape[1:]) != shape or self._ring.device != x_t.device:
            if self._seen:
                raise ValueError(f"x_t has {x_t.shape[0]} nodes on {x_t.device}, the cached steps {self._ring.shape[1]} on {self._ring.device}")
            self._ring = torch.empty(t, *shape, dtype=torch.float32, device=x_t.device)
        slot = self._seen % t                  # the library writes the step's cell output straight into its slab
        self.model.period_outputs(x_t.unsqueeze(0), self.graph, out=self._ring[slot:slot + 1])
        self._seen += 1
        if self._seen < t:
            return None
        m = self.model
        pred, hidden = ops.window_forward(self._ring, self._seen % t, 1, m.tgnn._attention, m.linear1.weight, m.linear1.bias,
                                          m.linear2.weight, m.linear2.bias)
        return pred[0], hidden[0]
