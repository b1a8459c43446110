"""run.py counterpart: the reference's training / evaluation loop semantics around the HIP hot path.

Kept from the reference (run.py:163-243):
* train(): one forward + ``mean((out - y)**2)`` + ``backward()`` per snapshot, gradients ACCUMULATE over all
  train snapshots, ``optimizer.step()`` + ``zero_grad()`` ONCE per epoch, returns the LAST snapshot's loss;
* test(): ``(sqrt(mean(se)), mean(se))`` over all test snapshots (the reference prints the second as "MAE");
* RMSprop(lr, weight_decay) (run.py:145); ``range(epochs + 1)`` epochs; state_dict saved every 10 epochs
  as ``model_in{T}_out{O}_epoch{k}.pt`` (run.py:242-243).
Changed on purpose: snapshots and the static graph live on the GPU for the whole run (the reference copies
every batch host->device and syncs on ``.cpu()`` every step, run.py:172,180), and the graph is prepared once.

    python -m regtgcn_amd.train --model RegionalTemporalGCN --num_timesteps_in 6 --num_timesteps_out 1 \
        --tr 0.2 --epochs 5 --fixture tests/golden/tpims_fixture.npz
"""
from __future__ import annotations

import argparse
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import functional as F_
from . import nn as rnn
from .data import snapshot_windows
from .dist import HaloPipeline, Shard, allreduce_gradients, allreduce_sum

REGIONS = ("IA", "KS", "KY", "OH", "WI")


def train_epoch(model, xs: Sequence[torch.Tensor], ys: Sequence[torch.Tensor], graph, optimizer, stepper=None) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """One epoch of run.py::train() on device-resident snapshots; returns (last loss, all losses) as device scalars.
    ``stepper`` (functional.FusedTrainStep): the same steps without autograd -- for graphs so small that the host work
    per step is the bound."""
    model.train()
    losses = []
    if stepper is not None:
        for x, y in zip(xs, ys):
            losses.append(stepper(x, y).clone())
        allreduce_gradients(list(model.parameters()))
        optimizer.step()
        stepper.zero_grad()
        return losses[-1][0], [l[0] for l in losses]
    # (the gradients of the epoch's snapshots add up in .grad, run.py:178-194: the model's backward does that addition itself, one
    # multi-tensor add instead of one autograd add per parameter -- functional.set_grad_accumulation_in_backward)
    with F_.grad_accumulation_in_backward():
        for x, y in zip(xs, ys):
            out, _ = model.forward_prepared(x, graph)
            loss = F_.mse_loss(out, y)               # torch.mean((out - y) ** 2), run.py:180, value and gradient in one kernel
            loss.backward()
            losses.append(loss.detach())
    allreduce_gradients(list(model.parameters()))
    optimizer.step()
    optimizer.zero_grad()
    return losses[-1], losses


@torch.no_grad()
def evaluate(model, xs, ys, graph) -> Tuple[float, float]:
    """run.py::test(): (rmse, mse)."""
    model.eval()
    se = [(model.forward_prepared(x, graph)[0] - y) ** 2 for x, y in zip(xs, ys)]
    m = torch.cat(se, dim=0).mean()
    return float(m.sqrt()), float(m)


# ---- snapshot batching ---------------------------------------------------------------------------------------------------------------
# run.py:170-192 runs one forward / backward per snapshot and ADDS the gradients of all train snapshots; the test loop (:208-216)
# averages squared errors over all test snapshots.  Both are additive over snapshots, and the graph is the same in every one of
# them, so B snapshots can run as ONE problem on the block-diagonal graph of B copies (graph.replicate_edges): M = B*N*T rows per
# launch instead of N*T.  At TPIMS size (N = 104) a per-snapshot step is ~40 dependent launches of 5-25 us -- latency, not work;
# batching turns the same launches into work.  Gradients = the same sum (another summation order), per-snapshot losses are
# still reported, the optimiser still steps once per epoch.

class WindowStore:
    """All sliding windows of a run, device-resident and stacked: X (S, N, F, T), Y (S, N, O) -- load_dataset.py:451-457 -- so that a
    batch of B consecutive snapshots is a VIEW (B*N, F, T) of X, no per-step copy."""

    def __init__(self, xs: Sequence[torch.Tensor], ys: Sequence[torch.Tensor]):
        self.X = torch.stack(list(xs)).contiguous() if len(xs) else torch.empty(0)
        self.Y = torch.stack(list(ys)).contiguous() if len(ys) else torch.empty(0)

    def __len__(self):
        return self.X.shape[0]

    def batches(self, snap_batch: int):
        """(first snapshot i, count b) of every batch of ``snap_batch`` consecutive snapshots; the last one may be shorter."""
        for i in range(0, len(self), snap_batch):
            yield i, min(snap_batch, len(self) - i)

    def batch(self, i: int, b: int):
        x, y = self.X[i:i + b], self.Y[i:i + b]
        return x.reshape(-1, x.shape[2], x.shape[3]), y.reshape(-1, y.shape[2])


class BatchedGraphs:
    """prepare_graph(copies=b) per batch size b in use (the epoch's last batch may be shorter), built on first use."""

    def __init__(self, build):
        self._build, self._by_size = build, {}

    def get(self, b: int):
        if b not in self._by_size:
            self._by_size[b] = self._build(b)
        return self._by_size[b]


def train_epoch_batched(model, store: WindowStore, graphs: BatchedGraphs, optimizer, snap_batch: int) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """train_epoch() with ``snap_batch`` snapshots per forward / backward; returns (last snapshot's loss, all per-snapshot losses)."""
    model.train()
    losses = []
    n_o = store.Y.shape[1] * store.Y.shape[2]                 # entries of ONE snapshot: the divisor of run.py:180's mean
    with F_.grad_accumulation_in_backward():
        for i, b in store.batches(snap_batch):
            x, y = store.batch(i, b)
            out, _ = model.forward_prepared(x, graphs.get(b))
            F_.mse_loss(out, y, n_o).backward()               # = the sum of the b snapshot means: gradients add up as in run.py
            losses.append(((out.detach() - y) ** 2).view(b, -1).mean(dim=1))
    allreduce_gradients(list(model.parameters()))
    optimizer.step()
    optimizer.zero_grad()
    all_l = torch.cat(losses)
    return all_l[-1], list(all_l.unbind(0))


@torch.no_grad()
def evaluate_batched(model, store: WindowStore, graphs: BatchedGraphs, snap_batch: int) -> Tuple[float, float]:
    """run.py::test() with ``snap_batch`` snapshots per forward: (rmse, mse)."""
    model.eval()
    se = torch.zeros((), dtype=torch.float64, device=store.X.device)
    for i, b in store.batches(snap_batch):
        x, y = store.batch(i, b)
        se += ((model.forward_prepared(x, graphs.get(b))[0] - y) ** 2).sum(dtype=torch.float64)
    m = float(se) / float(store.Y.numel())
    return m ** 0.5, m


def train_epoch_sharded(model, xs: Sequence[torch.Tensor], ys: Sequence[torch.Tensor], shard: Shard, pipe: HaloPipeline,
                        optimizer, global_nodes: int, group=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """train_epoch() for one region shard of a multi-GPU run: ``xs[i]`` (n_local, F, T) / ``ys[i]`` (n_local, O) are this
    rank's rows of snapshot i.  The loss is the mean over the GLOBAL graph (run.py:180), so the per-rank partial sums are
    scaled by 1/(global_nodes*O) before backward and the gradients of all ranks add up to the single-GPU gradient (one
    flat all-reduce before the optimiser step).  Halo rows of snapshot i+1 travel while snapshot i computes.
    Returns (last global loss, all global losses) as device tensors."""
    model.train()
    losses = []
    if len(xs):
        pipe.submit(0, xs[0])
    with F_.grad_accumulation_in_backward():
        for i, (x, y) in enumerate(zip(xs, ys)):
            buf = pipe.acquire(i % 2)
            if i + 1 < len(xs):
                pipe.submit((i + 1) % 2, xs[i + 1])
            out, _ = model.forward_packed(buf, shard.graph)
            loss = F_.mse_loss(out, y, global_nodes * y.shape[1])
            loss.backward()
            pipe.release(i % 2)
            losses.append(loss.detach())
    allreduce_gradients(list(model.parameters()), group)
    tot = allreduce_sum(torch.stack(losses), group)
    optimizer.step()
    optimizer.zero_grad()
    return tot[-1], tot


@torch.no_grad()
def evaluate_sharded(model, xs, ys, shard: Shard, pipe: HaloPipeline, global_nodes: int, group=None) -> Tuple[float, float]:
    """run.py::test() over region shards: (rmse, mse) of the global graph."""
    model.eval()
    se = torch.zeros((), dtype=torch.float32, device=xs[0].device)
    pipe.submit(0, xs[0])
    for i, (x, y) in enumerate(zip(xs, ys)):
        buf = pipe.acquire(i % 2)
        if i + 1 < len(xs):
            pipe.submit((i + 1) % 2, xs[i + 1])
        se += ((model.forward_packed(buf, shard.graph)[0] - y) ** 2).sum()
        pipe.release(i % 2)
    m = allreduce_sum(se, group) / float(global_nodes * ys[0].shape[1] * len(xs))
    return float(m.sqrt()), float(m)


@torch.no_grad()
def evaluate_streamed(model, node_data: torch.Tensor, t_in: int, t_out: int, build_graph, first: int, count: int,
                      step_batch: int = 64) -> Tuple[float, float]:
    """run.py::test() over the windows ``first .. first + count - 1`` of ``node_data`` (N, F, steps) as loaded: the (rmse, mse) of
    evaluate(), with every raw time step's cell output computed once and shared by the t_in windows that contain it
    (serve.window_outputs).  ``build_graph(b)``: the model's graph prepared with ``copies=b``.  RegionalTemporalGCN / TemporalGCN."""
    from .serve import window_outputs
    model.eval()
    if first + count + t_in + t_out - 1 > node_data.shape[2]:
        raise ValueError(f"window {first + count - 1} has no {t_out}-step target inside {node_data.shape[2]} time steps")
    se = []
    for i, out, _ in window_outputs(model, node_data, t_in, build_graph, first, count, step_batch):
        y = torch.stack([node_data[:, -1, k + t_in:k + t_in + t_out] for k in range(i, i + out.shape[0])]).to(out.device, torch.float32)
        se.append(((out - y) ** 2).flatten(0, 1))
    m = torch.cat(se, dim=0).mean()
    return float(m.sqrt()), float(m)


def refuse_streamed_train(a) -> None:
    """SystemExit with the reason unless ``--streamed_train`` covers the run the flags describe."""
    from .serve import STREAMED_MODELS
    if a.model not in STREAMED_MODELS:
        raise SystemExit(f"--streamed_train covers {' / '.join(STREAMED_MODELS)}: their cell starts from H = None in every period, so a time "
                         f"step's cell forward and backward are shared by every window that contains it; {a.model} trains window by window")
    if a.fused_step:
        raise SystemExit("--streamed_train and --fused_step are alternatives: the streamed epoch runs no per-window step that "
                         "FusedTrainStep could replace")
    if a.snap_batch > 1:
        raise SystemExit("--streamed_train and --snap_batch are alternatives: the streamed epoch batches raw time steps, not windows")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--streamed_train runs on one GPU: the region-sharded forward_packed path is out of its scope")


def train_epoch_streamed(model, node_data: torch.Tensor, t_in: int, t_out: int, build_graph, first: int, count: int, optimizer,
                         step_batch: int = 64) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """train_epoch() over the ``count`` stride-1 windows ``first .. first + count - 1`` of ``node_data`` (N, F, steps) as loaded, with
    every raw time step's cell forward AND backward run once: the weights are fixed until the epoch's single optimizer
    step, the epoch's gradient is a sum over windows, and that sum factors through the per-step cell outputs S_s.  Returns (last
    window's loss, all per-window losses), as train_epoch_batched.  ``build_graph(b)``: the model's graph prepared with ``copies=b``.

    Per batch of at most serve.WINDOW_BATCH windows, on two timelines S and dS of WINDOW_BATCH + t_in - 1 slabs (N, C): the batch's new
    S slabs (period_outputs), the window sum and head (ops.window_forward), the loss gradient with one window's N * O as divisor,
    ops.window_backward accumulating into dS and into ``.grad`` of ``tgnn._attention`` and the head; the steps whose dS is now complete
    (no later window contains them) go through model.period_gradients, always in the same groups of ``step_batch`` consecutive steps
    counted from the epoch's first one -- a group that straddles two batches waits in a staging buffer of ``step_batch`` slabs --, so
    the cell and embedding gradients are the same bits whatever WINDOW_BATCH is; then the last t_in - 1 slabs of both timelines move
    to the front.  The memory does not grow with ``count``.  RegionalTemporalGCN / TemporalGCN, fp32-storage arithmetics."""
    from . import ops, serve
    if t_in != int(model.tgnn.periods):
        raise ValueError(f"the model was built for {model.tgnn.periods} periods, got t_in={t_in}")
    if count < 1 or first < 0 or step_batch < 1 or first + count + t_in + t_out - 1 > node_data.shape[2]:
        raise ValueError(f"windows {first} .. {first + count - 1} of {t_in} steps and their {t_out}-step targets do not fit "
                         f"{node_data.shape[2]} time steps (step_batch={step_batch})")
    if t_in > ops.window_backward_max_t():
        raise ValueError(f"streamed training covers t_in <= {ops.window_backward_max_t()} (the window backward's limit), got {t_in}")
    model.train()
    att, l1, l2 = model.tgnn._attention, model.linear1, model.linear2
    direct = [att, l1.weight, l1.bias, l2.weight, l2.bias]        # the parameters ops.window_backward accumulates into
    dev = l1.weight.device
    for p in direct:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    n, c, o = node_data.shape[0], int(model.tgnn.out_channels), l2.weight.shape[0]
    wb = serve.WINDOW_BATCH
    slabs = min(count, wb) + t_in - 1
    s_line = torch.empty(slabs, n, c, dtype=torch.float32, device=dev)
    ds_line = torch.zeros(slabs, n, c, dtype=torch.float32, device=dev)
    stage = torch.empty(step_batch, n, c, dtype=torch.float32, device=dev)      # dS of the steps waiting for their group to fill
    graphs, losses = {}, []

    def graph_of(k):
        if k not in graphs:
            graphs[k] = build_graph(k)
        return graphs[k]

    def steps(a, k):                                   # raw time steps a .. a + k - 1 as (k, N, F)
        return node_data[:, :, a:a + k].permute(2, 0, 1).to(dev, torch.float32).contiguous()

    staged = 0                                         # slabs in `stage`; they are steps done - staged .. done - 1
    done = first                                       # the first step whose dS has not been handed on yet
    have = 0                                           # slabs at the front of both timelines that the batch at hand inherits
    for i in range(0, count, wb):
        b = min(wb, count - i)
        need = b + t_in - 1                            # the batch's windows read steps first + i .. first + i + need - 1
        for a in range(have, need, step_batch):
            k = min(step_batch, need - a)
            model.period_outputs(steps(first + i + a, k), graph_of(k), out=s_line[a:a + k])
        pred, hidden = ops.window_forward(s_line[:need], 0, b, att, l1.weight, l1.bias, l2.weight, l2.bias)
        y = torch.stack([node_data[:, -1, k + t_in:k + t_in + t_out] for k in range(first + i, first + i + b)]).to(dev, torch.float32)
        _, dpred = ops.mse_loss_grad(pred, y.contiguous(), n * o)        # the sum of the b window means: gradients add up as in run.py
        losses.append(((pred - y) ** 2).view(b, -1).mean(dim=1))
        ops.window_backward(s_line[:need], 0, b, att, l1.weight, l1.bias, l2.weight, l2.bias, hidden, dpred, ds_line[:need], True,
                            att.grad, l1.weight.grad, l1.bias.grad, l2.weight.grad, l2.bias.grad)
        last = i + b == count
        complete = need if last else b                 # no later window contains the batch's first b steps
        a = 0
        while a < complete:
            k = min(step_batch - staged, complete - a)
            stage[staged:staged + k].copy_(ds_line[a:a + k])
            staged, a, done = staged + k, a + k, done + k
            if staged == step_batch or (last and a == complete):
                model.period_gradients(steps(done - staged, staged), graph_of(staged), stage[:staged])
                staged = 0
        have = t_in - 1
        if not last:
            if have:
                for line in (s_line, ds_line):
                    line[:have].copy_(line[b:b + have].clone() if b < have else line[b:b + have])
            ds_line[have:].zero_()
    allreduce_gradients(list(model.parameters()))
    optimizer.step()
    optimizer.zero_grad()
    all_l = torch.cat(losses)
    return all_l[-1], list(all_l.unbind(0))


def streamed_split(steps: int, t_in: int, t_out: int, ratio: float) -> Tuple[int, int]:
    """(first window, window count) of the test split that split() cuts from snapshot_windows()' list, from the step count alone."""
    windows = max(steps - (t_in + t_out) + 1, 0)
    k = int(ratio * windows)
    return k, windows - k


def split(xs, ys, ratio: float):
    k = int(ratio * len(xs))          # temporal_signal_split: first int(ratio*n) snapshots train, rest test
    return (xs[:k], ys[:k]), (xs[k:], ys[k:])


# models of run.py:115-136: those built on the TGCN cell (the hot path and the SURVEY 8(f) baselines), SpatialGCN (two ChebConv
# layers, run.py:117-118), STNorm (gated dilated convolutions with temporal / spatial normalisation, no graph, run.py:135-136) and
# STID (a per-node MLP on the node's history and a learned node embedding, no graph, run.py:133-134) and StackedGRU (two GRU layers
# whose sequence runs over the nodes, no graph, run.py:123-124); TemporalGConvLSTM (which run.py:122 cannot construct) is out of scope.  STAEformer
# (run.py:131-132) trains through its own command, ``python -m regtgcn_amd.train_staeformer`` (nn.STAEformerTrainable,
# train_epoch_staeformer below), and is evaluated with evaluate.py --model STAEformer; this tuple and --model stay as they are
MODELS = ("RegionalTemporalGCN", "RandomTemporalGCN", "TemporalGCN", "ConvStackedTemporalGCN", "GraphSAGETemporalGCN", "GAT", "GATTemporal",
          "SpatialGCN", "STNorm", "STID", "StackedGRU")


# ---- STNorm and STID (run.py:181-186, 217-222) ------------------------------------------------------------------------------------------
# run.py feeds both batch.x.permute(2, 0, 1).unsqueeze(0) -- (1, T, N, F) -- and takes mean((out - y)**2) with out (1, O, N, L_out)
# (L_out = 1 for STID) and y (N, O): for O > 1 that broadcasts to (1, O, N, O), kept as it is.  test() compares out[0][0] (N, L_out)
# with y (N, O).  A batch of B snapshots runs as one (B, T, N, F) call.  STNorm takes tnorm_group = 1: TNorm's statistics and
# running-buffer updates stay per snapshot, in snapshot order, so the losses, the accumulated gradients and the buffers are those of
# B sequential run.py steps.  STID has no batch statistics: the batch is just B independent snapshots.  The window view below is
# strided; both modules make it contiguous once.

def stnorm_batch(store: "WindowStore", i: int, b: int):
    """Snapshots i .. i+b-1 as STNorm's / STID's input (b, T, N, F) and their targets (b, N, O)."""
    return store.X[i:i + b].permute(0, 3, 1, 2), store.Y[i:i + b]


def _train_epoch_windows(model, store: "WindowStore", optimizer, snap_batch: int, batch, losses_of) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """run.py::train() for the models without a graph: gradients accumulate over the epoch, one optimizer step at its end; returns
    (last snapshot's loss, all per-snapshot losses).  ``batch(store, i, b)`` gives snapshots i .. i+b-1 as the model's input and
    their targets, ``losses_of(x, y, i, b)`` runs the model on them and returns the b per-snapshot losses."""
    model.train()
    losses = []
    with F_.grad_accumulation_in_backward():
        for i, b in store.batches(snap_batch):
            per = losses_of(*batch(store, i, b), i, b)
            per.sum().backward()
            losses.append(per.detach())
    optimizer.step()
    optimizer.zero_grad()
    all_l = torch.cat(losses)
    return all_l[-1], list(all_l.unbind(0))


@torch.no_grad()
def _evaluate_windows(model, store: "WindowStore", snap_batch: int, batch, errors_of) -> Tuple[float, float]:
    """run.py::test() for the same models: (rmse, mse) over all snapshots; ``errors_of(x, y, i, b)`` runs the model on a batch
    and returns prediction - target for every entry run.py compares."""
    model.eval()
    se = torch.zeros((), dtype=torch.float64, device=store.X.device)
    count = 0
    for i, b in store.batches(snap_batch):
        e = errors_of(*batch(store, i, b), i, b) ** 2
        se += e.sum(dtype=torch.float64)
        count += e.numel()
    m = float(se) / float(max(count, 1))
    return m ** 0.5, m


def _window_losses(out: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return ((out - y.unsqueeze(1)) ** 2).mean(dim=(1, 2, 3))              # run.py:184 / :186 per snapshot


def train_epoch_stnorm(model, store: "WindowStore", optimizer, snap_batch: int) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """run.py::train() for STNorm; returns (last snapshot's loss, all per-snapshot losses)."""
    return _train_epoch_windows(model, store, optimizer, snap_batch, stnorm_batch,
                                lambda x, y, i, b: _window_losses(model(x, tnorm_group=1), y))


def evaluate_stnorm(model, store: "WindowStore", snap_batch: int) -> Tuple[float, float]:
    """run.py::test() for STNorm: (rmse, mse) of out[0][0] against y."""
    return _evaluate_windows(model, store, snap_batch, stnorm_batch, lambda x, y, i, b: model(x, tnorm_group=1)[:, 0] - y)


def train_epoch_stid(model, store: "WindowStore", optimizer, snap_batch: int,
                     keeps: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """run.py::train() for STID; returns (last snapshot's loss, all per-snapshot losses).  ``keeps``: the dropout keep bits of all
    snapshots, int32 (num_layer, len(store), N, hidden / 32), instead of a fresh draw per call."""
    return _train_epoch_windows(model, store, optimizer, snap_batch, stnorm_batch, lambda x, y, i, b: _window_losses(
        model(x, keep=None if keeps is None else keeps[:, i:i + b].contiguous()), y))


def evaluate_stid(model, store: "WindowStore", snap_batch: int) -> Tuple[float, float]:
    """run.py::test() for STID: (rmse, mse) of out[0][0] (N, 1) against y (N, O)."""
    return _evaluate_windows(model, store, snap_batch, stnorm_batch, lambda x, y, i, b: model(x)[:, 0] - y)


# ---- StackedGRU (run.py:174-176, 210-212) --------------------------------------------------------------------------------------------
# run.py feeds batch.x (N, F = 8, T) as it is: nn.GRU is sequence-first, so the sequence runs over the nodes and the F features are
# independent batch rows; the loss reads the last row only, mean((out[:, -1, :] - y)**2) with y (N, O).  B snapshots run as one call
# on (N, F B, T): rows F j .. F j + F - 1 are snapshot j's, its loss reads row F j + F - 1.  One snapshot is a view of the store;
# B > 1 gathers the rows once.

def gru_batch(store: "WindowStore", i: int, b: int):
    """Snapshots i .. i+b-1 as StackedGRU's input (N, F b, T) and their targets (b, N, O)."""
    x = store.X[i:i + b]
    x = x[0] if b == 1 else x.permute(1, 0, 2, 3).reshape(x.shape[1], b * x.shape[2], x.shape[3])
    return x, store.Y[i:i + b]


def _gru_last_rows(out: torch.Tensor, b: int) -> torch.Tensor:
    """out (N, F b, O) -> the last feature row of every snapshot, (b, N, O)."""
    n, fb, o = out.shape
    return out.view(n, b, fb // b, o)[:, :, -1, :].permute(1, 0, 2)


def train_epoch_gru(model, store: "WindowStore", optimizer, snap_batch: int) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """run.py::train() for StackedGRU: gradients accumulate over the epoch, one optimizer step at its end; returns (last snapshot's
    loss, all per-snapshot losses)."""
    return _train_epoch_windows(model, store, optimizer, snap_batch, gru_batch,                # (run.py:176 per snapshot)
                                lambda x, y, i, b: ((_gru_last_rows(model(x), b) - y) ** 2).mean(dim=(1, 2)))


def evaluate_gru(model, store: "WindowStore", snap_batch: int) -> Tuple[float, float]:
    """run.py::test() for StackedGRU: (rmse, mse) of out[:, -1, :] against y."""
    return _evaluate_windows(model, store, snap_batch, gru_batch, lambda x, y, i, b: _gru_last_rows(model(x), b) - y)


# ---- STAEformer (run.py:131-132, 181-186, 217-222) ---------------------------------------------------------------------------------------
# run.py feeds it what it feeds STNorm and STID, (1, T, N, F), and takes the same loss and metric; out is (1, O, N, output_dim = 1).  A
# batch of B snapshots is B independent rows of one call.  Its own command is ``python -m regtgcn_amd.train_staeformer``.

def staeformer_batch(store: "WindowStore", i: int, b: int):
    """Snapshots i .. i+b-1 as STAEformer's input (b, T, N, F) and their targets (b, N, O)."""
    return stnorm_batch(store, i, b)


def train_epoch_staeformer(model, store: "WindowStore", optimizer, snap_batch: int,
                           keeps: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """run.py::train() for nn.STAEformerTrainable; returns (last snapshot's loss, all per-snapshot losses).  ``keeps``: the dropout keep
    bits of all snapshots, int32 (4 num_layers, len(store), T N, model_dim / 32), instead of a fresh draw per call."""
    def losses_of(x, y, i, b):
        keep = None if keeps is None else keeps[:, i:i + b].reshape(keeps.shape[0], -1, keeps.shape[-1])
        return _window_losses(model(x, keep=keep), y)
    return _train_epoch_windows(model, store, optimizer, snap_batch, staeformer_batch, losses_of)


def evaluate_staeformer(model, store: "WindowStore", snap_batch: int) -> Tuple[float, float]:
    """run.py::test() for STAEformer: (rmse, mse) of out[0][0] (N, output_dim) against y (N, O)."""
    return _evaluate_windows(model, store, snap_batch, staeformer_batch, lambda x, y, i, b: model(x)[:, 0] - y)


def add_flags(ap: argparse.ArgumentParser, only: Optional[Sequence[str]] = None) -> argparse.ArgumentParser:
    """run.py's flags and this package's own, added to ``ap``; ``only``: the flags (by their first name) a command takes, the others
    are left out.  One statement of every flag's names, default and help for train.py and train_staeformer.py."""
    def add(*names, **kw):
        if only is None or names[0] in only:
            ap.add_argument(*names, **kw)
    add("--seed", default=42, type=int)
    add("--epochs", default=30, type=int)
    add("--lr", default=1e-3, type=float)
    add("--decay", default=1e-4, type=float)
    add("--momentum", default=0.9, type=float, help="accepted, unused (as in run.py)")
    add("--bs", "--batch_size", default=32, type=int, dest="bs", help="accepted, unused (as in run.py)")
    add("--tr", "--train_ratio", default=0.8, type=float, dest="tr")
    add("--tf", "--train_feature", default="available", type=str, dest="tf", help="occrate / available: the target column (run.py:31)")
    add("--edge_cut", default=None, type=str, help="dataloading_type 1 only in run.py; accepted, unused")
    add("--dataset_path", default=None, type=str, help="the reference's dataset/ directory (= --dataset_root)")
    add("--checkpoint_path", default="../checkpoints/", type=str, help="accepted, unused (as in run.py)")
    add("--dataloading_type", default=2, type=int, help="2 (TruckParkingDataset2 semantics) is what this loader implements")
    add("--decomp_type", default=None, type=str, help="regional: the five state link files; random: run.py's random decomposition "
                                                                  "(load_dataset.py:324-329) of the full graph into five overlapping parts")
    add("--num_timesteps_in", default=8, type=int)
    add("--num_timesteps_out", default=4, type=int)
    add("--model", default="TemporalGCN", choices=list(MODELS))
    add("--is_preprocessed", action="store_true", help="accepted: the data source decides (a .pkl / .npz is preprocessed by definition)")
    add("--is_pretrained", action="store_true")
    add("--pretrained_model", default="")
    add("--pretrained_model_epoch", default="0")
    add("--logs", action="store_true", help="also write the epoch lines to ./logs/<date>.txt (run.py:48-49)")
    # this package's own flags
    add("--fixture", help=".npz with node_data (N,F,steps), edge_index, edge_attr, edge_<R>_index/attr")
    add("--dataset_root", help="the reference's dataset/ directory (read through regtgcn_amd.etl)")
    add("--max_steps", type=int, default=None, help="with --dataset_root: use the first MAX_STEPS timesteps")
    add("--out_dir", default="pretrained")
    add("--loss_digits", default=4, type=int, help="decimals of the printed epoch line (run.py prints 4)")
    add("--fused_step", action="store_true", help="train through functional.FusedTrainStep (no autograd; faster on small graphs)")
    add("--snap_batch", type=int, default=1,
                    help="snapshots per forward / backward (block-diagonal graph of B copies; same accumulated gradients and metrics, "
                         "run.py:170-192 / 208-216 are additive over snapshots).  1 = one launch sequence per snapshot, as run.py")
    add("--streamed", action="store_true",
        help="RegionalTemporalGCN / RandomTemporalGCN / TemporalGCN: the per-epoch test pass computes every time step's cell output once "
             "and forms the windows from the cached outputs (evaluate_streamed; same metrics)")
    add("--streamed_train", action="store_true",
        help="RegionalTemporalGCN / RandomTemporalGCN / TemporalGCN: the training pass, too, runs every time step's cell forward and backward "
             "once per epoch (train_epoch_streamed; same accumulated gradients and losses); implies --streamed for the test pass")
    return ap


def build_parser() -> argparse.ArgumentParser:
    """run.py's flag set (run.py:22-45) -- the reference's own launch lines parse unchanged, e.g. scripts/RegionalTemporalGCN.sh:1 --
    plus this package's data-source flags.  Flags run.py parses and never reads (--momentum, --bs, --checkpoint_path: RMSprop is
    built from lr / decay only, run.py:145; snapshots are not batched, run.py:170) are accepted and ignored here too."""
    return add_flags(argparse.ArgumentParser(description="RegT-GCN training loop (reference run.py flags)"))


def random_decomposition(edge_index: torch.Tensor, edge_attr: torch.Tensor, parts: int = 5, seed: int = 42):
    """run.py --decomp_type random.  The reference reads five files links/0322/link{1..5}_data.csv there (load_dataset.py:324-329)
    that its repository does not ship; what they hold is a split of the full graph's edges into five parts that ignores the
    states.  Here the five parts are drawn (seeded) from the full edge list, so a node may receive edges in several of them --
    the "overlapping" layout of graph.prepare_graph, the general form of the regional embedding."""
    g = torch.Generator().manual_seed(seed)
    e = edge_index.shape[1]
    idx, att = [], []
    for _ in range(parts):
        pick = torch.randperm(e, generator=g)[: max(1, e // parts)]
        idx.append(edge_index[:, pick].contiguous())
        att.append(edge_attr[pick].contiguous())
    return idx, att


def load_windows(a, dev):
    """The data source the flags name -> (its arrays, N, F, (train xs, ys), (test xs, ys)), windows on ``dev`` (run.py:60-75)."""
    if a.dataloading_type != 2:
        raise SystemExit("--dataloading_type 2 (TruckParkingDataset2: full graph + five regional graphs) is the loader this package implements")
    root = a.dataset_root or (a.dataset_path if a.dataset_path and os.path.isdir(os.path.join(a.dataset_path, "nodes")) else None)
    if root:
        from . import etl
        d = {k: v.numpy() for k, v in etl.load_tpims(root, a.max_steps, train_feature=a.tf).as_dict().items()}
    elif a.fixture:
        d = np.load(a.fixture)
        if a.tf.lower() != "occrate":
            print("note: a fixture's target column is fixed when it is built (tests/golden/tpims_fixture.npz: OCCRATE); --tf is not applied")
    else:
        raise SystemExit("give --fixture, --dataset_root or a --dataset_path that holds the reference's dataset/ directory")
    node_data = torch.from_numpy(d["node_data"])
    n, f = node_data.shape[:2]
    if getattr(a, "streamed_train", False):
        return d, n, f, ([], []), ([], [])      # both passes read node_data as loaded (train_epoch_streamed, evaluate_streamed)
    if getattr(a, "streamed", False):
        # the test pass reads node_data as loaded (evaluate_streamed): only the train split's windows are built and moved
        k, _ = streamed_split(node_data.shape[2], a.num_timesteps_in, a.num_timesteps_out, a.tr)
        xs, ys = snapshot_windows(node_data[:, :, :k + a.num_timesteps_in + a.num_timesteps_out - 1] if k else node_data[:, :, :0],
                                  a.num_timesteps_in, a.num_timesteps_out)
        return d, n, f, ([x.to(dev) for x in xs], [y.to(dev) for y in ys]), ([], [])
    xs, ys = snapshot_windows(node_data, a.num_timesteps_in, a.num_timesteps_out)
    xs, ys = [x.to(dev) for x in xs], [y.to(dev) for y in ys]
    return d, n, f, *split(xs, ys, a.tr)


def make_optimizer(model, a):
    return torch.optim.RMSprop(model.parameters(), lr=a.lr, weight_decay=a.decay)          # run.py:145


def open_outputs(a, model_name: str):
    """(checkpoint directory pretrained/<tf>/<model>/ of run.py:138, 243, the --logs file or None)."""
    out_dir = os.path.join(a.out_dir, a.tf, model_name)
    os.makedirs(out_dir, exist_ok=True)
    log = None
    if a.logs:
        import datetime
        os.makedirs("logs", exist_ok=True)
        log = open(os.path.join("logs", datetime.datetime.now().strftime("%y-%m-%d_%H-%M") + ".txt"), "a")
    return out_dir, log


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.streamed_train:
        refuse_streamed_train(a)
        a.streamed = True                                     # the test pass streams as well
    if a.streamed:
        from .serve import refuse_streamed
        refuse_streamed(a.model)
    torch.manual_seed(a.seed)
    dev = torch.device("cuda:0")
    d, n, f, (tx, ty), (vx, vy) = load_windows(a, dev)
    ei = torch.from_numpy(d["edge_index"]).to(dev)
    ea = torch.from_numpy(d["edge_attr"]).to(dev)
    if a.model in ("RegionalTemporalGCN", "RandomTemporalGCN"):             # run.py:115-116: one class for both decompositions
        model = rnn.RegionalTemporalGCN(f, n, a.num_timesteps_in, a.num_timesteps_out).to(dev)
        if (a.decomp_type or "regional").lower() == "random":
            r_idx, r_att = random_decomposition(ei, ea, len(REGIONS), a.seed)
        else:
            r_idx = [torch.from_numpy(d[f"edge_{r}_index"]).to(dev) for r in REGIONS]
            r_att = [torch.from_numpy(d[f"edge_{r}_attr"]).to(dev) for r in REGIONS]
        graph = model.prepare_graph(ei, r_idx, r_att)
    elif a.model == "TemporalGCN":
        model = rnn.TemporalGCN(f, a.num_timesteps_in, a.num_timesteps_out).to(dev)
        graph = model.prepare_graph(ei, ea, n)
    elif a.model == "ConvStackedTemporalGCN":                               # run.py:125-126
        model = rnn.ConvStackedTemporalGCN(f, a.num_timesteps_in, a.num_timesteps_out).to(dev)
        graph = model.prepare_graph(ei, ea, n)
    elif a.model == "SpatialGCN":                                           # run.py:117-118
        model = rnn.SpatialGCN(f, a.num_timesteps_in, a.num_timesteps_out).to(dev)
        graph = model.prepare_graph(ei, ea, n)
    elif a.model == "STNorm":                                               # run.py:135-136 (in_dim = F of the data)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("STNorm runs on one GPU: SNorm normalises over all nodes in every layer, and sharding the nodes would "
                             "need one all-reduce per layer")
        if a.fused_step:
            raise SystemExit("--fused_step covers RegionalTemporalGCN (regional decomposition) / TemporalGCN")
        model = rnn.STNorm(num_nodes=n, in_dim=f, out_dim=a.num_timesteps_out).to(dev)
        graph = None
    elif a.model == "STID":                                                 # run.py:133-134 (input_dim = 3, the module's default)
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("STID runs on one GPU (it has no graph to shard; its kernels take all nodes in one launch)")
        if a.fused_step:
            raise SystemExit("--fused_step covers RegionalTemporalGCN (regional decomposition) / TemporalGCN")
        model = rnn.STID(num_nodes=n, input_len=a.num_timesteps_in, output_len=a.num_timesteps_out, if_time_in_day=False,
                         if_day_in_week=False).to(dev)
        graph = None
    elif a.model == "StackedGRU":                                           # run.py:123-124
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("StackedGRU runs on one GPU (its sequence runs over all nodes: there is nothing to shard)")
        if a.fused_step:
            raise SystemExit("--fused_step covers RegionalTemporalGCN (regional decomposition) / TemporalGCN")
        model = rnn.StackedGRU(in_channels=a.num_timesteps_in, node_features=f, periods=a.num_timesteps_in,
                               output_dim=a.num_timesteps_out).to(dev)
        graph = None
    elif a.model == "GraphSAGETemporalGCN":                                 # run.py:127-128
        model = rnn.GraphSAGETemporalGCN(f, n, a.num_timesteps_in, a.num_timesteps_out).to(dev)
        graph = model.prepare_graph(ei, n)
    else:                                                                   # 'GAT' in run.py:129-130 (class GATTemporal)
        model = rnn.GATTemporal(f, n, a.num_timesteps_in, a.num_timesteps_out).to(dev)
        graph = model.prepare_graph(ei, n)
    if a.is_pretrained:
        model.load_state_dict(torch.load(a.pretrained_model, map_location=dev, weights_only=True))
    opt = make_optimizer(model, a)
    out_dir, log = open_outputs(a, a.model)
    batched = None
    if a.model in ("STNorm", "STID", "StackedGRU"):
        from_store = (WindowStore(tx, ty), WindowStore(vx, vy))
        train_fn, eval_fn = {"STNorm": (train_epoch_stnorm, evaluate_stnorm), "STID": (train_epoch_stid, evaluate_stid),
                             "StackedGRU": (train_epoch_gru, evaluate_gru)}[a.model]
        for epoch in range(a.epochs + 1):
            last, _ = train_fn(model, from_store[0], opt, max(1, a.snap_batch))
            rmse, mse = eval_fn(model, from_store[1], max(1, a.snap_batch))
            _report(a, log, out_dir, model, epoch, last, rmse, mse)
        return
    if a.snap_batch > 1:
        if a.fused_step:
            raise SystemExit("--snap_batch and --fused_step are alternatives (both remove per-snapshot host work)")
        # every operator of these models is local to a node's in-neighbours (gcn_norm, ChebConv.__norm__, SAGE mean, GAT softmax), so
        # B disjoint copies of the graph are B independent snapshots
        if a.model in ("TemporalGCN", "ConvStackedTemporalGCN", "SpatialGCN"):
            graphs = BatchedGraphs(lambda b: model.prepare_graph(ei, ea, n, copies=b))
        elif a.model in ("GraphSAGETemporalGCN", "GAT", "GATTemporal"):
            graphs = BatchedGraphs(lambda b: model.prepare_graph(ei, n, copies=b))
        else:
            graphs = BatchedGraphs(lambda b: model.prepare_graph(ei, r_idx, r_att, copies=b))
        batched = (WindowStore(tx, ty), WindowStore(vx, vy), graphs)
    stepper = None
    if a.fused_step:
        if a.model not in ("RegionalTemporalGCN", "RandomTemporalGCN", "TemporalGCN") or getattr(graph, "overlap", False):
            raise SystemExit("--fused_step covers RegionalTemporalGCN (regional decomposition) / TemporalGCN")
        from .functional import FusedTrainStep
        stepper = FusedTrainStep(model, graph, f, a.num_timesteps_in)
    streamed = None
    if a.streamed:                                            # the test pass only: test windows len(tx) .. of the data as loaded
        if a.model == "TemporalGCN":
            s_graphs = BatchedGraphs(lambda b: model.prepare_graph(ei, ea, n, copies=b))
        else:
            s_graphs = BatchedGraphs(lambda b: model.prepare_graph(ei, r_idx, r_att, copies=b))
        nd = torch.from_numpy(np.asarray(d["node_data"]))
        streamed = (nd, s_graphs.get, *streamed_split(nd.shape[2], a.num_timesteps_in, a.num_timesteps_out, a.tr))
    for epoch in range(a.epochs + 1):
        if a.streamed_train:                                  # the train split: windows 0 .. k - 1 of the data as loaded
            last, _ = train_epoch_streamed(model, streamed[0], a.num_timesteps_in, a.num_timesteps_out, streamed[1], 0, streamed[2], opt)
        elif batched:
            last, _ = train_epoch_batched(model, batched[0], batched[2], opt, a.snap_batch)
        else:
            last, _ = train_epoch(model, tx, ty, graph, opt, stepper)
        if streamed:
            rmse, mse = evaluate_streamed(model, streamed[0], a.num_timesteps_in, a.num_timesteps_out, streamed[1], streamed[2], streamed[3])
        elif batched:
            rmse, mse = evaluate_batched(model, batched[1], batched[2], a.snap_batch)
        else:
            rmse, mse = evaluate(model, vx, vy, graph)
        _report(a, log, out_dir, model, epoch, last, rmse, mse)


def _report(a, log, out_dir, model, epoch, last, rmse, mse):
    line = "Train Loss: {:.{d}f}, Test RMSE: {:.{d}f}, MAE: {:.{d}f}".format(float(last), rmse, mse, d=a.loss_digits)   # run.py:236 format
    print(line)
    if log:
        log.write(line + "\n")
        log.flush()
    if epoch % 10 == 0:
        torch.save(model.state_dict(), os.path.join(out_dir, "model_in{}_out{}_epoch{}.pt".format(
            a.num_timesteps_in, a.num_timesteps_out, int(a.pretrained_model_epoch) + epoch)))


if __name__ == "__main__":
    main()
