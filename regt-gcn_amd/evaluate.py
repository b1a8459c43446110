"""predict.py counterpart: MAE / RMSE / MAPE of a trained checkpoint on the test split.

Metric definitions follow predict.py:141-194: per test snapshot ``|y - out|``, ``(y - out)**2`` and
``|y - out| / percentile_95(y)`` (the snapshot is left out of the MAPE if that ratio is infinite anywhere); the
reported numbers are the means over all snapshots, nodes and horizon steps, RMSE = sqrt(mean squared error),
MAPE in percent.  Also reads the reference's processed 13-tuple pickle (load_dataset.py:436-437, 445-471) when the
authors' file is available.
"""
from __future__ import annotations

import argparse
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import nn as rnn
from .data import snapshot_windows
from .train import REGIONS, split, streamed_split


@torch.no_grad()
def predict_metrics(model, xs: Sequence[torch.Tensor], ys: Sequence[torch.Tensor], graph) -> Tuple[float, float, float]:
    """(MAE, RMSE, MAPE %) over the given snapshots; everything stays on the device until the final three scalars."""
    model.eval()
    ae, se, ape = [], [], []
    for x, y in zip(xs, ys):
        out, _ = model.forward_prepared(x, graph)
        d = (y - out).abs()
        ae.append(d)
        se.append((y - out) ** 2)
        r = d / torch.quantile(y.flatten().double(), 0.95).to(d.dtype)     # np.percentile(q=95): linear interpolation
        if not torch.isinf(r).any():
            ape.append(r)
    mae = float(torch.cat(ae, dim=0).mean())
    rmse = float(torch.cat(se, dim=0).mean().sqrt())
    mape = float(torch.cat(ape, dim=0).mean()) * 100 if ape else float("nan")
    return mae, rmse, mape


@torch.no_grad()
def predict_metrics_batched(model, store, graphs, snap_batch: int) -> Tuple[float, float, float]:
    """predict_metrics() with ``snap_batch`` snapshots per forward (train.WindowStore / train.BatchedGraphs): the same three means --
    the 95th percentile and the infinity rule stay PER SNAPSHOT, as in predict.py:141-194."""
    model.eval()
    ae = torch.zeros((), dtype=torch.float64, device=store.X.device)
    se = torch.zeros_like(ae)
    ape = torch.zeros_like(ae)
    ape_n = torch.zeros_like(ae)
    per = store.Y.shape[1] * store.Y.shape[2]
    for i in range(0, len(store), snap_batch):
        b = min(snap_batch, len(store) - i)
        x, y = store.batch(i, b)
        out, _ = model.forward_prepared(x, graphs.get(b))
        d = (y - out).abs().view(b, per)
        ae += d.sum(dtype=torch.float64)
        se += (d * d).sum(dtype=torch.float64)
        q = torch.quantile(y.view(b, per).double(), 0.95, dim=1, keepdim=True).to(d.dtype)
        r = d / q
        ok = ~torch.isinf(r).any(dim=1)
        ape += r[ok].sum(dtype=torch.float64)
        ape_n += ok.sum() * per
    n = float(store.Y.numel())
    return float(ae) / n, (float(se) / n) ** 0.5, (float(ape) / float(ape_n) * 100 if float(ape_n) else float("nan"))


@torch.no_grad()
def predict_metrics_streamed(model, node_data: torch.Tensor, t_in: int, t_out: int, build_graph, first: int, count: int,
                             step_batch: int = 64) -> Tuple[float, float, float]:
    """predict_metrics() over the ``count`` windows ``first .. first + count - 1`` of ``node_data`` (N, F, steps) as loaded, with every
    raw time step's cell output computed once (serve.window_outputs): about 1 / t_in of the GEMM work, and no WindowStore -- the data
    is held once, not t_in times.  ``build_graph(b)``: the model's graph prepared with ``copies=b``.  RegionalTemporalGCN / TemporalGCN,
    fp32-storage arithmetics."""
    from .serve import window_outputs
    model.eval()
    if first + count + t_in + t_out - 1 > node_data.shape[2]:
        raise ValueError(f"window {first + count - 1} has no {t_out}-step target inside {node_data.shape[2]} time steps")
    ae, se, ape = [], [], []
    for i, out, _ in window_outputs(model, node_data, t_in, build_graph, first, count, step_batch):
        b = out.shape[0]
        y = torch.stack([node_data[:, -1, k + t_in:k + t_in + t_out] for k in range(i, i + b)]).to(out.device, torch.float32)
        d = (y - out).abs()
        ae.append(d.flatten(0, 1))
        se.append(((y - out) ** 2).flatten(0, 1))
        q = torch.quantile(y.flatten(1).double(), 0.95, dim=1).to(d.dtype)         # per snapshot, as predict_metrics
        r = d / q.view(b, 1, 1)
        ok = ~torch.isinf(r).flatten(1).any(dim=1)
        ape.append(r[ok].flatten(0, 1))
    mae = float(torch.cat(ae, dim=0).mean())
    rmse = float(torch.cat(se, dim=0).mean().sqrt())
    ape = torch.cat(ape, dim=0)
    mape = float(ape.mean()) * 100 if ape.numel() else float("nan")
    return mae, rmse, mape


def load_processed_pickle(path: str) -> Dict[str, torch.Tensor]:
    """The reference's ``tpims_data_small.pkl``: a ``torch.save``d 13-tuple (edge_index, edge_attr, 5 x (edge_r_index,
    edge_r_attr), node_data_list) with node_data_list = per-timestep (N, 8) float64 (load_dataset.py:436-437).
    Returns the dict layout of tests/golden/tpims_fixture.npz (node_data as (N, 8, steps) float32)."""
    t = torch.load(path, map_location="cpu", weights_only=False)
    if not (isinstance(t, (tuple, list)) and len(t) == 13):
        raise ValueError("expected the reference's 13-tuple (load_dataset.py:436)")
    out = {"edge_index": t[0].long(), "edge_attr": t[1].float()}
    for i, r in enumerate(REGIONS):
        out[f"edge_{r}_index"] = t[2 + 2 * i].long()
        out[f"edge_{r}_attr"] = t[3 + 2 * i].float()
    out["node_data"] = torch.stack(list(t[12]), dim=1).permute(0, 2, 1).float().contiguous()   # :447
    return out


@torch.no_grad()
def _predict_metrics_windows(model, xs, ys, snap_batch: int, call, stack=lambda x: x.permute(0, 3, 1, 2),
                             pick=lambda out, k, b: out[k:k + 1]):
    """predict.py:173-180 for the models fed (b, T, N, F) windows: the errors are ``batch.y - out`` with out (1, O, N, L_out) and
    y (N, O), broadcast as the reference broadcasts them; MAPE divides by the 95th percentile of the snapshot's y and skips a
    snapshot whose ratio is infinite.  ``stack`` turns the stacked snapshots (b, N, F, T) into the model's input and ``pick(out, k, b)``
    gives snapshot k's prediction (StackedGRU batches and slices differently: predict_metrics_gru)."""
    model.eval()
    ae = se = ape = 0.0
    count = ape_count = 0
    for i in range(0, len(xs), snap_batch):
        x = stack(torch.stack(list(xs[i:i + snap_batch])))                       # (b, T, N, F)
        y = torch.stack(list(ys[i:i + snap_batch]))
        out = call(x)
        for k in range(y.shape[0]):
            err = (y[k] - pick(out, k, y.shape[0])).double()
            ae += float(err.abs().sum())
            se += float((err ** 2).sum())
            count += err.numel()
            ratio = err.abs() / float(np.percentile(y[k].cpu().numpy(), q=95))
            if not torch.isinf(ratio).any():
                ape += float(ratio.sum())
                ape_count += ratio.numel()
    return ae / count, (se / count) ** 0.5, (ape / max(ape_count, 1)) * 100


def predict_metrics_stnorm(model, xs, ys, snap_batch: int = 1):
    """predict.py:173-180 for STNorm: (MAE, RMSE, MAPE).  Snapshots run ``snap_batch`` at a time with per-snapshot TNorm
    (tnorm_group = 1); eval mode reads only the running buffers."""
    return _predict_metrics_windows(model, xs, ys, snap_batch, lambda x: model(x, tnorm_group=1))


def predict_metrics_stid(model, xs, ys, snap_batch: int = 1):
    """predict.py:173-180 for STID: (MAE, RMSE, MAPE); out is (1, O, N, 1)."""
    return _predict_metrics_windows(model, xs, ys, snap_batch, lambda x: model(x))


def predict_metrics_staeformer(model, xs, ys, snap_batch: int = 1):
    """predict.py:173-180 for STAEformer: (MAE, RMSE, MAPE); out is (1, O, N, 1).  The model runs in inference only."""
    return _predict_metrics_windows(model, xs, ys, snap_batch, lambda x: model(x))


def predict_metrics_gru(model, xs, ys, snap_batch: int = 1):
    """predict.py:155-162 for StackedGRU: (MAE, RMSE, MAPE) of ``batch.y - out[:, -1, :]``.  ``snap_batch`` snapshots run as
    stacked batch rows (N, 8 b, T); snapshot k's prediction is its last feature row."""
    def stack(x):                                                                # (b, N, F, T) -> (N, F b, T)
        return x[0] if x.shape[0] == 1 else x.permute(1, 0, 2, 3).reshape(x.shape[1], x.shape[0] * x.shape[2], x.shape[3])

    def pick(out, k, b):                                                         # (N, F b, O) -> snapshot k's (N, O)
        return out.view(out.shape[0], b, -1, out.shape[2])[:, k, -1, :]

    return _predict_metrics_windows(model, xs, ys, snap_batch, lambda x: model(x), stack=stack, pick=pick)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="RegT-GCN evaluation (reference predict.py metrics)")
    ap.add_argument("--fixture", help=".npz in the layout of tests/golden/tpims_fixture.npz")
    ap.add_argument("--pickle", help="the reference's processed tpims_data_small.pkl")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--model", default="RegionalTemporalGCN", choices=["RegionalTemporalGCN", "TemporalGCN", "SpatialGCN", "STNorm", "STID", "StackedGRU", "STAEformer"])   # predict.py:110-114
    ap.add_argument("--num_timesteps_in", default=6, type=int)
    ap.add_argument("--num_timesteps_out", default=1, type=int)
    ap.add_argument("--tr", "--train_ratio", default=0.2, type=float, dest="tr")
    ap.add_argument("--snap_batch", type=int, default=1, help="test snapshots per forward (block-diagonal graph of B copies; same metrics)")
    ap.add_argument("--streamed", action="store_true",
                    help="RegionalTemporalGCN / TemporalGCN: compute every time step's cell output once and form the windows from the cached "
                         "outputs (predict_metrics_streamed; same metrics, about 1 / num_timesteps_in of the GEMM work)")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.streamed:
        from .serve import refuse_streamed
        refuse_streamed(a.model)
    if a.pickle:
        d = load_processed_pickle(a.pickle)
    elif a.fixture:
        z = np.load(a.fixture)
        d = {k: torch.from_numpy(z[k]) for k in z.files if z[k].ndim > 0}
    else:
        raise SystemExit("give --fixture or --pickle")
    dev = torch.device("cuda:0")
    n, f = d["node_data"].shape[:2]
    if a.streamed:                                            # no window is built: the test split is a range of window numbers
        first, count = streamed_split(d["node_data"].shape[2], a.num_timesteps_in, a.num_timesteps_out, a.tr)
        vx = vy = None
    else:
        xs, ys = snapshot_windows(d["node_data"], a.num_timesteps_in, a.num_timesteps_out)
        _, (vx, vy) = split([x.to(dev) for x in xs], [y.to(dev) for y in ys], a.tr)
    if a.model == "STNorm":                                   # predict.py:134-135, 173-180
        model = rnn.STNorm(num_nodes=n, in_dim=f, out_dim=a.num_timesteps_out).to(dev)
        model.load_state_dict(torch.load(a.checkpoint, map_location=dev, weights_only=True))
        mae, rmse, mape = predict_metrics_stnorm(model, vx, vy, max(1, a.snap_batch))
        print("MAE: {:.4f}, RMSE: {:.4f}, MAPE: {:.4f}".format(mae, rmse, mape))
        return
    if a.model == "STID":                                     # predict.py:132-133, 173-180
        model = rnn.STID(num_nodes=n, input_len=a.num_timesteps_in, output_len=a.num_timesteps_out, if_time_in_day=False,
                         if_day_in_week=False).to(dev)
        model.load_state_dict(torch.load(a.checkpoint, map_location=dev, weights_only=True))
        mae, rmse, mape = predict_metrics_stid(model, vx, vy, max(1, a.snap_batch))
        print("MAE: {:.4f}, RMSE: {:.4f}, MAPE: {:.4f}".format(mae, rmse, mape))
        return
    if a.model == "STAEformer":                               # predict.py:130-131, 173-180
        model = rnn.STAEformer(num_nodes=n, in_steps=a.num_timesteps_in, out_steps=a.num_timesteps_out, tod_embedding_dim=0).to(dev)
        model.load_state_dict(torch.load(a.checkpoint, map_location=dev, weights_only=True))
        mae, rmse, mape = predict_metrics_staeformer(model, vx, vy, max(1, a.snap_batch))
        print("MAE: {:.4f}, RMSE: {:.4f}, MAPE: {:.4f}".format(mae, rmse, mape))
        return
    if a.model == "StackedGRU":                               # predict.py:122-123, 155-162
        model = rnn.StackedGRU(in_channels=a.num_timesteps_in, node_features=f, periods=a.num_timesteps_in,
                               output_dim=a.num_timesteps_out).to(dev)
        model.load_state_dict(torch.load(a.checkpoint, map_location=dev, weights_only=True))
        mae, rmse, mape = predict_metrics_gru(model, vx, vy, max(1, a.snap_batch))
        print("MAE: {:.4f}, RMSE: {:.4f}, MAPE: {:.4f}".format(mae, rmse, mape))
        return
    if a.model == "RegionalTemporalGCN":
        model = rnn.RegionalTemporalGCN(f, n, a.num_timesteps_in, a.num_timesteps_out).to(dev)
        graph = model.prepare_graph(d["edge_index"].to(dev), [d[f"edge_{r}_index"].to(dev) for r in REGIONS],
                                    [d[f"edge_{r}_attr"].to(dev) for r in REGIONS])
    elif a.model == "SpatialGCN":
        model = rnn.SpatialGCN(f, a.num_timesteps_in, a.num_timesteps_out).to(dev)
        graph = model.prepare_graph(d["edge_index"].to(dev), d["edge_attr"].to(dev), n)
    else:
        model = rnn.TemporalGCN(f, a.num_timesteps_in, a.num_timesteps_out).to(dev)
        graph = model.prepare_graph(d["edge_index"].to(dev), d["edge_attr"].to(dev), n)
    model.load_state_dict(torch.load(a.checkpoint, map_location=dev, weights_only=True))
    if a.streamed:
        if a.model == "RegionalTemporalGCN":
            idx, att = [d[f"edge_{r}_index"].to(dev) for r in REGIONS], [d[f"edge_{r}_attr"].to(dev) for r in REGIONS]
            build = lambda b: model.prepare_graph(d["edge_index"].to(dev), idx, att, copies=b)      # noqa: E731
        else:
            build = lambda b: model.prepare_graph(d["edge_index"].to(dev), d["edge_attr"].to(dev), n, copies=b)      # noqa: E731
        mae, rmse, mape = predict_metrics_streamed(model, d["node_data"], a.num_timesteps_in, a.num_timesteps_out, build, first, count)
    elif a.snap_batch > 1:
        from .train import BatchedGraphs, WindowStore
        if a.model == "RegionalTemporalGCN":
            idx, att = [d[f"edge_{r}_index"].to(dev) for r in REGIONS], [d[f"edge_{r}_attr"].to(dev) for r in REGIONS]
            graphs = BatchedGraphs(lambda b: model.prepare_graph(d["edge_index"].to(dev), idx, att, copies=b))
        else:
            graphs = BatchedGraphs(lambda b: model.prepare_graph(d["edge_index"].to(dev), d["edge_attr"].to(dev), n, copies=b))
        mae, rmse, mape = predict_metrics_batched(model, WindowStore(vx, vy), graphs, a.snap_batch)
    else:
        mae, rmse, mape = predict_metrics(model, vx, vy, graph)
    print("MAE: {:.4f}, RMSE: {:.4f}, MAPE: {:.4f}".format(mae, rmse, mape))


if __name__ == "__main__":
    main()
