"""Training loop for STAEformer (run.py --model STAEformer, run.py:131-132):

    python -m regtgcn_amd.train_staeformer --fixture tests/golden/tpims_fixture.npz --num_timesteps_in 6 --num_timesteps_out 1 --epochs 30

It constructs ``nn.STAEformerTrainable(num_nodes=N, in_steps, out_steps, tod_embedding_dim=0)`` as run.py:132 does (model_dim 128,
4 heads of 32, dropout 0.1) and takes train.py's flags where they apply; the data source, the split, the optimizer, the epoch line
and the checkpoint names are train.py's own.  A checkpoint written here loads into ``python -m regtgcn_amd.evaluate --model
STAEformer``.  One GPU: attention along the node axis reads every node in every spatial layer.
"""
from __future__ import annotations

import argparse
import os

import torch

from . import nn as rnn
from . import train as T

MODEL = "STAEformer"
# train.py's flags that apply to a model without a graph, a region decomposition or a fused step
FLAGS = ("--seed", "--epochs", "--lr", "--decay", "--tr", "--tf", "--dataset_path", "--dataloading_type", "--num_timesteps_in",
         "--num_timesteps_out", "--is_pretrained", "--pretrained_model", "--pretrained_model_epoch", "--logs", "--fixture", "--dataset_root",
         "--max_steps", "--out_dir", "--loss_digits", "--snap_batch")


def build_parser() -> argparse.ArgumentParser:
    """train.add_flags' own definitions of FLAGS (names, aliases, defaults, help), nothing restated."""
    return T.add_flags(argparse.ArgumentParser(description="STAEformer training loop (reference run.py flags, --model STAEformer)"), FLAGS)


def main(argv=None):
    a = build_parser().parse_args(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("STAEformer runs on one GPU: its spatial layers attend over all nodes, and sharding the nodes would need an "
                         "all-gather per layer")
    torch.manual_seed(a.seed)
    dev = torch.device("cuda:0")
    _, n, _, (tx, ty), (vx, vy) = T.load_windows(a, dev)
    model = rnn.STAEformerTrainable(num_nodes=n, in_steps=a.num_timesteps_in, out_steps=a.num_timesteps_out, tod_embedding_dim=0).to(dev)
    if a.is_pretrained:
        model.load_state_dict(torch.load(a.pretrained_model, map_location=dev, weights_only=True))
    opt = T.make_optimizer(model, a)
    out_dir, log = T.open_outputs(a, MODEL)
    train_store, test_store = T.WindowStore(tx, ty), T.WindowStore(vx, vy)
    for epoch in range(a.epochs + 1):
        last, _ = T.train_epoch_staeformer(model, train_store, opt, max(1, a.snap_batch))
        rmse, mse = T.evaluate_staeformer(model, test_store, max(1, a.snap_batch))
        T._report(a, log, out_dir, model, epoch, last, rmse, mse)


if __name__ == "__main__":
    main()
