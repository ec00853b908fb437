#!/usr/bin/env python3
"""Training on a robust regression loss without leaving the fused step: A1-C2 on a resident sequence, L1 or Huber instead of the reference's MSE.

    wrapper.set_regression_loss("huber", delta)      ("mse" | "l1" | "huber": torch.nn.MSELoss / L1Loss / HuberLoss(delta), mean reduction)
    ->  SequenceStore.batch (window indices; the encoder gathers them from the resident series)
    ->  HGNN_C2_Lightning_Reg.training_step(batch)   the one-call series step: decoder, the chosen loss and the decoder's backward in the tail of the fused
                                                     kernel; returns that loss, logs it as "train_loss" next to MSE_loss / RMSE_loss / L1_loss, which stay
                                                     the metric kernel's values
    ->  loss.backward(); optimizer.step()            (optim.FlatAdam from configure_optimizers())

The labels of the synthetic sequence (examples/train_flat.py: GRFs are a fixed linear function of the joint torques) get impact spikes -- every `--spike-every`
rows one foot's GRF jumps by `--spike` -- which is what the robust losses are for: with --loss mse the spikes pull the fit, with l1 / huber the MSE on the
spike-free rows ends lower.  Prints MSE_loss, L1_loss and the training loss per epoch.
Usage:  python examples/train_robust.py [--loss huber] [--delta 0.5] [--epochs 5] [--steps 40] [--batch 4096] [--dtype bf16]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (build_spec)
from examples.train_flat import synthetic_sequence  # noqa: E402
from morphsym_hgnn_amd import wrappers  # noqa: E402
from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe  # noqa: E402


def spiky_sequence(rows, spike, spike_every, seed=0):
    """examples/train_flat.py's sequence with impact spikes on its labels: every `spike_every` rows one label column jumps by +-`spike`."""
    seq = synthetic_sequence(rows, seed=seed)
    if spike_every > 0:
        rng = np.random.default_rng(seed + 17)
        at = np.arange(spike_every // 2, rows, spike_every)
        seq["F"] = seq["F"].copy()      # the GRF labels, [rows, 12]
        seq["F"][at, rng.integers(0, seq["F"].shape[1], at.size)] += spike * rng.choice([-1.0, 1.0], at.size)
    return seq


def train(loss="huber", delta=0.5, epochs=5, steps=40, batch=4096, dtype="bf16", layers=3, lr=1e-3, rows=60_000, spike=8.0, spike_every=97, quiet=False):
    dev = torch.device("cuda", torch.cuda.current_device())
    spec = bench.build_spec(layers)
    store = SequenceStore(spiky_sequence(rows, spike, spike_every), quadsdk_a1_c2_recipe(range(12), range(4), 150, 3), dtype=dtype, device=dev)
    ei = spec.topology.edge_index_dict(batch, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1234)

    def next_batch():
        return store.batch(torch.randint(0, len(store), (batch,), generator=gen, device=dev), ei)

    os.environ["MSHGNN_DTYPE"] = dtype
    torch.manual_seed(0)
    cfg = os.path.join(bench.ROOT, "morphsym_hgnn_amd", "cfg", "a1-c2.yaml")
    first = next_batch()
    dummy = types.SimpleNamespace(edge_index_dict=ei, x_dict={t: x[:, :store.recipe.width(t)].float().contiguous() for t, x in first.x_dict.items()})
    w = wrappers.HGNN_C2_Lightning_Reg(spec.hidden, layers, spec.topology.metadata(), dummy, optimizer="adam", lr=lr, symmetry_mode="MorphSym",
                                       group_operator_path=cfg, grf_body_to_world_frame=False).to(dev)
    w.set_regression_loss(loss, delta)      # the model's fused engines and the wrapper's `loss`; "mse": everything as without this line
    opt = w.configure_optimizers()
    log = []
    for epoch in range(1, epochs + 1):
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
        for step in range(steps):
            l = w.training_step(next_batch(), step)
            opt.zero_grad(set_to_none=True)
            l.backward()
            opt.step()
            sums += torch.stack([w.logged["train_MSE_loss"].double(), w.logged["train_L1_loss"].double(), l.detach().double().reshape(())])
        mse, l1, tr = (sums / steps).tolist()      # (one read-back per epoch)
        log.append((epoch, mse, l1, tr))
        if not quiet:
            print(f"epoch {epoch:3d}  MSE_loss {mse:.5f}  L1_loss {l1:.5f}  training loss ({loss}{f', delta {delta}' if loss == 'huber' else ''}) {tr:.5f}")
    torch.cuda.synchronize()
    return log


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss", default="huber", choices=["mse", "l1", "huber"]); ap.add_argument("--delta", type=float, default=0.5)
    ap.add_argument("--epochs", type=int, default=5); ap.add_argument("--steps", type=int, default=40); ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16", "x3"]); ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--spike", type=float, default=8.0); ap.add_argument("--spike-every", type=int, default=97)
    a = ap.parse_args()
    train(a.loss, a.delta, a.epochs, a.steps, a.batch, a.dtype, lr=a.lr, spike=a.spike, spike_every=a.spike_every)
