#!/usr/bin/env python3
"""Training on a dataset of several sequences, as the reference's scripts do (research/train_regression-grf_msgn.py:57-93):

    ResidentDataset(sequences)            every sequence's series resident on the GPU, concatenated row-wise: ONE SequenceStore
    train, val = dataset.split(0.85)      per sequence: the first 85 % of its windows (without the last one) / the rest -- ConcatDataset of Subsets
    for indices in train.epoch(32, gen):  one device randperm per epoch, minibatches of 32 windows shuffled across ALL sequences, no host round trip
        HGNN_C2_Lightning_Reg.training_step(train.batch(indices, edges))   dataset indices -> start rows on the device (mshgnn_dataset_starts),
                                                                            then the fused step straight from the resident series
    evaluate_sequence(model, val, ...)    a validation sweep over the view, predictions in dataset-index order

Data are synthetic (examples/train_flat.py's sequences, three of different lengths: GRFs are a fixed linear function of the joint torques).
Usage:  python examples/train_dataset.py [--epochs 2] [--batch 32] [--rows 700 1300 2900] [--dtype bf16] [--normalize]
"""
import argparse
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (build_spec)
from examples.train_flat import synthetic_sequence  # noqa: E402
from morphsym_hgnn_amd import wrappers  # noqa: E402
from morphsym_hgnn_amd.windows import ResidentDataset, quadsdk_a1_c2_recipe  # noqa: E402


def train(epochs=2, batch=32, rows=(700, 1300, 2900), dtype="bf16", layers=3, lr=1e-3, normalize=False, quiet=False):
    dev = torch.device("cuda", torch.cuda.current_device())
    spec = bench.build_spec(layers)
    recipe = quadsdk_a1_c2_recipe(range(12), range(4), 150, 3, normalize=normalize)
    dataset = ResidentDataset([synthetic_sequence(n, seed=s) for s, n in enumerate(rows)], recipe, dtype=dtype, device=dev)
    train_view, val_view = dataset.split(0.85)
    if not quiet:
        print(f"{len(rows)} sequences of {list(rows)} rows: {len(dataset)} windows, {len(train_view)} to train on, {len(val_view)} to validate on")
    edges = {}
    edges_for = lambda B: edges.setdefault(B, spec.topology.edge_index_dict(B, device=dev))
    os.environ["MSHGNN_DTYPE"] = dtype
    torch.manual_seed(0)
    cfg = os.path.join(bench.ROOT, "morphsym_hgnn_amd", "cfg", "a1-c2.yaml")
    # the lazy-initialising dummy forward (gnnLightning.py:593-595) sees the reference's feature widths (900 / 450 / 1), not the aligned pitch
    first = train_view.batch([0, 1], edges_for(2))
    dummy = types.SimpleNamespace(edge_index_dict=edges_for(2), x_dict={t: x[:, :recipe.width(t)].float().contiguous() for t, x in first.x_dict.items()})
    model = wrappers.HGNN_C2_Lightning_Reg(spec.hidden, layers, spec.topology.metadata(), dummy, optimizer="adam", lr=lr,
                                           symmetry_mode="MorphSym", group_operator_path=cfg, grf_body_to_world_frame=False).to(dev)
    opt = model.configure_optimizers()
    gen = torch.Generator(device=dev).manual_seed(1234)
    history = []
    for epoch in range(epochs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        steps = 0
        for step, indices in enumerate(train_view.epoch(batch, gen, drop_last=True)):      # (one batch size: one set of window buffers)
            loss = model.training_step(train_view.batch(indices, edges_for(batch)), step)   # Lightning's order: training_step, zero_grad, backward, step
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            steps += 1
        torch.cuda.synchronize(); dt = time.perf_counter() - t0      # (the epoch's end has read the views' out-of-range flag once)
        train_mse = float(model.logged["train_MSE_loss"].detach())
        pred = wrappers.evaluate_sequence(model, val_view, edges_for(1), 256)
        val_mse = float(model.logged["test_MSE_loss"].detach())
        history.append((epoch, train_mse, val_mse))
        if not quiet:
            print(f"epoch {epoch}: {steps} steps of {batch} windows in {dt:.2f} s ({dt / max(steps, 1) * 1e3:.3f} ms/step), last train mse {train_mse:.5f}, "
                  f"validation mse {val_mse:.5f} over {pred.shape[0]} windows")
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=2); ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rows", type=int, nargs="+", default=[700, 1300, 2900]); ap.add_argument("--dtype", default="bf16", choices=["bf16", "x3"])
    ap.add_argument("--layers", type=int, default=3); ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--normalize", action="store_true", help="standardise every run over its window (the reference's normalize=True)")
    a = ap.parse_args()
    train(a.epochs, a.batch, tuple(a.rows), a.dtype, a.layers, a.lr, a.normalize)
