#!/usr/bin/env python3
"""The MLP baseline (the reference's `--model_type mlp`, gnnLightning.py:363-413) trained straight from a resident dataset:

    ResidentDataset(sequences, quadsdk_a1_mlp_recipe(...))   one node type holding one node: a window row is get_helper_mlp's input
    MLP_Lightning(in = history x 42, hidden, out = 4, ...)   models.MLP at the default precision ("x3", the split-bf16 parity plan): the fused engine (engine.MLPEngine)
    GraphedTrainingStep(model, opt, batch, index_source=train)   index mapping + the fused series step + FlatAdam captured once, replayed per batch
    evaluate_table(model, val.orbit view, {})                the evaluators' table (one row per symmetry operator, one column per sequence)

Data are synthetic (examples/train_flat.py's sequences: the GRFs are a fixed linear function of the joint torques).
Usage:  python examples/train_mlp.py [--epochs 3] [--batch 64] [--rows 700 1300] [--history 150] [--layers 8] [--eager]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.train_flat import synthetic_sequence  # noqa: E402
from morphsym_hgnn_amd import wrappers  # noqa: E402
from morphsym_hgnn_amd.windows import GroupAction, ResidentDataset, quadsdk_a1_mlp_recipe  # noqa: E402


def train(epochs=3, batch=64, rows=(700, 1300), history=150, hidden=128, layers=8, lr=1e-3, graphed=True, quiet=False):
    dev = torch.device("cuda", torch.cuda.current_device())
    recipe = quadsdk_a1_mlp_recipe(range(12), range(4), history, 1)
    dataset = ResidentDataset([synthetic_sequence(n, seed=s) for s, n in enumerate(rows)], recipe, dtype="bf16", device=dev)
    train_view, val_view = dataset.split(0.85)
    torch.manual_seed(0)
    model = wrappers.MLP_Lightning(recipe.width("mlp"), hidden, 4, layers, batch, optimizer="adam", lr=lr, regression=True).to(dev)
    # (the default precision "x3" runs the fused split-bf16 step at 1e-4 of fp64; model.model.set_precision("bf16") trades that for the bf16 step's speed)
    model.graph_safe_optimizer = graphed
    opt = model.configure_optimizers()
    gen = torch.Generator(device=dev).manual_seed(1234)
    step_fn = None
    history_log = []
    for epoch in range(epochs):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        steps = 0
        for indices in train_view.epoch(batch, gen, drop_last=True):
            if graphed:
                if step_fn is None:
                    step_fn = wrappers.GraphedTrainingStep(model, opt, train_view.batch(indices, {}), index_source=train_view)
                step_fn(indices)
            else:
                loss = model.training_step(train_view.batch(indices, {}), steps)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
            steps += 1
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        train_mse = float(model.logged["train_MSE_loss"].detach())
        pred = wrappers.evaluate_sequence(model, val_view, {}, 256)
        val_mse = float(model.logged["test_MSE_loss"].detach())
        history_log.append((epoch, train_mse, val_mse))
        if not quiet:
            print(f"epoch {epoch}: {steps} steps of {batch} windows in {dt:.2f} s ({dt / max(steps, 1) * 1e3:.3f} ms/step), last train mse {train_mse:.5f}, "
                  f"validation mse {val_mse:.5f} over {pred.shape[0]} windows")
    # the augmented baseline's table: every validation window under the identity and gs / gt / gr, per sequence
    orbit = dataset.orbit(GroupAction.load("a1-c2"))
    table = wrappers.evaluate_table(model, orbit.view(), {}, 256)
    if not quiet:
        ops = ["e" if op in (None, "None") else str(op) for op in table.operators]
        for name, t in table.table.items():
            print(f"{name}: " + "; ".join(f"{op}: " + ", ".join(f"{float(v):.4f}" for v in row) for op, row in zip(ops, t)))
    return history_log, table


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3); ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rows", type=int, nargs="+", default=[700, 1300]); ap.add_argument("--history", type=int, default=150)
    ap.add_argument("--hidden", type=int, default=128); ap.add_argument("--layers", type=int, default=8); ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--eager", action="store_true", help="no HIP graph: training_step / backward / optimizer.step by hand")
    a = ap.parse_args()
    train(a.epochs, a.batch, tuple(a.rows), a.history, a.hidden, a.layers, a.lr, not a.eager)
