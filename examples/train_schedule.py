#!/usr/bin/env python3
"""A learning-rate schedule and gradient clipping INSIDE the replayed training step, at the reference's own batch size (32 windows):

    optim.FlatSGD(model, lr, momentum=0.9, graph_safe=True, device_lr=True)      a torch.optim.SGD: one launch on the flat buffers, step count and
                                                                                   learning rate on the device (configure_optimizers() returns it for
                                                                                   optimizer = "sgd" with graph_safe_optimizer / device_lr_optimizer set)
    ->  wrappers.GraphedTrainingStep(wrapper, optimizer, batch, max_grad_norm=...) captures zero_grad + training_step + backward + clip_grad_norm_ + step ONCE
    ->  per batch: graphed(batch); scheduler.step()      (torch.optim.lr_scheduler.StepLR -- the replay reads the new rate from the device scalar)

Data are synthetic windows from morphsym_hgnn_amd/synth.py (labels a fixed linear function of the joint features, so the loss falls).  Runs in seconds.
Usage:  python examples/train_schedule.py [--steps 60] [--batch 32] [--momentum 0.9] [--max-grad-norm 1.0]
"""
import argparse
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (build_spec)
from morphsym_hgnn_amd import optim, synth, wrappers  # noqa: E402


def train(steps=60, batch=32, layers=3, lr=1e-2, momentum=0.9, max_grad_norm=1.0, step_size=20, gamma=0.5, quiet=False):
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.set_default_dtype(torch.float64)      # (the reference's convention: fp64 batches; the engine casts them)
    spec = bench.build_spec(layers)
    n_out = spec.out_channels * spec.num_nodes[spec.out_type]
    ei = spec.topology.edge_index_dict(batch, device=dev)
    mix = synth.det_uniform(11, "schedule:mix", (spec.widths["joint"], n_out), -0.05, 0.05).double()

    def make_batch(seed):
        x_dict, _ = synth.make_windows(seed, batch, spec.num_nodes, spec.widths, n_out, classification=False)
        joints = x_dict["joint"].double().reshape(batch, spec.num_nodes["joint"], -1).mean(1)
        return types.SimpleNamespace(x_dict={k: v.to(dev) for k, v in x_dict.items()}, edge_index_dict=ei, y=(joints @ mix).flatten().to(dev), batch_size=batch)

    batches = [make_batch(100 + s) for s in range(8)]
    torch.manual_seed(0)
    cfg = os.path.join(bench.ROOT, "morphsym_hgnn_amd", "cfg", "a1-c2.yaml")
    w = wrappers.HGNN_C2_Lightning_Reg(spec.hidden, layers, spec.topology.metadata(), batches[0], optimizer="sgd", lr=lr, symmetry_mode="MorphSym",
                                       group_operator_path=cfg, grf_body_to_world_frame=False).to(dev)
    # what configure_optimizers() returns for optimizer = "sgd" with wrapper.graph_safe_optimizer = wrapper.device_lr_optimizer = True, plus momentum
    # (the reference's configure_optimizers passes lr only)
    opt = optim.FlatSGD(w.model, lr=lr, momentum=momentum, graph_safe=True, device_lr=True)
    graphed = wrappers.GraphedTrainingStep(w, opt, batches[0], max_grad_norm=max_grad_norm)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=step_size, gamma=gamma)
    log = []
    for step in range(1, steps + 1):
        loss = graphed(batches[step % len(batches)])
        sched.step()
        if step % 10 == 0 or step == 1:
            log.append((step, float(loss), float(graphed.grad_norm), float(opt._lr_dev), opt.param_groups[0]["lr"]))
            if not quiet:
                print(f"step {step:4d}  loss {log[-1][1]:.5f}  grad norm {log[-1][2]:.4f}  lr on the device {log[-1][3]:.3e}  (param group: {log[-1][4]:.3e})")
    torch.cuda.synchronize()
    return log


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60); ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lr", type=float, default=1e-2); ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    a = ap.parse_args()
    train(a.steps, a.batch, lr=a.lr, momentum=a.momentum, max_grad_norm=a.max_grad_norm)
