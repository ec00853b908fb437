"""Symmetry augmentation: train the non-equivariant MI-HGNN on an ORBIT view -- every minibatch mixes the identity and the gs / gt / gr copies of its windows,
the reference's `ConcatDataset([ds, ds_gs, ds_gt, ds_gr])` under a shuffling DataLoader -- from one resident copy of the series, then sweep the whole orbit of
the validation windows with `evaluate_sequence` and print the loss per group element.

    python examples/train_augmented.py [--plan bf16|x3] [--steps 20] [--batch 256] [--rows 2000]

Synthetic A1 series stand in for recorded sequences."""
import argparse
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morphsym_hgnn_amd import topology, wrappers                                                   # noqa: E402
from morphsym_hgnn_amd.windows import GroupAction, ResidentDataset, quadsdk_a1_c2_recipe          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", default="bf16", choices=["bf16", "x3"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rows", type=int, default=2000)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    seqs = [{"imu_acc": f(n, 3), "imu_omega": f(n, 3), "q": f(n, 12), "qd": f(n, 12), "tau": f(n, 12), "F": f(n, 12), "r_o": f(n, 4)} for n in (a.rows, a.rows // 2)]
    topo, group = topology.TOPOLOGIES["a1-c2"](), GroupAction.load("a1-c2")
    recipe = quadsdk_a1_c2_recipe(list(range(12)), list(range(4)), 150, 3)
    orbit = ResidentDataset(seqs, recipe, dtype=a.plan).orbit(group)      # K = 4 elements per window, no second copy of the data
    train, val = orbit.split(0.85)                                        # windows are split, not (element, window) pairs
    xs, _, _ = orbit.assemble([0, 1])
    dummy = types.SimpleNamespace(edge_index_dict=topo.edge_index_dict(2, device=dev),
                                  x_dict={t: x[:, :recipe.width(t)].float().contiguous() for t, x in zip(recipe.node_types, xs)})
    os.environ["MSHGNN_DTYPE"] = a.plan
    w = wrappers.HGNN_C2_Lightning_Reg(128, 3, topo.metadata(), dummy, symmetry_mode=None, group_operator_path=None).to(dev)      # the plain MI-HGNN baseline
    opt = w.configure_optimizers()
    edges = topo.edge_index_dict(a.batch, device=dev)
    step = 0
    while step < a.steps:
        for ix in train.epoch(a.batch, drop_last=True):                   # a shuffled epoch over the orbit view: augmented training
            opt.zero_grad(set_to_none=True)
            loss = w.training_step(train.batch(ix, edges), step)          # one fused step: the encoder gathers each window under its own element
            loss.backward()
            opt.step()
            step += 1
            if step % 5 == 0 or step == a.steps:
                print(f"step {step}: loss {float(loss):.6g}")
            if step >= a.steps:
                break
    pred = wrappers.evaluate_sequence(w, val, topo.edge_index_dict(1, device=dev), a.batch)      # an ordered sweep: the K prediction blocks of the orbit
    n = val.n_windows
    y = torch.cat([orbit.assemble(val.starts(list(range(e * n, (e + 1) * n))))[1] for e in range(orbit.n_elements)])
    for e, op in enumerate(orbit.operators):
        blk = slice(e * n, (e + 1) * n)
        print(f"  {op or 'identity'}: validation MSE {float(((pred[blk].reshape(n, -1) - y[blk]) ** 2).mean()):.6g} over {n} windows")


if __name__ == "__main__":
    main()
