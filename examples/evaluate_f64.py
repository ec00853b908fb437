"""Evaluate a checkpoint at the reference's own precision: load an fp64 state dict into a model at precision "f64", sweep a sequence, and print how far
the default split-bf16 plan ("x3") is from it.

    python examples/evaluate_f64.py [--checkpoint state_dict.pt] [--rows 1200] [--batch 256]

The reference trains and stores its parameters in float64 (torch.set_default_dtype(torch.float64), gnnLightning.py:1183).  `set_precision("f64")` makes
the model's parameters fp64 BEFORE the state dict is loaded, so every bit of the checkpoint is kept, and runs every Linear / GraphConv on the fp64 MFMA
operators (csrc/mshgnn_ops.hip).  Without --checkpoint a synthetic fp64 state dict in the reference's layout (the model's own parameter names,
values that are not fp32 numbers) stands in.  Synthetic A1 series stand in for a recorded sequence."""
import argparse
import copy
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morphsym_hgnn_amd import topology, wrappers                                   # noqa: E402
from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None, help="a torch-saved state dict of the model (or a Lightning checkpoint: its 'state_dict', 'model.' prefixes stripped)")
    ap.add_argument("--rows", type=int, default=1200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--history", type=int, default=150)
    ap.add_argument("--layers", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    seq = {"imu_acc": f(a.rows, 3), "imu_omega": f(a.rows, 3), "q": f(a.rows, 12), "qd": f(a.rows, 12), "tau": f(a.rows, 12), "F": f(a.rows, 12), "r_o": f(a.rows, 4)}
    topo = topology.TOPOLOGIES["a1-c2"]()
    recipe = quadsdk_a1_c2_recipe(list(range(12)), list(range(4)), a.history, 3)
    store = SequenceStore(seq, recipe, dtype="x3")      # fp32 series: the "x3" plan gathers them, the "f64" model widens the assembled windows
    xs, _, _ = store.assemble([0, 1])
    dummy = types.SimpleNamespace(edge_index_dict=topo.edge_index_dict(2, device=dev),
                                  x_dict={t: x[:, :recipe.width(t)].float().contiguous() for t, x in zip(recipe.node_types, xs)})
    torch.manual_seed(0)
    w64 = wrappers.HGNN_C2_Lightning_Reg(128, a.layers, topo.metadata(), dummy, symmetry_mode=None)
    w64.model.set_precision("f64")      # fp64 parameters from here on: load_state_dict below narrows nothing
    if a.checkpoint:
        sd = torch.load(a.checkpoint, map_location="cpu")
        sd = sd.get("state_dict", sd)
        sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in sd.items()}
    else:
        g = torch.Generator().manual_seed(1)
        sd = {k: v.detach().double() * (1.0 + 1e-3 * torch.randn(v.shape, generator=g, dtype=torch.float64)) for k, v in w64.model.state_dict().items()}
    w64.model.load_state_dict(sd)
    assert all(torch.equal(p.detach(), sd[k].double()) for k, p in w64.model.named_parameters()), "a parameter was narrowed"
    wx3 = copy.deepcopy(w64)
    wx3.model.set_precision("x3")       # the same parameters, rounded to fp32 once, on the default plan
    w64, wx3 = w64.to(dev), wx3.to(dev)
    ei1 = topo.edge_index_dict(1, device=dev)
    p64 = wrappers.evaluate_sequence(w64, store, ei1, a.batch)
    px3 = wrappers.evaluate_sequence(wx3, store, ei1, a.batch)
    torch.cuda.synchronize()
    diff = (px3.double() - p64).abs().max()
    print(f"{p64.shape[0]} windows of {a.history} steps; predictions {tuple(p64.shape)} in {p64.dtype}")
    print(f"largest |x3 - f64| over all predictions: {float(diff):.3e}  ({float(diff / p64.abs().max()):.3e} of the largest prediction)")
    for name, w in (("f64", w64), ("x3", wx3)):
        print(f"  {name}: " + ", ".join(f"{k} {float(v):.9g}" for k, v in sorted(w.logged.items()) if k.startswith("test_") and v is not None))


if __name__ == "__main__":
    main()
