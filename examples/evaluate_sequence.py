"""Evaluate a model over every window of one recorded sequence, straight from the resident series (no assembled windows).

    python examples/evaluate_sequence.py [--normalize] [--plan bf16|x3] [--rows 5000] [--batch 1024]

Synthetic A1 series stand in for a recorded sequence; the loop is the reference's `evaluate_model` without its dataset plumbing
(`wrappers.evaluate_sequence`): predictions per window, the epoch's metrics in the wrapper's state."""
import argparse
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
    ap.add_argument("--normalize", action="store_true", help="standardise every variable over its window (flexibleDataset.py:390-396)")
    ap.add_argument("--plan", default="bf16", choices=["bf16", "x3"])
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--history", type=int, default=150)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    seq = {"imu_acc": f(a.rows, 3), "imu_omega": f(a.rows, 3), "q": f(a.rows, 12), "qd": f(a.rows, 12), "tau": f(a.rows, 12), "F": f(a.rows, 12), "r_o": f(a.rows, 4)}
    topo = topology.TOPOLOGIES["a1-c2"]()
    recipe = quadsdk_a1_c2_recipe(list(range(12)), list(range(4)), a.history, 3, normalize=a.normalize)
    store = SequenceStore(seq, recipe, dtype=a.plan)
    xs, _, _ = store.assemble([0, 1])
    dummy = types.SimpleNamespace(edge_index_dict=topo.edge_index_dict(2, device=dev),
                                  x_dict={t: x[:, :recipe.width(t)].float().contiguous() for t, x in zip(recipe.node_types, xs)})
    os.environ["MSHGNN_DTYPE"] = a.plan
    w = wrappers.HGNN_C2_Lightning_Reg(128, 3, topo.metadata(), dummy, symmetry_mode=None).to(dev)
    pred = wrappers.evaluate_sequence(w, store, topo.edge_index_dict(1, device=dev), a.batch)
    torch.cuda.synchronize()
    print(f"{pred.shape[0]} windows of {a.history} steps, predictions {tuple(pred.shape)}")
    for k, v in sorted(w.logged.items()):
        if k.startswith("test_") and v is not None:
            print(f"  {k}: {float(v):.6g}")


if __name__ == "__main__":
    main()
