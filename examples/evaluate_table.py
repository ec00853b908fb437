"""The evaluators' table -- one row per symmetry operator (None, gs, gt, gr), MSE / RMSE / L1 per test sequence -- out of ONE sweep over an orbit view of a
resident dataset: every window carries the segment id element * n_sequences + sequence and `metrics.SegmentedMetrics` keeps the sums per id, one
deterministic launch per batch and no host read until the sweep is over (the reference's research/evaluator_regression-grf_c2.py runs one evaluation per
operator and sequence).

    python examples/evaluate_table.py [--plan bf16|x3] [--batch 512] [--history 150] [--csv PATH]

Three synthetic A1 sequences of different lengths stand in for recorded ones; the CSV goes to stdout (or --csv)."""
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
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--history", type=int, default=150)
    ap.add_argument("--csv", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    seq = lambda n: {"imu_acc": f(n, 3), "imu_omega": f(n, 3), "q": f(n, 12), "qd": f(n, 12), "tau": f(n, 12), "F": f(n, 12), "r_o": f(n, 4)}
    topo = topology.TOPOLOGIES["a1-c2"]()
    group = GroupAction.load("a1-c2")
    recipe = quadsdk_a1_c2_recipe(list(range(12)), list(range(4)), a.history, 3)
    ds = ResidentDataset([seq(n) for n in (1500, 900, 400)], recipe, dtype=a.plan, names=["forest", "sidewalk", "small_pebbles"])
    xs, _, _ = ds.assemble([0, 1])
    dummy = types.SimpleNamespace(edge_index_dict=topo.edge_index_dict(2, device=dev),
                                  x_dict={t: x[:, :recipe.width(t)].float().contiguous() for t, x in zip(recipe.node_types, xs)})
    os.environ["MSHGNN_DTYPE"] = a.plan
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "morphsym_hgnn_amd", "cfg", "a1-c2.yaml")
    w = wrappers.HGNN_C2_Lightning_Reg(128, 3, topo.metadata(), dummy, symmetry_mode="MorphSym", group_operator_path=cfg).to(dev)
    view = ds.orbit(group).view()
    res = wrappers.evaluate_table(w, view, topo.edge_index_dict(1, device=dev), a.batch)
    print(f"# {len(view)} windows = {view.n_elements} operators x {view.n_windows} windows of {view.n_sequences} sequences, one sweep; "
          f"windows per sequence {[int(v) for v in res.table['n'][0].tolist()]}", file=sys.stderr)
    res.to_csv(a.csv if a.csv else sys.stdout)


if __name__ == "__main__":
    main()
