"""The Solo-12 centroidal-momentum models under the symmetry group: the orbit view of a resident dataset, the reference evaluator's table -- one row per
symmetry operator with Test Loss, Test Cos Sim Lin and Test Cos Sim Ang (research/evaluator_regression-com.py:50-76, whose own loop cannot run: its loader hands
apply_symmetry a Python list) -- out of ONE sweep, and the MLP baseline symmetrised over the orbit.

    python examples/evaluate_com_symmetry.py [--batch 512] [--layers 3] [--csv PATH]

Synthetic Solo series stand in for recorded ones: X [N, 24] (q | qd) and Y [N, 6] random, the base series zeros as in the dataset, stats = (zeros, ones).
COM_HGNN_K4 is equivariant by architecture on that data (its rows agree up to rounding and its defect is 0); the MLP is not, and `Symmetrised` makes it so."""
import argparse
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morphsym_hgnn_amd import symmetrise as sym, topology, wrappers                                                                      # noqa: E402
from morphsym_hgnn_amd.windows import GroupAction, ResidentDataset, solo_com_arrays, solo_com_mlp_recipe, solo_com_recipe          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--csv", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    seqs = [solo_com_arrays(rng.standard_normal((n, 24)).astype(np.float32), rng.standard_normal((n, 6)).astype(np.float32)) for n in (1500, 900, 400)]
    names, stats = ["trot", "walk", "bound"], (np.zeros(6), np.ones(6))
    jp = list(range(12))
    group = GroupAction.load("solo-k4")

    # the K4 model: symmetry=True recipes name the group parts of their series, so the dataset has an orbit
    topo = topology.TOPOLOGIES["solo-k4-com"]()
    ds = ResidentDataset(seqs, solo_com_recipe("k4_com", jp, 1, symmetry=True), dtype="x3", names=names)
    view = ds.orbit(group).view()
    xs, _, _ = ds.assemble([0, 1])
    dummy = types.SimpleNamespace(edge_index_dict=topo.edge_index_dict(2, device=dev),
                                  x_dict={t: x[:, :ds.recipe.width(t)].float().contiguous() for t, x in zip(ds.recipe.node_types, xs)})
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "morphsym_hgnn_amd", "cfg", "solo-k4.yaml")
    torch.manual_seed(0)
    k4 = wrappers.COM_HGNN_SYM_Lightning(128, a.layers, topo.metadata(), dummy, symmetry_mode="MorphSym", group_operator_path=cfg,
                                         model_type="heterogeneous_gnn_k4_com", stats=stats).to(dev)
    res = wrappers.evaluate_table(k4, view, topo.edge_index_dict(1, device=dev), a.batch)
    print(f"# COM_HGNN_K4: {len(view)} windows = {view.n_elements} operators x {view.n_windows} windows of {view.n_sequences} sequences, one sweep; "
          f"per-sequence MSE of the identity row {[round(v, 6) for v in res.table['MSE'][0].tolist()]}", file=sys.stderr)
    res.to_csv(a.csv if a.csv else sys.stdout)

    # the MLP baseline: its table differs from row to row; symmetrised over the orbit it is exactly equivariant
    ds_mlp = ResidentDataset(seqs, solo_com_mlp_recipe(jp, 1, symmetry=True), dtype="x3", names=names)
    orbit = ds_mlp.orbit(group)
    mlp = wrappers.COM_MLP_Lightning(24, 128, 6, a.layers, batch_size=a.batch, stats=stats).to(dev)
    wrappers.evaluate_table(mlp, orbit.view(), {}, a.batch).to_csv(sys.stdout)
    action = sym.OutputAction.from_store(orbit, True)
    view_mlp = sym.Symmetrised(mlp, action)
    preds, report = sym.evaluate_sequence_symmetrised(view_mlp, orbit, {}, a.batch)
    print(f"# COM MLP: raw equivariance defect per operator (max |f(g x) - g f(x)|) {({op: round(r['max_abs'], 4) for op, r in report.items()})}; "
          f"{preds.shape[0]} symmetrised predictions of {preds.shape[1]} values", file=sys.stderr)


if __name__ == "__main__":
    main()
