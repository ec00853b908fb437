"""Symmetrisation: the non-equivariant MI-HGNN on A1, made exactly C2-equivariant by averaging its predictions over the orbit {identity, gs} --

    f_sym(x) = 1/2 (f(x) + rho_out(gs)^-1 f(gs x))

-- trained THROUGH the average (`symmetrise.Symmetrised`: every step runs the model on an orbit-complete batch, the loss is the averaged prediction's), then
evaluated with `evaluate_sequence_symmetrised`, which also measures how far the raw model is from equivariant.  The symmetrised model's own defect is measured
by feeding it the orbit of x and the orbit of gs x.

    python examples/train_symmetrised.py [--plan bf16|x3] [--steps 20] [--batch 128] [--rows 2000]

Synthetic A1 series stand in for recorded sequences."""
import argparse
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morphsym_hgnn_amd import symmetrise, topology, wrappers                                       # noqa: E402
from morphsym_hgnn_amd.windows import ROW_MASK, GroupAction, ResidentDataset, quadsdk_a1_c2_recipe          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", default="bf16", choices=["bf16", "x3"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128, help="base windows per step (the model sees K times as many)")
    ap.add_argument("--rows", type=int, default=2000)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    seqs = [{"imu_acc": f(n, 3), "imu_omega": f(n, 3), "q": f(n, 12), "qd": f(n, 12), "tau": f(n, 12), "F": f(n, 12), "r_o": f(n, 4)} for n in (a.rows, a.rows // 2)]
    topo, group = topology.TOPOLOGIES["quadruped-mi"](), GroupAction.load("a1-c2")
    recipe = quadsdk_a1_c2_recipe(list(range(12)), list(range(4)), 150, 3, n_base=1)
    orbit = ResidentDataset(seqs, recipe, dtype=a.plan).orbit(group, ("gs",))      # C2: K = 2 elements per window over one resident copy of the series
    action = symmetrise.OutputAction.from_store(orbit, regression=True)             # how gs acts on the 12 GRF outputs: read off the label tables
    K = action.n_elements
    train, val = orbit.split(0.85)
    xs, _, _ = orbit.assemble([0, 1])
    dummy = types.SimpleNamespace(edge_index_dict=topo.edge_index_dict(2, device=dev),
                                  x_dict={t: x[:, :recipe.width(t)].float().contiguous() for t, x in zip(recipe.node_types, xs)})
    os.environ["MSHGNN_DTYPE"] = a.plan
    raw = wrappers.Heterogeneous_GNN_Lightning(128, 3, topo.metadata(), dummy, grf_dimension=3).to(dev)
    sym = symmetrise.Symmetrised(raw, action)      # the same model; its steps run on the averaged prediction
    opt = sym.configure_optimizers()
    edges = topo.edge_index_dict(K * a.batch, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    for step in range(1, a.steps + 1):
        base = torch.randint(0, train.n_windows, (a.batch,), generator=gen, device=dev)      # BASE windows; orbit_batch adds every element of each
        opt.zero_grad(set_to_none=True)
        loss = sym.training_step(train.orbit_batch(base, edges), step)
        loss.backward()
        opt.step()
        if step % 5 == 0 or step == a.steps:
            print(f"step {step}: symmetrised loss {float(loss.detach()):.6g}")
    train.check()

    pred, report = symmetrise.evaluate_sequence_symmetrised(sym, val, topo.edge_index_dict(1, device=dev), a.batch)
    y = orbit.assemble(val.starts(list(range(val.n_windows))))[1]
    print(f"validation MSE of the symmetrised model: {float(((pred - y) ** 2).mean()):.6g} over {val.n_windows} windows")
    for op, r in report.items():
        print(f"  raw model, defect under {op}: rms {r['rms']:.3e}, max {r['max_abs']:.3e}, relative rms {r['relative_rms']:.3e} over {r['n']} values")

    # the symmetrised model's own defect: f_sym(x) from the orbit of x = {x, gs x}, f_sym(gs x) from the orbit of gs x = {gs x, x}
    n = min(val.n_windows, a.batch)
    rows = val.starts(list(range(n))) & ROW_MASK
    el = torch.tensor([0] * n + [1] * n + [1] * n + [0] * n, dtype=torch.int64, device=dev)
    batch = orbit.batch(rows.repeat(4), topo.edge_index_dict(4 * n, device=dev), elements=el)
    with torch.no_grad():
        _, out = raw.step_helper_function(batch)
    halves = [symmetrise.orbit_average(out[:2 * n], action, n), symmetrise.orbit_average(out[2 * n:], action, n)]
    d = symmetrise.EquivarianceDefect(action, dev)
    d.update(torch.cat(halves), n)
    for op, r in d.report().items():
        print(f"  symmetrised model, defect under {op}: rms {r['rms']:.3e}, max {r['max_abs']:.3e} over {r['n']} values")


if __name__ == "__main__":
    main()
