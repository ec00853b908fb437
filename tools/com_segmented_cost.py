"""What the per-segment centroidal-momentum sums cost ("Solo centroidal-momentum windows under the symmetry group").

    python tools/com_segmented_cost.py launches [--json OUT.json]
    python tools/com_segmented_cost.py sweep [--json OUT.json]
    python tools/com_segmented_cost.py all --json profiles/com_segmented_cost.json

`launches`: time per launch from HIP events after warm-up, alternating passes over four cases on one build: mshgnn_metrics_com_segmented at 8192 windows x 4
bases (24 values per window) with sorted ids in three runs and with 8192 distinct shuffled ids, next to mshgnn_metrics_regression_segmented at 8192 x 24 with the
same two id arrangements.  PASSES passes, each timing CALLS back-to-back launches of every case between two events; per case the median over the passes
(min .. max).
`sweep`: one wrappers.evaluate_table sweep over the K = 4 orbit view of a synthetic Solo dataset (COM_HGNN_K4, 3 layers, the default plan) against four
wrappers.evaluate_sequence calls over the identity and the three transformed datasets; alternating, wall time around a device synchronise."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

B, NB, WARM, CALLS, PASSES = 8192, 4, 20, 50, 15


def _summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def launches():
    from morphsym_hgnn_amd import metrics as M
    g = torch.Generator().manual_seed(1)
    y, yp = torch.randn(B, NB * 6, generator=g).cuda(), torch.randn(B, NB * 6, generator=g).cuda()
    ids = {"sorted_3_runs": torch.from_numpy(np.sort(np.arange(B) % 3).astype(np.int32)).cuda(),
           "8192_distinct_shuffled": torch.randperm(B, generator=g).to(torch.int32).cuda()}
    mean, std = np.zeros(6), np.ones(6)
    cases = {}
    for name, seg in ids.items():
        n_seg = 3 if name.startswith("sorted") else B
        com, reg = M.SegmentedComMetrics(n_seg, NB, mean, std), M.SegmentedMetrics(n_seg, True)
        cases["com_segmented_" + name] = (lambda com=com, seg=seg: com.update(y, yp, seg))
        cases["regression_segmented_" + name] = (lambda reg=reg, seg=seg: reg.update(y, yp, seg))
    for f in cases.values():
        for _ in range(WARM):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(PASSES):
        for k, f in cases.items():          # alternating: every pass visits every case
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / CALLS)
    return {"what": f"us per launch (HIP events around {CALLS} launches, {PASSES} alternating passes, after {WARM} warm-up launches), {B} windows x {NB * 6} values",
            **{k: _summary(v) for k, v in times.items()}}


def sweep(rounds=7):
    from morphsym_hgnn_amd import synth, topology, wrappers
    from morphsym_hgnn_amd.spec import ModelSpec
    from morphsym_hgnn_amd.windows import GroupAction, ResidentDataset, solo_com_arrays, solo_com_recipe
    import types
    import yaml
    rng = np.random.default_rng(3)
    rows = (20000, 12000, 6000)
    seqs = [solo_com_arrays(rng.standard_normal((n, 24)).astype(np.float32), rng.standard_normal((n, 6)).astype(np.float32)) for n in rows]
    jp = list(range(12))
    ds = ResidentDataset(seqs, solo_com_recipe("k4_com", jp, 1, symmetry=True), dtype="x3")
    group = GroupAction.load("solo-k4")
    orbit = ds.orbit(group)
    cfg = os.path.join(os.path.dirname(os.path.abspath(wrappers.__file__)), "cfg", "solo-k4.yaml")
    topo = topology.TOPOLOGIES["solo-k4-com"]()
    spec = ModelSpec(kind="k4_com", topology=topo, hidden=128, num_layers=3, widths=synth.feature_widths("k4_com", True), regression=True, grf_dimension=3,
                     group=yaml.safe_load(open(cfg)))
    xs, _, _ = ds.assemble([0, 1])
    dev = ds.device
    dummy = types.SimpleNamespace(edge_index_dict=topo.edge_index_dict(2, device=dev),
                                  x_dict={t: x[:, :ds.recipe.width(t)].float().contiguous() for t, x in zip(ds.recipe.node_types, xs)})
    w = wrappers.COM_HGNN_SYM_Lightning(128, 3, topo.metadata(), dummy, symmetry_mode="MorphSym", group_operator_path=cfg, model_type="heterogeneous_gnn_k4_com",
                                        stats=(np.zeros(6), np.ones(6))).to(dev)
    ei1 = topo.edge_index_dict(1, device=dev)
    stores = [ds] + [ds.transformed(op, group) for op in ("gs", "gt", "gr")]
    view = orbit.view()

    def four():
        out = []
        for s in stores:
            wrappers.evaluate_sequence(w, s, ei1, B)
            out.append(float(w.mse_loss))          # (one host read per call, as the table's one read at its end)
        return out

    def table():
        return wrappers.evaluate_table(w, view, ei1, B).totals["MSE"].cpu().tolist()

    a, b = four(), table()          # warm-up, and the values agree
    worst = max(abs(x - z) / abs(x) for x, z in zip(a, b))
    times = {"four_evaluate_sequence": [], "one_evaluate_table": []}
    for _ in range(rounds):
        for k, f in (("four_evaluate_sequence", four), ("one_evaluate_table", table)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {"what": f"ms per whole sweep (wall time around a device synchronise, {rounds} alternating rounds), COM_HGNN_K4 L=3, default plan, batch {B}, "
                    f"sequences of {rows} rows, orbit K = 4", "windows": view.n_windows, "worst_relative_difference_of_the_rows_MSE": worst,
            **{k: _summary(v) for k, v in times.items()}}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["launches", "sweep", "all"])
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: nothing is measured without one")
    out = {}
    if args.mode in ("launches", "all"):
        out["launches"] = launches()
    if args.mode in ("sweep", "all"):
        out["sweep"] = sweep()
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
