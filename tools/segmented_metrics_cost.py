"""What the segmented step metrics cost: the launch against the whole-batch step metrics, and the one-sweep evaluation table
against one sweep per (operator, sequence).

    python tools/segmented_metrics_cost.py launches                                  (the launches alone; meant to run under the profiler)
    python tools/segmented_metrics_cost.py profile [--json OUT.json]                 (ONE `rocprofv3 --kernel-trace --stats` run of `launches`, read back)
    python tools/segmented_metrics_cost.py sweep --route {table,twelve} [--json OUT.json]
    python tools/segmented_metrics_cost.py compare [--json OUT.json]                 (fresh processes, interleaved: twelve, table, twelve, table)
    python tools/segmented_metrics_cost.py all --json profiles/segmented_metrics_cost.json

`launches`: 8192 x 12 fp32 inputs; CALLS launches each of mshgnn_metrics_regression_step (the yardstick), of mshgnn_metrics_regression_segmented with
sorted ids in three runs (an evaluation sweep's batch) and of the same with 8192 distinct shuffled ids, in that order: `profile` separates the two
segmented cases by their position in the kernel trace.
`sweep`: A1-C2, 3 layers, bf16 plan, batch 8192, three sequences, orbit of K = 4.  `table` = one wrappers.evaluate_table over the orbit view; `twelve` =
wrappers.evaluate_sequence once per (operator, sequence) over the sibling stores' one-sequence views -- what a library without the segmented metrics
offers.  ROUNDS rounds of one whole sweep each, wall time around a device synchronisation (each of the twelve calls ends in a host read of its own: that
is part of its cost); median and spread (max - min).  Every child process runs under its own time limit and a failure stops the chain."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, PER, CALLS, WARM = 8192, 12, 50, 5
ROUNDS, T, SEQ_ROWS, BATCH = 5, 150, (20000, 12000, 6000), 8192
STEP_KERNEL, SEG_KERNEL = "k_metrics_reg<256>", "k_metrics_reg_seg"


def launches():
    import torch
    from morphsym_hgnn_amd import metrics as M
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(0)
    y, yp = torch.randn(B, PER, generator=g).to(dev), torch.randn(B, PER, generator=g).to(dev)
    sorted_ids = (torch.arange(B) * 3 // B).to(torch.int32).to(dev)
    shuffled = torch.randperm(B, generator=g).to(torch.int32).to(dev)
    step = M.StepMetrics(True, dev)
    seg3, seg_all = M.SegmentedMetrics(3, True, dev), M.SegmentedMetrics(B, True, dev)
    for n in (WARM, CALLS):          # (the warm-up launches come first in the trace: `profile` takes the last CALLS of every group)
        for _ in range(n):
            step._launch(y, yp, False)
        torch.cuda.synchronize()
    for n in (WARM, CALLS):
        for _ in range(n):
            seg3.update(y, yp, sorted_ids)
        torch.cuda.synchronize()
    for n in (WARM, CALLS):
        for _ in range(n):
            seg_all.update(y, yp, shuffled)
        torch.cuda.synchronize()
    seg3.check(); seg_all.check()
    print("launches done", flush=True)


def profile(out_json):
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "seg", "--",
                        sys.executable, os.path.abspath(__file__), "launches"], check=True, timeout=240)
        trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not trace:
            raise SystemExit("no kernel trace written")
        rows = sorted(csv.DictReader(open(trace[0])), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    step = [us(r) for r in rows if r["Kernel_Name"].startswith("void k_metrics_reg<256>") or STEP_KERNEL in r["Kernel_Name"]]
    seg = [us(r) for r in rows if SEG_KERNEL in r["Kernel_Name"]]
    if len(step) != WARM + CALLS or len(seg) != 2 * (WARM + CALLS):
        raise SystemExit(f"unexpected launch counts in the trace: step {len(step)}, segmented {len(seg)}")
    groups = {"regression_step": step[WARM:], "segmented_sorted_3_runs": seg[WARM:WARM + CALLS], "segmented_8192_distinct_shuffled": seg[2 * WARM + CALLS:]}
    res = {k: {"launches": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for k, v in groups.items()}
    base = res["regression_step"]["median_us"]
    for k in ("segmented_sorted_3_runs", "segmented_8192_distinct_shuffled"):
        res[k]["ratio_to_regression_step"] = round(res[k]["median_us"] / base, 2)
    res["note"] = f"one rocprofv3 --kernel-trace --stats run, {B} x {PER} fp32, kernel durations from the trace"
    print(json.dumps(res, indent=1), flush=True)
    if out_json:
        open(out_json, "w").write(json.dumps(res, indent=1) + "\n")
    return res


def make_sweep(route):
    import numpy as np
    import torch
    import bench
    from morphsym_hgnn_amd import wrappers
    from morphsym_hgnn_amd.windows import GroupAction, ResidentDataset, quadsdk_a1_c2_recipe
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(1)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    seq = lambda n: {"imu_acc": f(n, 3), "imu_omega": f(n, 3), "q": f(n, 12), "qd": f(n, 12), "tau": f(n, 12), "F": f(n, 12), "r_o": f(n, 4)}
    cfg = os.path.join(ROOT, "morphsym_hgnn_amd", "cfg", "a1-c2.yaml")
    group = GroupAction.load("a1-c2")
    recipe = quadsdk_a1_c2_recipe(list(range(12)), list(range(4)), T, 3)
    spec = bench.build_spec(3)
    ds = ResidentDataset([seq(n) for n in SEQ_ROWS], recipe, dtype="bf16", device=dev)
    os.environ["MSHGNN_DTYPE"] = "bf16"
    torch.manual_seed(0)
    xs, _, _ = ds.assemble([0, 1])
    dummy = types.SimpleNamespace(edge_index_dict=spec.topology.edge_index_dict(2, device=dev),
                                  x_dict={t: x[:, :recipe.width(t)].float().contiguous() for t, x in zip(recipe.node_types, xs)})
    model = wrappers.HGNN_C2_Lightning_Reg(spec.hidden, 3, spec.topology.metadata(), dummy, symmetry_mode="MorphSym", group_operator_path=cfg).to(dev)
    edges = {}

    def ei(n):
        if n not in edges:
            edges[n] = spec.topology.edge_index_dict(n, device=dev)
        return edges[n]
    if route == "table":
        view = ds.orbit(group).view()

        def sweep():
            res = wrappers.evaluate_table(model, view, ei, BATCH)
            return [float(v) for v in res.table["MSE"].flatten().tolist()]
    else:
        sibs = [ds] + [ds.transformed(op, group) for op in ("gs", "gt", "gr")]
        views = [[s.subset([(0, n) if j == k else (0, 0) for j, n in enumerate(ds.seq_windows)]) for k in range(len(SEQ_ROWS))] for s in sibs]

        def sweep():
            out = []
            for per_op in views:
                for v in per_op:
                    wrappers.evaluate_sequence(model, v, ei, BATCH)
                    out.append(float(model.mse_loss))
            return out
    return sweep


def sweep_route(route, out_json):
    import torch
    sweep = make_sweep(route)
    mse = sweep()          # warm-up: plans, buffers, edge tensors
    torch.cuda.synchronize()
    rounds = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        mse = sweep()
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) * 1e3)
    res = {"route": route, "ms_per_sweep_rounds": [round(r, 3) for r in rounds], "median_ms": round(statistics.median(rounds), 3),
           "spread_ms": round(max(rounds) - min(rounds), 3), "mse": mse}
    print(json.dumps(res), flush=True)
    if out_json:
        open(out_json, "w").write(json.dumps(res, indent=1) + "\n")
    return res


def compare(out_json):
    runs = []
    with tempfile.TemporaryDirectory() as d:
        for k, route in enumerate(("twelve", "table", "twelve", "table")):
            tmp = os.path.join(d, f"sweep_{k}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "sweep", "--route", route, "--json", tmp], check=True, timeout=240)
            runs.append(json.load(open(tmp)))
    med = lambda route: statistics.mean(r["median_ms"] for r in runs if r["route"] == route)
    worst = max(abs(a - b) / abs(b) for a, b in zip(runs[1]["mse"], runs[0]["mse"]))
    res = {"runs": [{k: r[k] for k in ("route", "median_ms", "spread_ms", "ms_per_sweep_rounds")} for r in runs],
           "twelve_ms": round(med("twelve"), 3), "table_ms": round(med("table"), 3), "difference_ms": round(med("table") - med("twelve"), 3),
           "largest_spread_ms": max(r["spread_ms"] for r in runs), "worst_relative_mse_difference_between_routes": worst,
           "note": f"A1-C2 L=3 bf16 plan, batch {BATCH}, sequences of {SEQ_ROWS} rows, K = 4; one sweep = all 12 (operator, sequence) cells"}
    print(json.dumps(res, indent=1), flush=True)
    if out_json:
        open(out_json, "w").write(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["launches", "profile", "sweep", "compare", "all"])
    ap.add_argument("--route", default="table", choices=["table", "twelve"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.mode == "launches":
        launches()
    elif a.mode == "profile":
        profile(a.json)
    elif a.mode == "sweep":
        sweep_route(a.route, a.json)
    elif a.mode == "compare":
        compare(a.json)
    else:
        # (the two measurements in processes of their own, one after the other; a failure of the first stops the second)
        me = [sys.executable, os.path.abspath(__file__)]
        with tempfile.TemporaryDirectory() as d:
            subprocess.run(me + ["profile", "--json", os.path.join(d, "p.json")], check=True, timeout=300)
            subprocess.run(me + ["compare", "--json", os.path.join(d, "c.json")], check=True, timeout=1000)
            out = {"launch": json.load(open(os.path.join(d, "p.json"))), "sweep": json.load(open(os.path.join(d, "c.json")))}
        print(json.dumps(out, indent=1))
        if a.json:
            open(a.json, "w").write(json.dumps(out, indent=1) + "\n")
