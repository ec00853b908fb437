"""What the index-mapping launch of a resident dataset costs in front of a training step.

    python tools/dataset_starts_cost.py time --route {dataset,store} [--windows 32 8192] [--json OUT.json]
    python tools/dataset_starts_cost.py compare --parent-lib PATH/libmshgnn.so [--json OUT.json]

`dataset` = DatasetView.batch(device indices) -- mshgnn_dataset_starts -- + HGNN_C2_Lightning_Reg.training_step, on a ResidentDataset of three sequences;
`store` = SequenceStore.batch(device start rows) + training_step on one sequence of as many rows: the only route of a library without the entry point
(a build of the parent commit handed over through MSHGNN_LIB).  A1-C2, 3 layers, bf16 plan, 32 and 8192 windows of 150 steps.

`time`: after WARM calls, ROUNDS rounds of CALLS calls each between two device events, stepping through SETS index sets; ms per call of every round, their
median and their spread (max - min over the rounds: what a difference is read against) -- the method of tools/series_train_std_cost.py.
`compare`: fresh child processes, interleaved: parent store, dataset, parent store, dataset, then store on this build (which must give the parent's figure);
prints one table row per batch size."""
import argparse
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, CALLS, ROUNDS, SETS, T = 20, 200, 5, 4, 150
SEQ_ROWS = (3000, 7000, 10000)      # the dataset's sequences; the store route's single sequence has their sum


def make_case(route, windows):
    import numpy as np
    import torch
    import bench
    from morphsym_hgnn_amd import wrappers
    from morphsym_hgnn_amd.windows import ResidentDataset, SequenceStore, quadsdk_a1_c2_recipe
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(1)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    seq = lambda n: {"imu_acc": f(n, 3), "imu_omega": f(n, 3), "q": f(n, 12), "qd": f(n, 12), "tau": f(n, 12), "F": f(n, 12), "r_o": f(n, 4)}
    recipe = quadsdk_a1_c2_recipe(list(range(12)), list(range(4)), T, 3)
    spec = bench.build_spec(3)
    if route == "dataset":
        store = ResidentDataset([seq(n) for n in SEQ_ROWS], recipe, dtype="bf16", device=dev)
        source = store.split()[0]
    else:
        store = source = SequenceStore(seq(sum(SEQ_ROWS)), recipe, dtype="bf16", device=dev)
    os.environ["MSHGNN_DTYPE"] = "bf16"
    torch.manual_seed(0)
    xs, _, _ = store.assemble([0, 1])
    dummy = types.SimpleNamespace(edge_index_dict=spec.topology.edge_index_dict(2, device=dev),
                                  x_dict={t: x[:, :recipe.width(t)].float().contiguous() for t, x in zip(recipe.node_types, xs)})
    cfg = os.path.join(ROOT, "morphsym_hgnn_amd", "cfg", "a1-c2.yaml")
    model = wrappers.HGNN_C2_Lightning_Reg(spec.hidden, 3, spec.topology.metadata(), dummy, symmetry_mode="MorphSym", group_operator_path=cfg).to(dev)
    ei = spec.topology.edge_index_dict(windows, device=dev)
    sets = [torch.randint(0, len(source), (windows,), generator=torch.Generator().manual_seed(2 + i)).to(dev) for i in range(SETS)]

    def call(ix, step):
        return model.training_step(source.batch(ix, ei), step)
    return call, sets, source


def time_route(route, sizes, out_json):
    import statistics
    import torch
    res = {}
    for windows in sizes:
        call, sets, source = make_case(route, windows)
        for i in range(WARM):
            loss = call(sets[i % SETS], i)
        torch.cuda.synchronize()
        rounds = []
        for _ in range(ROUNDS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(CALLS):
                loss = call(sets[i % SETS], i)
            b.record()
            torch.cuda.synchronize()
            rounds.append(a.elapsed_time(b) / CALLS)
        if route == "dataset":
            source.check()
        key = f"{route} B{windows}"
        res[key] = {"ms_per_call_rounds": [round(r, 4) for r in rounds], "median_ms": round(statistics.median(rounds), 4),
                    "spread_ms": round(max(rounds) - min(rounds), 4), "loss": float(loss.detach())}
        print(f"{key}: {json.dumps(res[key])}", flush=True)
    if out_json:
        open(out_json, "w").write(json.dumps(res, indent=1) + "\n")
    return res


def compare(parent_lib, sizes, out_json):
    if not os.path.exists(parent_lib):
        raise SystemExit(f"{parent_lib}: no such library (build the parent commit and pass its libmshgnn.so)")
    runs = []
    for label, route, lib in (("parent store", "store", parent_lib), ("dataset", "dataset", None), ("parent store", "store", parent_lib),
                              ("dataset", "dataset", None), ("store", "store", None)):
        env = dict(os.environ)
        env.pop("MSHGNN_LIB", None)
        if lib:
            env["MSHGNN_LIB"] = os.path.abspath(lib)
        tmp = os.path.join(os.path.dirname(os.path.abspath(out_json)) if out_json else "/tmp", f"dataset_starts_cost_{len(runs)}.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "time", "--route", route, "--windows", *map(str, sizes), "--json", tmp], check=True, env=env)
        runs.append((label, json.load(open(tmp))))
        os.remove(tmp)
    table = {}
    for windows in sizes:
        row = {}
        for label, res in runs:
            r = res[f"{'dataset' if label == 'dataset' else 'store'} B{windows}"]
            row.setdefault(label, []).append({"median_ms": r["median_ms"], "spread_ms": r["spread_ms"]})
        med = lambda label: sum(x["median_ms"] for x in row[label]) / len(row[label])
        row["difference_ms"] = round(med("dataset") - med("parent store"), 4)
        row["largest_spread_ms"] = max(x["spread_ms"] for label in ("parent store", "dataset") for x in row[label])
        table[f"B{windows}"] = row
        print(f"B{windows}: {json.dumps(row)}", flush=True)
    if out_json:
        open(out_json, "w").write(json.dumps(table, indent=1) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "compare"])
    ap.add_argument("--route", default="dataset", choices=["dataset", "store"])
    ap.add_argument("--windows", type=int, nargs="+", default=[32, 8192])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.mode == "time":
        time_route(a.route, a.windows, a.json)
    else:
        compare(a.parent_lib or "", a.windows, a.json)
