"""What the sign of group-transformed windows costs the series routes ("Group-transformed windows").

    python tools/window_symmetry_cost.py time [--operator none|gs] [--json OUT.json]
    python tools/window_symmetry_cost.py merge A.json B.json ... --json profiles/window_symmetry_cost.json

`time`: 8192 windows, A1-C2 L=3 and MiniCheetah-K4 L=8, plain and standardised recipes, both plans, evaluation (Engine.forward_series) and training
(Engine.step_*_series / step_*_series_std) straight from the resident series -- the timing loop of tools/series_train_std_cost.py: WARM calls, then ROUNDS rounds
of CALLS calls between two device events over SETS start sets; ms per call of every round, their median and spread.  `--operator none` is an unsigned recipe
(also what a build of the parent commit handed over through MSHGNN_LIB can run: the comparison is this build against that one, two interleaved fresh
processes each); `--operator gs` times the transformed sibling store beside it."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WINDOWS, WARM, CALLS, ROUNDS, SETS, T, ROWS = 8192, 20, 100, 5, 4, 150, 20000
CASES = {"a1c2_L3": ("a1c2", 3), "mck4_L8": ("mck4", 8)}


def make_case(kind, L, std, plan, operator):
    import numpy as np
    import torch
    from morphsym_hgnn_amd import engine as eng, synth, topology
    from morphsym_hgnn_amd.spec import ModelSpec
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    rng = np.random.default_rng(1)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    jp, fp = list(range(12)), list(range(4))
    if kind == "a1c2":
        recipe, gname = quadsdk_a1_c2_recipe(jp, fp, T, 3, normalize=std), "a1-c2"
        seq = {"imu_acc": f(ROWS, 3), "imu_omega": f(ROWS, 3), "q": f(ROWS, 12), "qd": f(ROWS, 12), "tau": f(ROWS, 12), "F": f(ROWS, 12), "r_o": f(ROWS, 4)}
        spec = ModelSpec(kind="c2", topology=topology.TOPOLOGIES["a1-c2"](), hidden=128, num_layers=L, widths={t: recipe.width(t) for t in recipe.node_types},
                         regression=True, grf_dimension=3, group=None)
    else:
        recipe, gname = minicheetah_k4_recipe(jp, fp, T, normalize=std), "mini_cheetah-k4"
        seq = {"imu_acc": f(ROWS, 3), "imu_omega": f(ROWS, 3), "q": f(ROWS, 12), "qd": f(ROWS, 12), "p": f(ROWS, 12), "v": f(ROWS, 12),
               "contacts": (f(ROWS, 4) > 0).astype(np.float32)}
        spec = ModelSpec(kind="k4", topology=topology.TOPOLOGIES["mini_cheetah-k4"](), hidden=128, num_layers=L, widths={t: recipe.width(t) for t in recipe.node_types},
                         regression=False, grf_dimension=3, group=None)
    store = SequenceStore(seq, recipe, dtype=plan)
    if operator != "none":
        from morphsym_hgnn_amd.windows import GroupAction
        store = store.transformed(operator, GroupAction.load(gname))
    e = eng.Engine(spec, plan)
    flat = eng.flatten_params(spec, synth.make_params(3, spec.param_shapes()), e.device)
    sets = [torch.randint(0, ROWS - T + 1, (WINDOWS,), generator=torch.Generator().manual_seed(2 + i)).cuda() for i in range(SETS)]
    out, grad, loss = e._results(WINDOWS, None, None, None)
    if std:
        step = e.step_mse_series_std if spec.regression else e.step_ce_series_std
    else:
        step = e.step_mse_series if spec.regression else e.step_ce_series
    return {"eval": lambda st: e.forward_series(store, st, flat, labels=False)[3], "train": lambda st: step(store, st, flat, out=out, grad_flat=grad, loss=loss)[3]}, sets


def time_all(operator, out_json):
    import torch
    res = {"library": os.environ.get("MSHGNN_LIB", "this build"), "operator": operator, "windows": WINDOWS, "cases": {}}
    for name, (kind, L) in CASES.items():
        for std in (False, True):
            for plan in ("bf16", "x3"):
                calls, sets = make_case(kind, L, std, plan, operator)
                for route, call in calls.items():
                    for i in range(WARM):
                        call(sets[i % SETS])
                    torch.cuda.synchronize()
                    rounds = []
                    for _ in range(ROUNDS):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for i in range(CALLS):
                            call(sets[i % SETS])
                        b.record()
                        torch.cuda.synchronize()
                        rounds.append(a.elapsed_time(b) / CALLS)
                    key = f"{name}{'_std' if std else ''} {plan} {route}"
                    res["cases"][key] = {"ms_per_call_rounds": [round(r, 4) for r in rounds], "median_ms": round(statistics.median(rounds), 4),
                                         "spread_ms": round(max(rounds) - min(rounds), 4)}
                    print(f"{key}: {json.dumps(res['cases'][key])}", flush=True)
    if out_json:
        open(out_json, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "merge"])
    ap.add_argument("files", nargs="*")
    ap.add_argument("--operator", default="none", choices=["none", "gs", "gt", "gr"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.mode == "time":
        time_all(a.operator, a.json)
    else:
        runs = [dict(json.load(open(f)), run=os.path.splitext(os.path.basename(f))[0]) for f in a.files]
        open(a.json, "w").write(json.dumps({"runs": runs}, indent=1) + "\n")
