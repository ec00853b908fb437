"""What a training step straight from a resident sequence costs on STANDARDISED windows beside the two-call route it replaces.

    python tools/series_train_std_cost.py time --route {series,assemble} [--only CASE] [--plan bf16|x3] [--json OUT.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/series_train_std_cost.py run --route {series,assemble} [--only CASE] [--plan bf16|x3]
    python tools/series_train_std_cost.py summarise OUT_series OUT_assemble --json profiles/series_train_std_<name>.json

Cases, 8192 windows, both plans: A1-C2 L=3 standardised (regression) and MiniCheetah-K4 L=8 standardised (contact classification).  `series` =
Engine.step_mse_series_std / step_ce_series_std; `assemble` = SequenceStore.assemble(reuse_buffers=True) + Engine.step_mse / step_ce (classification: plus the
contact flags from the label rows, as models.fused_training_step makes them) -- the only route of a library without the _std entry points (a build of the parent
commit handed over through MSHGNN_LIB).

`time`: after WARM calls, ROUNDS rounds of CALLS calls each between two device events, stepping through SETS start sets; ms per call of every round, their median
and their spread (max - min over the rounds: the run-to-run spread the comparison is read against).  `run` / `summarise`: the per-kernel split from the
profiler's kernel statistics, as tools/series_eval_cost.py."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WINDOWS, WARM, CALLS, ROUNDS, SETS, T, ROWS = 8192, 20, 200, 5, 4, 150, 20000
PROFILE_WARM, PROFILE_ITERS = 3, 20
CASES = {"a1c2_L3_std": ("a1c2", 3), "mck4_L8_std": ("mck4", 8)}


def make_case(kind, L, plan):
    import numpy as np
    import torch
    from morphsym_hgnn_amd import engine as eng, synth, topology
    from morphsym_hgnn_amd.spec import ModelSpec
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    rng = np.random.default_rng(1)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    jp, fp = list(range(12)), list(range(4))
    if kind == "a1c2":
        recipe = quadsdk_a1_c2_recipe(jp, fp, T, 3, normalize=True)
        seq = {"imu_acc": f(ROWS, 3), "imu_omega": f(ROWS, 3), "q": f(ROWS, 12), "qd": f(ROWS, 12), "tau": f(ROWS, 12), "F": f(ROWS, 12), "r_o": f(ROWS, 4)}
        spec = ModelSpec(kind="c2", topology=topology.TOPOLOGIES["a1-c2"](), hidden=128, num_layers=L, widths={t: recipe.width(t) for t in recipe.node_types},
                         regression=True, grf_dimension=3, group=None)
    else:
        recipe = minicheetah_k4_recipe(jp, fp, T, normalize=True)
        seq = {"imu_acc": f(ROWS, 3), "imu_omega": f(ROWS, 3), "q": f(ROWS, 12), "qd": f(ROWS, 12), "p": f(ROWS, 12), "v": f(ROWS, 12),
               "contacts": (f(ROWS, 4) > 0).astype(np.float32)}
        spec = ModelSpec(kind="k4", topology=topology.TOPOLOGIES["mini_cheetah-k4"](), hidden=128, num_layers=L, widths={t: recipe.width(t) for t in recipe.node_types},
                         regression=False, grf_dimension=3, group=None)
    store = SequenceStore(seq, recipe, dtype=plan)
    e = eng.Engine(spec, plan)
    flat = eng.flatten_params(spec, synth.make_params(3, spec.param_shapes()), e.device)
    sets = [torch.randint(0, ROWS - T + 1, (WINDOWS,), generator=torch.Generator().manual_seed(2 + i)).cuda() for i in range(SETS)]
    out, grad, loss = e._results(WINDOWS, None, None, None)

    def series(starts):
        step = e.step_mse_series_std if spec.regression else e.step_ce_series_std
        return step(store, starts, flat, out=out, grad_flat=grad, loss=loss)[3]

    def assemble(starts):
        xs, y, _ = store.assemble(starts, reuse_buffers=True)
        if spec.regression:
            return e.step_mse(xs, flat, y.reshape(-1), WINDOWS, out=out, grad_flat=grad, loss=loss)[1]
        return e.step_ce(xs, flat, (y != 0).to(torch.int32).reshape(WINDOWS, 4), WINDOWS, out=out, grad_flat=grad, loss=loss)[1]
    return {"series": series, "assemble": assemble}, sets


def cases(only, plans):
    for name, (kind, L) in CASES.items():
        if only and name != only:
            continue
        for plan in plans:
            yield name, plan, make_case(kind, L, plan)


def time_route(route, only, plans, out_json):
    import statistics
    import torch
    res = {}
    for name, plan, (calls, sets) in cases(only, plans):
        call = calls[route]
        for i in range(WARM):
            loss = call(sets[i % SETS])
        torch.cuda.synchronize()
        rounds = []
        for _ in range(ROUNDS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(CALLS):
                loss = call(sets[i % SETS])
            b.record()
            torch.cuda.synchronize()
            rounds.append(a.elapsed_time(b) / CALLS)
        res[f"{name} {plan} {route}"] = {"ms_per_call_rounds": [round(r, 4) for r in rounds], "median_ms": round(statistics.median(rounds), 4),
                                         "spread_ms": round(max(rounds) - min(rounds), 4), "loss": float(loss)}
        print(f"{name} {plan} {route}: {json.dumps(res[f'{name} {plan} {route}'])}", flush=True)
    if out_json:
        open(out_json, "w").write(json.dumps(res, indent=1) + "\n")


def run(route, only, plans):
    import torch
    for name, plan, (calls, sets) in cases(only, plans):
        for i in range(PROFILE_WARM + PROFILE_ITERS):
            loss = calls[route](sets[i % SETS])
        torch.cuda.synchronize()
        print(f"{name} {plan} {route}: {PROFILE_WARM + PROFILE_ITERS} calls, loss {float(loss):.6g}", flush=True)


def summarise(dirs, out_json):
    from series_eval_cost import kernel_ms
    res = {}
    n = PROFILE_WARM + PROFILE_ITERS
    for d in dirs:
        k = kernel_ms(d)
        res[os.path.basename(os.path.normpath(d))] = {"ms_per_call": sum(k.values()) / n,
                                                      "kernels_ms_per_call": {name[:80]: v / n for name, v in sorted(k.items(), key=lambda x: -x[1])}}
    txt = json.dumps(res, indent=1)
    print(txt)
    if out_json:
        open(out_json, "w").write(txt + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "run", "summarise"])
    ap.add_argument("dirs", nargs="*")
    ap.add_argument("--route", default="series", choices=["series", "assemble"])
    ap.add_argument("--only", default=None, choices=list(CASES))
    ap.add_argument("--plan", default=None, choices=["bf16", "x3"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    plans = [a.plan] if a.plan else ["bf16", "x3"]
    if a.mode == "time":
        time_route(a.route, a.only, plans, a.json)
    elif a.mode == "run":
        run(a.route, a.only, plans)
    else:
        summarise(a.dirs, a.json)
