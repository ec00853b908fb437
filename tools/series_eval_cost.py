"""What evaluation straight from a resident sequence costs beside the two-call route it replaces.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/series_eval_cost.py run --route {series,assemble} [--only CASE] [--plan bf16|x3]
    python tools/series_eval_cost.py summarise OUT_series OUT_assemble --json profiles/series_eval_<name>.json

`run` executes, for 8192 windows on both plans, the cases A1-C2 L=3, MiniCheetah-K4 L=8 and MiniCheetah-K4 L=8 standardised: WARM untimed calls, then ITERS
calls of ONE route -- `series` = Engine.forward_series, `assemble` = SequenceStore.assemble + Engine.forward(training=False), the only route of a library
without mshgnn_forward_series (a build of the parent commit handed over through MSHGNN_LIB).  Kernel times come from the profiler's per-kernel statistics,
not from host clocks; `summarise` adds the kernels of each route up per call."""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WINDOWS, WARM, ITERS, T, ROWS = 8192, 3, 20, 150, 20000
CASES = {"a1c2_L3": ("a1c2", 3, False), "mck4_L8": ("mck4", 8, False), "mck4_L8_std": ("mck4", 8, True)}


def run(route, only, plans):
    import numpy as np
    import torch
    from morphsym_hgnn_amd import engine as eng, synth, topology
    from morphsym_hgnn_amd.spec import ModelSpec
    from morphsym_hgnn_amd.windows import SequenceStore, quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    rng = np.random.default_rng(1)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    for name, (kind, L, std) in CASES.items():
        if only and name != only:
            continue
        for plan in plans:
            if kind == "a1c2":
                topo = topology.TOPOLOGIES["a1-c2"]()
                jp, fp = list(range(12)), list(range(4))
                recipe = quadsdk_a1_c2_recipe(jp, fp, T, 3, normalize=std)
                seq = {"imu_acc": f(ROWS, 3), "imu_omega": f(ROWS, 3), "q": f(ROWS, 12), "qd": f(ROWS, 12), "tau": f(ROWS, 12), "F": f(ROWS, 12), "r_o": f(ROWS, 4)}
                spec = ModelSpec(kind="c2", topology=topo, hidden=128, num_layers=L, widths={t: recipe.width(t) for t in recipe.node_types}, regression=True,
                                 grf_dimension=3, group=None)
            else:
                topo = topology.TOPOLOGIES["mini_cheetah-k4"]()
                jp, fp = list(range(12)), list(range(4))
                recipe = minicheetah_k4_recipe(jp, fp, T, normalize=std)
                seq = {"imu_acc": f(ROWS, 3), "imu_omega": f(ROWS, 3), "q": f(ROWS, 12), "qd": f(ROWS, 12), "p": f(ROWS, 12), "v": f(ROWS, 12),
                       "contacts": (f(ROWS, 4) > 0).astype(np.float32)}
                spec = ModelSpec(kind="k4", topology=topo, hidden=128, num_layers=L, widths={t: recipe.width(t) for t in recipe.node_types}, regression=False,
                                 grf_dimension=3, group=None)
            store = SequenceStore(seq, recipe, dtype=plan)
            e = eng.Engine(spec, plan)
            flat = eng.flatten_params(spec, synth.make_params(3, spec.param_shapes()), e.device)
            starts = torch.randint(0, ROWS - T + 1, (WINDOWS,), generator=torch.Generator().manual_seed(2)).cuda()

            def call():
                if route == "series":
                    return e.forward_series(store, starts, flat)[3]
                xs, _, _ = store.assemble(starts, reuse_buffers=True)
                return e.forward(xs, flat, WINDOWS, training=False)
            for _ in range(WARM + ITERS):
                out = call()
            torch.cuda.synchronize()
            print(f"{name} {plan} {route}: {WARM + ITERS} calls, out sum {float(out.sum()):.6g}", flush=True)


def kernel_ms(directory):
    """{kernel name: total ms} from the profiler's kernel statistics under `directory`."""
    tot = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            tot[row["Name"]] = tot.get(row["Name"], 0.0) + float(row["TotalDurationNs"]) / 1e6
    return tot


def summarise(dirs, out_json):
    res = {}
    for d in dirs:
        k = kernel_ms(d)
        calls = WARM + ITERS
        res[os.path.basename(os.path.normpath(d))] = {"ms_per_call": sum(k.values()) / calls, "kernels_ms_per_call": {n[:80]: v / calls for n, v in sorted(k.items(), key=lambda x: -x[1])}}
    txt = json.dumps(res, indent=1)
    print(txt)
    if out_json:
        open(out_json, "w").write(txt + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "summarise"])
    ap.add_argument("dirs", nargs="*")
    ap.add_argument("--route", default="series", choices=["series", "assemble"])
    ap.add_argument("--only", default=None, choices=list(CASES))
    ap.add_argument("--plan", default=None, choices=["bf16", "x3"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.mode == "run":
        run(a.route, a.only, [a.plan] if a.plan else ["bf16", "x3"])
    else:
        summarise(a.dirs, a.json)
