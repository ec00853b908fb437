"""What a group element per window costs: an orbit batch with random elements beside the same calls on ONE sibling store, whose kernels are
the parent commit's, byte for byte (profiles/orbit_device_text.txt).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/window_orbit_cost.py run --store {orbit,sibling} --call {forward,step,assemble} [--only CASE] [--plan bf16|x3]
    python tools/window_orbit_cost.py summarise OUT_a OUT_b ... --json profiles/window_orbit_cost.json

`run` executes, for 8192 windows, the cases A1-C2 L=3 and MiniCheetah-K4 L=8 standardised on both plans: WARM untimed calls, then ITERS calls of ONE route --
`forward` = Engine.forward_series, `step` = the one-call training step from the series (standardised case: its _std form), `assemble` = SequenceStore.assemble alone
(the pass an assemble-then-call default would add).  Kernel times come from the profiler's per-kernel statistics, not from host clocks; `summarise` adds the kernels
of each run up per call (a directory's name says what ran)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.series_eval_cost import kernel_ms      # noqa: E402
WINDOWS, WARM, ITERS, T, ROWS = 8192, 3, 20, 150, 20000
CASES = {"a1c2_L3": ("a1c2", 3, False), "mck4_L8_std": ("mck4", 8, True)}


def run(which, call_name, only, plans):
    import numpy as np
    import torch
    from morphsym_hgnn_amd import engine as eng, synth, topology
    from morphsym_hgnn_amd.spec import ModelSpec
    from morphsym_hgnn_amd.windows import GroupAction, SequenceStore, quadsdk_a1_c2_recipe, minicheetah_k4_recipe
    rng = np.random.default_rng(1)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    jp, fp = list(range(12)), list(range(4))
    for name, (kind, L, std) in CASES.items():
        if only and name != only:
            continue
        for plan in plans:
            if kind == "a1c2":
                topo, group = topology.TOPOLOGIES["a1-c2"](), GroupAction.load("a1-c2")
                recipe = quadsdk_a1_c2_recipe(jp, fp, T, 3, normalize=std)
                seq = {"imu_acc": f(ROWS, 3), "imu_omega": f(ROWS, 3), "q": f(ROWS, 12), "qd": f(ROWS, 12), "tau": f(ROWS, 12), "F": f(ROWS, 12), "r_o": f(ROWS, 4)}
            else:
                topo, group = topology.TOPOLOGIES["mini_cheetah-k4"](), GroupAction.load("mini_cheetah-k4")
                recipe = minicheetah_k4_recipe(jp, fp, T, normalize=std)
                seq = {"imu_acc": f(ROWS, 3), "imu_omega": f(ROWS, 3), "q": f(ROWS, 12), "qd": f(ROWS, 12), "p": f(ROWS, 12), "v": f(ROWS, 12),
                       "contacts": (f(ROWS, 4) > 0).astype(np.float32)}
            spec = ModelSpec(kind="c2" if kind == "a1c2" else "k4", topology=topo, hidden=128, num_layers=L, widths={t: recipe.width(t) for t in recipe.node_types},
                             regression=kind == "a1c2", grf_dimension=3, group=None)
            parent = SequenceStore(seq, recipe, dtype=plan)
            store = parent.orbit(group) if which == "orbit" else parent.transformed("gs", group)
            e = eng.Engine(spec, plan)
            flat = eng.flatten_params(spec, synth.make_params(3, spec.param_shapes()), e.device)
            g = torch.Generator().manual_seed(2)
            starts = torch.randint(0, ROWS - T + 1, (WINDOWS,), generator=g)
            if which == "orbit":      # a random element per window
                starts = starts | (torch.randint(0, store.n_elements, (WINDOWS,), generator=g) << 56)
            starts = starts.cuda()
            if call_name == "forward":
                call = lambda: e.forward_series(store, starts, flat)[3]
            elif call_name == "assemble":
                call = lambda: store.assemble(starts, reuse_buffers=True)[0][1]
            elif std:
                call = lambda: (e.step_mse_series_std if spec.regression else e.step_ce_series_std)(store, starts, flat)[3]
            else:
                call = lambda: (e.step_mse_series if spec.regression else e.step_ce_series)(store, starts, flat)[3]
            for _ in range(WARM + ITERS):
                out = call()
            torch.cuda.synchronize()
            print(f"{name} {plan} {which} {call_name}: {WARM + ITERS} calls, sum {float(out.float().sum()):.6g}", flush=True)


def summarise(dirs, out_json):
    res = {}
    for d in dirs:
        k = kernel_ms(d)
        calls = WARM + ITERS
        res[os.path.basename(os.path.normpath(d))] = {"ms_per_call": sum(k.values()) / calls,
                                                      "kernels_ms_per_call": {n[:90]: v / calls for n, v in sorted(k.items(), key=lambda x: -x[1])}}
    txt = json.dumps(res, indent=1)
    print(txt)
    if out_json:
        open(out_json, "w").write(txt + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "summarise"])
    ap.add_argument("dirs", nargs="*")
    ap.add_argument("--store", default="orbit", choices=["orbit", "sibling"])
    ap.add_argument("--call", default="forward", choices=["forward", "step", "assemble"])
    ap.add_argument("--only", default=None, choices=list(CASES))
    ap.add_argument("--plan", default=None, choices=["bf16", "x3"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.mode == "run":
        run(a.store, a.call, a.only, [a.plan] if a.plan else ["bf16", "x3"])
    else:
        summarise(a.dirs, a.json)
