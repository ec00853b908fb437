"""What the flat optimizers and gradient clipping cost per call, beside mshgnn_adam_step on the same buffers and beside torch's per-tensor code they replace.

  * at n = 996 227, 2 312 067 and 16 438 787 (the parameter counts of DESIGN section 1): mshgnn_sgd_step (plain / momentum / nesterov + weight decay),
    mshgnn_adamw_step (decoupled, coupled, and with step count + lr on the device), mshgnn_grad_norm, mshgnn_grad_clip, mshgnn_grad_norm + mshgnn_grad_clip,
    and mshgnn_adam_step -- device events around at least 0.5 s of back-to-back calls each, the launches ALTERNATING in rounds (every round times every
    launch once), medians and min-max over the rounds;
  * on an A1-C2 L=3 model (84 parameter tensors): torch.optim.SGD / AdamW .step() and torch.nn.utils.clip_grad_norm_ on the views against FlatSGD / FlatAdamW
    .step() and optim.clip_grad_norm_, wall clock per call (these are host-bound);
  * the B = 32 wrapper step replayed from one HIP graph with FlatSGD(momentum) against FlatAdam.

The whole run repeats in a second, fresh process (`--child` is that process); both land in profiles/flat_optim_cost.json.
usage: python tools/flat_optim_cost.py [--rounds 5] [--out profiles/flat_optim_cost.json]"""
import argparse, json, os, statistics, subprocess, sys, time, types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (996227, 2312067, 16438787)


def _summary(xs):
    return {"median_us": round(statistics.median(xs), 3), "min_us": round(min(xs), 3), "max_us": round(max(xs), 3), "rounds": len(xs)}


def _device_time(fn, seconds=0.5):
    """us per call: device events around enough back-to-back calls to fill `seconds`."""
    import torch
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    calls = max(200, int(seconds / max((time.perf_counter() - t0) / 50, 1e-7)))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def _wall_time(fn, n=200):
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def launches(n, dev):
    import torch
    from morphsym_hgnn_amd import engine as eng
    lib = eng.load_library()
    gen = torch.Generator().manual_seed(n)
    p, m, v, buf = (torch.randn(n, generator=gen).to(dev) * 1e-2 for _ in range(4))
    v = v.abs()
    g = torch.randn(n, generator=gen).to(dev) * 1e-3
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    lr_dev = torch.full((1,), 1e-6, dtype=torch.float32, device=dev)
    norm = torch.zeros(1, dtype=torch.float64, device=dev)
    scratch = torch.zeros((lib.mshgnn_grad_norm_scratch_bytes(n) + 7) // 8, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    P, G, M, V, B = (t.data_ptr() for t in (p, g, m, v, buf))
    keep = (p, g, m, v, buf, count, lr_dev, norm, scratch)
    lr = 1e-6      # (small: hundreds of thousands of steps must not drive the buffers to infinity)
    return keep, {
        "adam_step (parent's kernel)": lambda: lib.mshgnn_adam_step(P, G, M, V, n, 5, lr, 0.9, 0.999, 1e-8, 1.0, st),
        "adamw_step decoupled": lambda: lib.mshgnn_adamw_step(P, G, M, V, n, 5, None, lr, None, 0.9, 0.999, 1e-8, 1e-2, 1, 1.0, st),
        "adamw_step coupled": lambda: lib.mshgnn_adamw_step(P, G, M, V, n, 5, None, lr, None, 0.9, 0.999, 1e-8, 1e-2, 0, 1.0, st),
        "adamw_step decoupled, device count + lr": lambda: lib.mshgnn_adamw_step(P, G, M, V, n, 0, count.data_ptr(), lr, lr_dev.data_ptr(), 0.9, 0.999, 1e-8,
                                                                                  1e-2, 1, 1.0, st),
        "sgd_step plain": lambda: lib.mshgnn_sgd_step(P, G, None, n, 5, None, lr, None, 0.0, 0.0, 0.0, 0, 1.0, st),
        "sgd_step momentum": lambda: lib.mshgnn_sgd_step(P, G, B, n, 5, None, lr, None, 0.9, 0.0, 0.0, 0, 1.0, st),
        "sgd_step nesterov + weight decay": lambda: lib.mshgnn_sgd_step(P, G, B, n, 5, None, lr, None, 0.9, 0.0, 1e-3, 1, 1.0, st),
        "grad_norm": lambda: lib.mshgnn_grad_norm(G, n, norm.data_ptr(), scratch.data_ptr(), st),
        "grad_clip": lambda: lib.mshgnn_grad_clip(G, n, norm.data_ptr(), 1e30, st),
        "grad_norm + grad_clip": lambda: (lib.mshgnn_grad_norm(G, n, norm.data_ptr(), scratch.data_ptr(), st), lib.mshgnn_grad_clip(G, n, norm.data_ptr(), 1e30, st)),
    }


def wrapper_pair(dev, B, optimizer, graph_safe, **flat_kw):
    import torch
    import bench
    from morphsym_hgnn_amd import optim, synth, wrappers
    from morphsym_hgnn_amd.checkpoint import load_into
    spec = bench.build_spec(3)
    cfg = os.path.join(ROOT, "morphsym_hgnn_amd", "cfg", "a1-c2.yaml")
    x, y = bench.make_batch(spec, B, 5)
    x64 = {k: v.to(dev, torch.float64) for k, v in x.items()}
    ei = spec.topology.edge_index_dict(B, device=dev)
    os.environ["MSHGNN_DTYPE"] = "bf16"
    w = wrappers.HGNN_C2_Lightning_Reg(spec.hidden, spec.num_layers, spec.topology.metadata(), types.SimpleNamespace(x_dict=dict(x64), edge_index_dict=ei),
                                       lr=1e-4, symmetry_mode="MorphSym", group_operator_path=cfg)
    load_into(w.model, {"state_dict": {"model." + k: v for k, v in synth.make_params(0, spec.param_shapes()).items()}})
    w.model.set_precision("bf16"); w.to(dev)
    batch = types.SimpleNamespace(x_dict=dict(x64), edge_index_dict=ei, y=y.to(dev, torch.float64).view(B, -1), batch_size=B)
    opt = {"adam": optim.FlatAdam, "adamw": optim.FlatAdamW, "sgd": optim.FlatSGD}[optimizer](w.model, lr=1e-4, graph_safe=graph_safe, **flat_kw)
    return w, opt, batch


def child(rounds):
    import torch
    from morphsym_hgnn_amd import optim, wrappers
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "launch_us": {}, "model_84_tensors_wall_us": {}, "replayed_wrapper_step_B32_us": {}}
    for n in SIZES:
        keep, fns = launches(n, dev)
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                times[k].append(_device_time(fn))
        res["launch_us"][str(n)] = {k: _summary(v) for k, v in times.items()}
        del keep, fns
        torch.cuda.empty_cache()
    prev = torch.get_default_dtype(); torch.set_default_dtype(torch.float64)
    try:
        # torch's per-tensor code on the 84 views against the flat route, one model each
        for name, optimizer, kw, torch_cls in (("SGD(momentum=0.9)", "sgd", dict(momentum=0.9), torch.optim.SGD), ("AdamW", "adamw", {}, torch.optim.AdamW)):
            w, flat_opt, batch = wrapper_pair(dev, 32, optimizer, False, **kw)
            w.training_step(batch, 0).backward()
            t_opt = torch_cls(w.model.parameters(), lr=1e-6, **kw)
            flat_opt.param_groups[0]["lr"] = 1e-6
            a, b = [], []
            for _ in range(rounds):
                a.append(_wall_time(t_opt.step)); b.append(_wall_time(flat_opt.step))
            res["model_84_tensors_wall_us"][f"torch.optim.{name}.step"] = _summary(a)
            res["model_84_tensors_wall_us"][f"Flat{name}.step"] = _summary(b)
            if optimizer == "sgd":
                a, b = [], []
                for _ in range(rounds):
                    a.append(_wall_time(lambda: torch.nn.utils.clip_grad_norm_(w.model.parameters(), 1e30)))
                    b.append(_wall_time(lambda: optim.clip_grad_norm_(w.model, 1e30)))
                res["model_84_tensors_wall_us"]["torch.nn.utils.clip_grad_norm_"] = _summary(a)
                res["model_84_tensors_wall_us"]["optim.clip_grad_norm_"] = _summary(b)
        graphs = {}
        for name, optimizer, kw in (("FlatAdam", "adam", {}), ("FlatSGD(momentum=0.9)", "sgd", dict(momentum=0.9)),
                                    ("FlatSGD(momentum=0.9, device_lr) + max_grad_norm", "sgd", dict(momentum=0.9, device_lr=True))):
            w, opt, batch = wrapper_pair(dev, 32, optimizer, True, **kw)
            graphs[name] = wrappers.GraphedTrainingStep(w, opt, batch, max_grad_norm=1e30 if "max_grad_norm" in name else None)
        times = {k: [] for k in graphs}
        for _ in range(rounds):
            for k, gs in graphs.items():
                times[k].append(_wall_time(gs, 300))
        res["replayed_wrapper_step_B32_us"] = {k: _summary(v) for k, v in times.items()}
    finally:
        torch.set_default_dtype(prev)
    print("__RESULT__" + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_optim_cost.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.rounds)
    runs = []
    for k in range(2):      # two fresh processes, one after the other
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds)], capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("__RESULT__")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"process {k + 1} failed ({r.returncode})")
        runs.append(json.loads(line[0][len("__RESULT__"):]))
    out = {"what": __doc__.split("\n\n")[0], "bytes_per_element": {"sgd plain": 12, "sgd momentum": 20, "adamw": 28, "adam": 28, "grad_norm": 4, "grad_clip": 8},
           "processes": runs}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["processes"][0]["launch_us"], indent=1))


if __name__ == "__main__":
    main()
