"""Measure one training step of the MLP baselines on one GPU (reported, not gated; bench.py stays the project's benchmark).

Shapes: MiniCheetah (in = 150 x 54 = 8100, hidden 128, 8 layers, out 8, cross entropy) and A1 (in = 150 x 42 = 6300, hidden 128, 8 layers, out 4, MSE),
at 64 and 8192 windows.  Routes:
  (a) series   MLPEngine.step_*_series: the fused step straight from the resident series
  (b) dense    SequenceStore.assemble + MLPEngine.step_*: the fused step on materialised windows
  (c) ops      models.MLP at precision "f32": operator by operator on ops.linear (fp32 MFMA) with torch's loss and autograd -- what the package could already run
  (d) torch    nn.Sequential under bf16 autocast on assembled windows with torch's loss and backward
  (e) x3       SequenceStore.assemble (fp32 store) + MLPEngine("x3").step_*: the fused split-bf16 step on dense fp32 rows -- what models.MLP runs at the
               default precision, to be compared with (c), the route the same request took before
Every step is bracketed by HIP events on the stream; the `starts` rotate over resident index tensors, so no step re-reads the previous step's windows;
warm-up steps come first.  Prints one JSON line per (shape, batch)."""
import argparse
import json
import statistics
import sys
import os

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morphsym_hgnn_amd import engine, models, windows  # noqa: E402

DEV = "cuda:0"
JP, FP = list(range(12)), list(range(4))


def sequence(kind, n_rows, seed=0):
    g = np.random.default_rng(seed)
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    if kind == "minicheetah":
        return {"imu_acc": f(n_rows, 3), "imu_omega": f(n_rows, 3), "q": f(n_rows, 12), "qd": f(n_rows, 12), "p": f(n_rows, 12), "v": f(n_rows, 12),
                "contacts": g.integers(0, 2, (n_rows, 4)).astype(np.float32)}
    q = f(n_rows, 4); q[:, 3] += 4
    return {"imu_acc": f(n_rows, 3), "imu_omega": f(n_rows, 3), "q": f(n_rows, 12), "qd": f(n_rows, 12), "tau": f(n_rows, 12), "F": f(n_rows, 12), "r_o": q}


def timed(step, starts_list, steps, warmup):
    for i in range(warmup):
        step(starts_list[i % len(starts_list)])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for i, (a, b) in enumerate(ev):
        st = starts_list[(warmup + i) % len(starts_list)]
        a.record(); step(st); b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 8192])
    ap.add_argument("--routes", default="abcde")
    ap.add_argument("--shapes", nargs="+", default=["minicheetah", "a1"])
    args = ap.parse_args()
    for kind in args.shapes:
        ce = kind == "minicheetah"
        recipe = windows.minicheetah_mlp_recipe(JP, FP, 150) if ce else windows.quadsdk_a1_mlp_recipe(JP, FP, 150, 1)
        store = windows.SequenceStore(sequence(kind, args.rows), recipe, dtype="bf16", device=DEV)
        in_channels, out = recipe.width("mlp"), (8 if ce else 4)
        store32 = windows.SequenceStore(sequence(kind, args.rows), recipe, dtype="f32", device=DEV)
        e = engine.MLPEngine(in_channels, 128, out, 8, "bf16", DEV)
        e3 = engine.MLPEngine(in_channels, 128, out, 8, "x3", DEV)
        torch.manual_seed(0)
        m_ops = models.MLP(in_channels, 128, out, 8).to(DEV).set_precision("f32")
        m_torch = nn.Sequential(*[type(mod)(mod.in_features, mod.out_features) if isinstance(mod, nn.Linear) else nn.ReLU() for mod in m_ops]).to(DEV)
        flat = torch.cat([p.detach().reshape(-1) for p in m_ops.parameters()]).contiguous()
        for B in args.batches:
            gen = torch.Generator().manual_seed(B)
            starts_list = [torch.randint(0, len(store), (B,), generator=gen).to(DEV) for _ in range(8)]
            out_t, grad, loss = torch.empty(B, out, device=DEV), torch.empty(e.n_flat, device=DEV), torch.empty(1, device=DEV)
            lossf = (lambda o, y: nn.functional.cross_entropy(o.reshape(-1, 2).float(), (y.reshape(-1) != 0).long())) if ce else \
                (lambda o, y: nn.functional.mse_loss(o.float(), y))

            def a(st):
                (e.step_ce_series if ce else e.step_mse_series)(store, st, flat, out=out_t, grad_flat=grad, loss=loss)

            def b(st):
                xs, y, _ = store.assemble(st, reuse_buffers=True)
                if ce:
                    e.step_ce(xs[0], flat, (y != 0).to(torch.int32), out=out_t, grad_flat=grad, loss=loss)
                else:
                    e.step_mse(xs[0], flat, y, out=out_t, grad_flat=grad, loss=loss)

            def c(st):
                xs, y, _ = store.assemble(st, reuse_buffers=True)
                m_ops.zero_grad(set_to_none=True)
                lossf(m_ops(xs[0][:, :in_channels].float()), y).backward()

            def d(st):
                xs, y, _ = store.assemble(st, reuse_buffers=True)
                m_torch.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    o = m_torch(xs[0][:, :in_channels])
                lossf(o, y).backward()

            def x3(st):
                xs, y, _ = store32.assemble(st, reuse_buffers=True)
                if ce:
                    e3.step_ce(xs[0], flat, (y != 0).to(torch.int32), out=out_t, grad_flat=grad, loss=loss)
                else:
                    e3.step_mse(xs[0], flat, y, out=out_t, grad_flat=grad, loss=loss)

            res = {"shape": kind, "in": in_channels, "hidden": 128, "layers": 8, "out": out, "loss": "ce" if ce else "mse", "windows": B}
            for key, fn, name in (("a", a, "series"), ("b", b, "dense"), ("c", c, "ops"), ("d", d, "torch"), ("e", x3, "x3")):
                if key in args.routes:
                    med, best = timed(fn, starts_list, args.steps, args.warmup)
                    res[name + "_ms"], res[name + "_min_ms"], res[name + "_windows_per_s"] = round(med, 4), round(best, 4), round(B / med * 1e3)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
