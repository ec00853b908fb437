"""Cost of the input gradients (mshgnn_input_grad) on the flagship shape: A1-C2, L = 3, 8192 windows, bf16 and split (x3) plans.

Per plan, HIP-event times (median of --reps) of
  fwd_bwd        training forward + mshgnn_backward (the two-call route the module takes)
  fwd_bwd_ig32   the same + mshgnn_input_grad into fp32 rows at the reference's width (all three types)
  fwd_bwd_ig64   the same into fp64 rows (the reference's own input dtype, gnnLightning.py:1183)
  ig32 / ig64    mshgnn_input_grad alone (behind a backward), with the bytes it moves and the rate that makes
  bwd / bwd_frozen  mshgnn_backward with / without the weight-gradient and finalize launches (grad_params = NULL)
One JSON line per plan.  Usage: python tools/input_grad_cost.py [--windows 8192] [--reps 20]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from morphsym_hgnn_amd import engine as eng, synth  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    B = args.windows
    spec = bench.build_spec(3, "a1c2")
    g = torch.Generator(device="cuda").manual_seed(0)
    x_dict = {t: torch.randn(B * spec.num_nodes[t], spec.widths[t], generator=g, device="cuda") for t in spec.node_types}
    params = synth.make_params(0, spec.param_shapes())
    for plan in ("bf16", "x3"):
        e = eng.Engine(spec, plan, device="cuda:0")
        xs = e.cast_inputs(x_dict)
        flat = eng.flatten_params(spec, params, device=e.device)
        out = e.forward(xs, flat, B, training=True)
        gout = torch.randn(out.numel(), generator=g, device="cuda")
        gflat = torch.empty(spec.flat_size(), dtype=torch.float32, device="cuda")
        _, need = spec.node_liveness()
        enc_nodes = sum(len(need[0][t]) for t in spec.node_types)
        bytes_dy = enc_nodes * B * spec.hidden * (2 if plan == "bf16" else 4)
        out_elems = sum(B * spec.num_nodes[t] * spec.widths[t] for t in spec.node_types)

        def fb():
            e.forward(xs, flat, B, training=True)
            e.backward(xs, flat, gout, B, grad_flat=gflat)

        def fb_ig(dt):
            def f():
                fb()
                e.input_grad(B, flat, dtype=dt)
            return f

        def bwd():
            e.backward(xs, flat, gout, B, grad_flat=gflat)

        def bwd_frozen():
            e.backward(xs, flat, gout, B, weights=False)

        def ig(dt):
            return lambda: e.input_grad(B, flat, dtype=dt)

        for f in (fb, fb_ig(torch.float32), fb_ig(torch.float64)):      # warm-up (allocator, first-use tables)
            f()
        torch.cuda.synchronize()
        r = {"plan": plan, "windows": B, "layers": 3, "unit": "us"}
        r["fwd_bwd"] = timed(fb, args.reps)
        r["fwd_bwd_ig32"] = timed(fb_ig(torch.float32), args.reps)
        r["fwd_bwd_ig64"] = timed(fb_ig(torch.float64), args.reps)
        fb()
        r["bwd"] = timed(bwd, args.reps)
        r["bwd_frozen"] = timed(bwd_frozen, args.reps)
        for name, dt, eb in (("ig32", torch.float32, 4), ("ig64", torch.float64, 8)):
            t_us = timed(ig(dt), args.reps)
            mb = (bytes_dy + out_elems * eb) / 1e6
            r[name] = t_us
            r[name + "_MB"] = round(mb, 1)
            r[name + "_TBps"] = round(mb / t_us, 2)      # MB / us = TB / s
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
