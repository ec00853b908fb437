"""Measure the fp64 operators (csrc/mshgnn_ops.hip) on one GPU: reported, not gated; bench.py stays the project's benchmark.

1. mshgnn_op_gemm_f64 on the three products of the model at 8192 A1 windows (12 joints: 98 304 rows):
     98 304 x 128 x 450   (the joint encoder, y = x W^T + b)
     98 304 x 128 x 128   (a GraphConv's lin_rel / lin_root)
     128 x 128 x 98 304   (their weight gradient dY^T X: column-major operands, split-K)
   each against torch.matmul in fp64 on the SAME buffers and against the fp32 mshgnn_op_gemm on fp32 copies.
2. An A1-C2 L=3 forward and forward+backward at 1024 windows at precision "f64" (models.set_precision), in windows/s.  The figure to put it next to
   is `cpu_baseline` of `bench.py --full` (the fp64 oracle port on the host: DESIGN.md, cited there, not re-measured here).

Every timed call is bracketed by HIP events on the stream: 10 warm-up and 40 timed launches, the median (and the minimum).  The operands ROTATE over
enough buffer sets that a launch never finds its operands in the 256 MB last-level cache from the launch before (sets x bytes per set >= 1 GB).
FLOP = 2 M N K.  The fp64 matrix peak used for the share is AMD's public figure for the MI355X, 78.6 TFLOP/s (FP64 matrix), named as such in the output.  Prints one JSON line per measurement; --out writes the same lines to a file."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morphsym_hgnn_amd import ops  # noqa: E402

DEV = "cuda:0"
FP64_MATRIX_PEAK_TF = 78.6      # AMD's public MI355X figure
GEMMS = [      # (name, M, N, K, A layout, B layout): "row" = [rows, K] row-major, "col" = [K, rows] row-major (the weight gradient's operands)
    ("encoder 98304x128x450", 98304, 128, 450, "row", "row"),
    ("conv    98304x128x128", 98304, 128, 128, "row", "row"),
    ("wgrad   128x128x98304", 128, 128, 98304, "col", "col"),
]


def timed(fn, n_sets, steps, warmup):
    for i in range(warmup):
        fn(i % n_sets)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for i, (a, b) in enumerate(ev):
        a.record(); fn((warmup + i) % n_sets); b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms)


def operand(rows, K, layout, dtype, gen):
    t = torch.randn(rows, K, generator=gen, dtype=torch.float32).to(dtype)
    return (t.contiguous() if layout == "row" else t.t().contiguous()).to(DEV)


def strides(rows, K, layout):
    return (K, 1) if layout == "row" else (1, rows)


def logical(buf, layout):
    return buf if layout == "row" else buf.t()


def bench_gemms(steps, warmup, emit):
    for name, M, N, K, la, lb in GEMMS:
        gen = torch.Generator().manual_seed(M + K)
        per_set = 8 * (M * K + N * K + M * N)
        n_sets = max(2, -(-(1 << 30) // per_set))
        A64 = [operand(M, K, la, torch.float64, gen) for _ in range(n_sets)]
        B64 = [operand(N, K, lb, torch.float64, gen) for _ in range(n_sets)]
        C64 = [torch.empty(M, N, dtype=torch.float64, device=DEV) for _ in range(n_sets)]
        (sAm, sAk), (sBn, sBk) = strides(M, K, la), strides(N, K, lb)

        def ours(i):
            ops.gemm(A64[i], sAm, sAk, B64[i], sBn, sBk, M, N, K, out=C64[i], dtype=torch.float64)

        def torch64(i):
            torch.matmul(logical(A64[i], la), logical(B64[i], lb).t(), out=C64[i])

        flop = 2.0 * M * N * K
        res = {"what": "gemm", "shape": name.strip(), "M": M, "N": N, "K": K, "buffer_sets": n_sets}
        med, best = timed(ours, n_sets, steps, warmup)
        check = C64[0].clone()
        res.update(f64_ms=round(med, 4), f64_min_ms=round(best, 4), f64_tflops=round(flop / med / 1e9, 2),
                   f64_share_of_public_peak=round(flop / med / 1e9 / FP64_MATRIX_PEAK_TF, 3))
        med, best = timed(torch64, n_sets, steps, warmup)
        res.update(torch_f64_ms=round(med, 4), torch_f64_min_ms=round(best, 4), torch_f64_tflops=round(flop / med / 1e9, 2))
        res["max_rel_diff_to_torch"] = float((C64[0] - check).abs().max() / C64[0].abs().max())      # (set 0 was last written by torch: warmup + steps = 50, even)
        del C64
        A32, B32 = [a.float() for a in A64], [b.float() for b in B64]
        del A64, B64
        C32 = [torch.empty(M, N, dtype=torch.float32, device=DEV) for _ in range(n_sets)]

        def ours32(i):
            ops.gemm(A32[i], sAm, sAk, B32[i], sBn, sBk, M, N, K, out=C32[i], dtype=torch.float32)

        med, best = timed(ours32, n_sets, steps, warmup)
        res.update(f32_ms=round(med, 4), f32_min_ms=round(best, 4), f32_tflops=round(flop / med / 1e9, 2))
        emit(res)
        del A32, B32, C32
        torch.cuda.empty_cache()


def bench_model(steps, warmup, emit, B=1024):
    import bench
    from morphsym_hgnn_amd import models
    from tests import helpers
    from tests.test_models import _build
    torch.set_default_dtype(torch.float64)
    spec = bench.build_spec(3, "a1c2")
    case = dict(kind="c2", cfg="a1-c2", hidden=spec.hidden, layers=3, regression=True, grf=3)
    m = _build(case, spec).set_precision("f64").to(DEV)
    n_sets = 4
    sets = []
    for s in range(n_sets):
        x_dict, y, _ = helpers.random_case(spec, B, seed=s)
        sets.append(({k: v.to(DEV) for k, v in x_dict.items()}, y.to(DEV)))
    ei = {k: v.to(DEV) for k, v in spec.topology.edge_index_dict(B).items()}
    with torch.no_grad():
        m(x_dict=sets[0][0], edge_index_dict=ei)
    assert isinstance(m, models._MSHGNNBase) and not m._engines

    def fwd(i):
        with torch.no_grad():
            m(x_dict=sets[i][0], edge_index_dict=ei)

    def fwd_bwd(i):
        m.zero_grad(set_to_none=True)
        out = m(x_dict=sets[i][0], edge_index_dict=ei)
        ((out.reshape(B, -1) - sets[i][1]) ** 2).mean().backward()

    for name, fn in (("forward", fwd), ("forward+backward", fwd_bwd)):
        med, best = timed(fn, n_sets, steps, warmup)
        emit({"what": "model", "model": "A1-C2 L3 h%d" % spec.hidden, "precision": "f64", "route": name, "windows": B, "ms": round(med, 3), "min_ms": round(best, 3),
              "windows_per_s": round(B / med * 1e3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ops_f64 needs a HIP device: a CPU run gives no time")
    lines = []

    def emit(res):
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

    emit({"what": "setup", "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "fp64_matrix_peak_tflops_public_figure": FP64_MATRIX_PEAK_TF})
    bench_gemms(args.steps, args.warmup, emit)
    if not args.skip_model:
        bench_model(args.steps, args.warmup, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
