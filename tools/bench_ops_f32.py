"""Measure the fp32 operator mshgnn_op_gemm (csrc/mshgnn_ops.hip, k_op_gemm) at the GEMM shapes of tests/test_ops_gpu.py, y = x W^T + b: reported, not gated.
The fp32 counterpart of tools/bench_ops_f64.py and its method: 10 warm-up and 40 timed launches, each bracketed by HIP events, the median and the minimum; the operands
rotate over enough buffer sets (>= 1 GB in all, at most 64 sets) that a launch never finds its operands in the last-level cache from the launch before.  One JSON line per
shape; --out writes the same lines to a file.  MSHGNN_LIB selects another build of the library (A/B runs: alternate fresh processes)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_ops_f64 import DEV, timed  # noqa: E402
from morphsym_hgnn_amd import ops  # noqa: E402

SHAPES = [(1, 7, 5), (50, 450, 128), (3000, 900, 128), (257, 128, 3), (70000, 128, 128)]      # (M, K, N) of tests/test_ops_gpu.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for M, K, N in SHAPES:
        gen = torch.Generator().manual_seed(M + K)
        n_sets = min(64, max(2, -(-(1 << 30) // (4 * (M * K + N * K + N + M * N)))))
        A = [torch.randn(M, K, generator=gen).to(DEV) for _ in range(n_sets)]
        W = [torch.randn(N, K, generator=gen).to(DEV) for _ in range(n_sets)]
        b = [torch.randn(N, generator=gen).to(DEV) for _ in range(n_sets)]
        C = [torch.empty(M, N, device=DEV) for _ in range(n_sets)]

        def ours(i):
            ops.gemm(A[i], K, 1, W[i], K, 1, M, N, K, bias=b[i], out=C[i], dtype=torch.float32)

        med, best = timed(ours, n_sets, args.steps, args.warmup)
        ref = torch.addmm(b[0].double(), A[0].double(), W[0].double().t())
        ours(0)
        torch.cuda.synchronize()
        res = {"what": "gemm_f32", "M": M, "K": K, "N": N, "buffer_sets": n_sets, "f32_us": round(med * 1e3, 2), "f32_min_us": round(best * 1e3, 2),
               "max_abs_diff_to_fp64": float((C[0].double() - ref).abs().max())}
        print(json.dumps(res), flush=True)
        lines.append(res)
        del A, W, b, C
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
