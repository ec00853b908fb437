"""The three launches of csrc/mshgnn_orbit.hip alone, timed with HIP events: K = 4 (the A1 'fs' tables under gs / gt / gr), 8192 base windows, 12 units of width 1,
rotating over three buffer sets; 10 warm-up + 40 timed launches each, median (min .. max) in microseconds.  Event pairs around one launch include the launch
gap, so these are upper bounds of the kernel durations.

    python tools/orbit_average_cost.py [--out profiles/orbit_average_cost.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from morphsym_hgnn_amd import symmetrise as sym          # noqa: E402
from morphsym_hgnn_amd.windows import GroupAction        # noqa: E402

K, B, U = 4, 8192, 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = GroupAction.load("a1-c2")
    tabs = [g.table("fs", op) for op in ("gs", "gt", "gr")]
    act = sym.OutputAction.from_tables([list(range(U))] + [t[0] for t in tabs], [[1] * U] + [t[1] for t in tabs], 1, [None, "gs", "gt", "gr"])
    bufs = [(torch.randn(K * B, U, device="cuda"), torch.empty(B, U, device="cuda"), torch.randn(B, U, device="cuda"), torch.empty(K * B, U, device="cuda"),
             torch.zeros(K, 4, dtype=torch.float64, device="cuda")) for _ in range(3)]
    res = {"elements": K, "base_windows": B, "units": U, "width": 1, "warmup": 10, "timed": 40}
    for name, pick in (("mshgnn_orbit_average", lambda b: (b[0], b[1])), ("mshgnn_orbit_average_backward", lambda b: (b[2], b[3])),
                       ("mshgnn_orbit_defect", lambda b: (b[0], b[4]))):
        times = []
        for i in range(50):
            src, dst = pick(bufs[i % 3])
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            sym._launch(name, act, src, B, dst)
            t1.record()
            t1.synchronize()
            if i >= 10:
                times.append(t0.elapsed_time(t1) * 1e3)
        res[name] = {"median_us": round(statistics.median(times), 2), "min_us": round(min(times), 2), "max_us": round(max(times), 2)}
        print(f"{name}: median {res[name]['median_us']} us ({res[name]['min_us']} .. {res[name]['max_us']})")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
