"""Device time of the standardisation's two sweeps over a window table (csrc/standardize.hip), as GB/s, next to
`ib_column_range` over the same table and the 6.0-6.3 TB/s an in-order sweep of HBM achieves on an MI355X.

A synthetic bf16 table of N windows of 50 x 300 values (DeviceMotionCache.synthetic; N = 65536 is 1.97 GB, far beyond the
256 MB Infinity Cache), three launches:
  moments   ib_column_moments_accum, MOMENTS_SLOTS workgroups: reads the table once
  affine    ib_column_affine in place, mode 0 with mean 0 and inv 1 (the identity: the table keeps its values): reads and
            writes the table once, so its bytes are twice the table's
  range     ib_column_range as hip.column_range launches it (both its launches): reads the table once
Each timed window is `--launches` launches of one kind between two HIP events on the launch stream; the kinds alternate,
the order rotates from one repetition to the next, the median over `--reps` windows is reported with its spread.  One JSON
line.

    python tools/standardize_rate.py [--windows 65536] [--launches 5] [--reps 7]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

T, D = 50, 300
SWEEP_TBS = (6.0, 6.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.data.WindowCache import DeviceMotionCache
    if not torch.cuda.is_available():
        raise SystemExit("standardize_rate: needs a GPU (a rate is a device time)")
    dev = torch.device("cuda", 0)
    cache = DeviceMotionCache.synthetic(a.windows, T, D, dev, torch.bfloat16, seed=1)
    table = cache.table
    table_bytes = table.numel() * table.element_size()
    shift = table[0, :D].to(torch.float32).contiguous()
    acc = hip.column_moments_acc(D, dev)
    zero, one = torch.zeros(D, device=dev), torch.ones(D, device=dev)
    out = torch.empty(D, 2, device=dev)
    kinds = {"moments": (lambda: hip.column_moments(table, T, D, shift, acc), table_bytes),
             "affine": (lambda: hip.column_affine(table, table, zero, one, mode=hip.STANDARDIZE, window=T), 2 * table_bytes),
             "range": (lambda: hip.column_range(table, T, D, out=out), table_bytes)}
    before = table[:64].clone()
    for fn, _ in kinds.values():                     # warm-up: code objects, the allocator
        fn()
    torch.cuda.synchronize()
    assert torch.equal(table[:64], before), "the identity affine must leave the table as it was"
    times = {k: [] for k in kinds}
    names = list(kinds)
    for r in range(a.reps):
        for k in names[r % len(names):] + names[:r % len(names)]:
            e0, e1 = hip.Event(), hip.Event()
            e0.record()
            for _ in range(a.launches):
                kinds[k][0]()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_ms(e1) / a.launches)
    line = {"windows": a.windows, "T": T, "D": D, "dtype": "bf16", "table_GB": round(table_bytes / 1e9, 3),
            "slots": hip.MOMENTS_SLOTS, "launches": a.launches, "reps": a.reps, "sweep_TBps_guide": list(SWEEP_TBS)}
    for k, ts in times.items():
        med = statistics.median(ts)
        line[f"{k}_ms"] = round(med, 4)
        line[f"{k}_GBps"] = round(kinds[k][1] / (med * 1e-3) / 1e9, 1)
        line[f"{k}_spread_pct"] = round(100 * (max(ts) - min(ts)) / med, 1)
    line["moments_over_range"] = round(line["moments_GBps"] / line["range_GBps"], 3)
    line["moments_share_of_sweep"] = round(line["moments_GBps"] / (1e3 * SWEEP_TBS[0]), 3)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
