#!/usr/bin/env python3
"""Device time of the ensemble reductions at the label predictor's shape, in one process, alternating: ib_ensemble_order over
the 30 label columns of an ensemble [256, 8, 50, 300] (256 windows, K = 8 members, 50 frames, 300 columns), scored, bf16 and
fp32, next to ib_ensemble_stats over the whole rows of the same tensor, which is what the predictor runs before it.

ib_ensemble_order reads only the label block: 60 of every 600 bytes of a bf16 row, so at most one 64-byte sector in ten is
touched and the sectors it touches are used in part.  Printed per launch: the median device time, the spread over the rounds
and the achieved bytes per second against the bytes the launch NEEDS (the label block's members, the truth and the outputs
for ib_ensemble_order; the whole tensor and both outputs for ib_ensemble_stats) -- not the sectors moved.

Each launch is timed by hip.time_recorded_call: `--reps` launches captured in a graph and replayed between two device events.
One JSON line.  Needs a GPU.

  python tools/ensemble_rate.py [--rounds 7] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, K, ROWS, LD, W = 256, 8, 50, 300, 30
LEVEL = 0.8


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_rate measures on the GPU: none found")
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd.diffusion.ensemble import interval_levels, quantile_position
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x32 = torch.randn(B, K, ROWS, LD, generator=g)
    y = torch.randn(B, ROWS, W, generator=g).to(dev)
    pos = [quantile_position(q, K) for q in interval_levels(LEVEL)]
    n = B * ROWS * W
    f = lambda: torch.empty(n, dtype=torch.float32, device=dev)
    u = lambda: torch.empty(n, dtype=torch.uint8, device=dev)
    outs = (f(), f(), f(), f(), u(), u())
    mean, std = (torch.empty(B * ROWS * LD, dtype=torch.float32, device=dev) for _ in range(2))
    calls = {}
    for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        x = x32.to(dt).to(dev)
        e = x.element_size()
        calls[f"ensemble_order_{name}"] = (
            "ib_ensemble_order",
            (x.data_ptr(), y.data_ptr(), *(t.data_ptr() for t in outs), B, K, ROWS, LD, LD - W, W, pos[0][0], pos[0][1],
             pos[1][0], pos[1][1], pos[2][0], pos[2][1], hip.dtype_code(dt), None),
            n * (K * e + 4 + 4 * 4 + 2), x)
        calls[f"ensemble_stats_{name}"] = (
            "ib_ensemble_stats", (x.data_ptr(), mean.data_ptr(), std.data_ptr(), B, K, ROWS * LD, hip.dtype_code(dt), None),
            B * ROWS * LD * (K * e + 8), x)
    us = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, (entry, args, _, _) in calls.items():
            us[name].append(hip.time_recorded_call(entry, args, reps=a.reps, rounds=3))
    med = {name: statistics.median(v) for name, v in us.items()}
    out = {"workload": f"ensemble [{B}, {K}, {ROWS}, {LD}], label columns ({LD - W}, {W}), level {LEVEL}, scored",
           "device_us": {name: [round(t, 2) for t in v] for name, v in us.items()},
           "median_us": {name: round(m, 2) for name, m in med.items()},
           "spread": {name: round((max(v) - min(v)) / med[name], 4) for name, v in us.items()},
           "needed_bytes": {name: c[2] for name, c in calls.items()},
           "needed_GB_per_s": {name: round(c[2] / med[name] * 1e-3, 1) for name, c in calls.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
