#!/usr/bin/env python3
"""Denoiser evaluations per second of the resampled masked loop next to the plain masked loop, in one process, alternating,
at the shape of bench.py's configs[4] (the T = 200 transformer denoiser, B = 16 windows, D = 300, bf16, 100 sampling steps,
the captured step replayed).  Resampling adds two small launches (ib_resample_renoise, ib_counter_add) per `jump` evaluations
and nothing else, so the cost per evaluation is expected within run-to-run noise of the plain loop's; this measures it.

Both loops run on ONE sampler object (the same buffers and the same captured step: `resample` is switched between calls), each
once untimed, then `--rounds` times alternating, a host clock around a call that ends in a device synchronise.  Printed: one
JSON line with the evaluations per second of every timed call, the medians and their ratio.  Needs a GPU.

  python tools/resample_rate.py [--rounds 5] [--jump 10] [--times 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--jump", type=int, default=10)
    ap.add_argument("--times", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("resample_rate measures on the GPU: none found")
    import bench
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    from inferbiomechanics_amd.diffusion.schedule import resample_evaluations
    B, T, D, S = 16, 200, 300, 100
    dev = torch.device("cuda", 0)
    model = bench.build_model("transformer", T, D, torch.bfloat16, dev)
    sampler = ConditionalDDIMSampler(model, S, use_graph=True, seed=1)
    g = torch.Generator().manual_seed(0)
    z, obs = torch.randn(B, T, D, generator=g).to(dev), torch.randn(B, T, D, generator=g).to(dev)
    mask = torch.ones(T, D, dtype=torch.bool)
    mask[:, D - 30:] = False                                           # the label columns are free
    loops = {"plain": (None, S), "resampled": ((a.jump, a.times), resample_evaluations(S, a.jump, a.times))}

    def run(name):
        sampler.resample = loops[name][0]
        t0 = time.perf_counter()
        sampler.sample(z, obs, mask)
        torch.cuda.synchronize()
        return loops[name][1] / (time.perf_counter() - t0)

    for name in loops:                                                 # untimed: buffers, tables, the capture
        run(name)
    rates = {name: [] for name in loops}
    for _ in range(a.rounds):
        for name in loops:
            rates[name].append(run(name))
    med = {name: statistics.median(v) for name, v in rates.items()}
    out = {"workload": f"transformer_denoiser_T{T} B={B} masked {S}-step DDIM, resample=({a.jump}, {a.times})",
           "evaluations": {name: loops[name][1] for name in loops},
           "evaluations_per_sec": {name: [round(r, 1) for r in v] for name, v in rates.items()},
           "median": {name: round(m, 1) for name, m in med.items()},
           "spread": {name: round((max(v) - min(v)) / med[name], 4) for name, v in rates.items()},
           "resampled_over_plain": round(med["resampled"] / med["plain"], 4)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
