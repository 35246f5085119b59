"""Steps/s of the masked (label-inference) DDIM sampler against the unconditional one, in one process, alternating.

The benched sampler shape (BASELINE configs[4]: DiffusionTransformer, 4 layers, d_model 512, T = 200, D = 300, bf16) and
100 steps; the conditional sampler observes every column but the last 30 (the label block).  Each timed call is a whole
`sample()` (start-state copies, 100 graph replays, the result copy) between two device synchronisations; the order of
the samplers rotates from one repetition to the next.  A second unconditional sampler of its own (`uncond_b`: its own
capture of the same step) is the A / A control: how far two identical captured loops differ on the box.  One JSON line
per batch size, then one summary line.

    python tools/cond_sampler_rate.py [--batches 1 16 256] [--reps 20] [--only cond]

`--only cond --batches 256 --reps 1` is the form to run under `rocprofv3 --kernel-trace --stats -- python ...`."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

T, D, S, FREE = 200, 300, 100, 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["both", "cond", "uncond"], default="both")
    a = ap.parse_args()
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)                               # bench.py::build_model
    model = DiffusionTransformer(D, T, d_model=512, num_heads=8, dim_feedforward=2048, num_layers=4, device=dev,
                                 compute_dtype=torch.bfloat16)
    mask = torch.ones(T, D, dtype=torch.bool)
    mask[:, D - FREE:] = False
    summary = {}
    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        x_T = torch.randn(B, T, D, generator=g).to(torch.bfloat16).to(dev)
        obs = torch.randn(B, T, D, generator=g).to(dev)
        runs = {}
        if a.only in ("both", "uncond"):
            unc = DDIMSampler(model, S)
            runs["uncond"] = lambda: unc.sample(x_T)
        if a.only == "both":
            unc_b = DDIMSampler(model, S)
            runs["uncond_b"] = lambda: unc_b.sample(x_T)
        if a.only in ("both", "cond"):
            cond = ConditionalDDIMSampler(model, S)
            runs["cond"] = lambda: cond.sample(x_T, obs, mask)
        for fn in runs.values():                      # capture + warm-up
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        names = list(runs)
        for r in range(a.reps):
            for k in names[r % len(names):] + names[:r % len(names)]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runs[k]()
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
        line = {"B": B, "T": T, "D": D, "steps": S, "reps": a.reps}
        for k, ts in times.items():
            med = statistics.median(ts)
            line[f"{k}_ms"] = round(med * 1e3, 3)
            line[f"{k}_steps_per_s"] = round(S / med, 1)
            line[f"{k}_spread_pct"] = round(100 * (max(ts) - min(ts)) / med, 1)
        if a.only == "both":
            line["cond_over_uncond"] = round(line["cond_steps_per_s"] / line["uncond_steps_per_s"], 4)
            line["uncond_b_over_uncond"] = round(line["uncond_b_steps_per_s"] / line["uncond_steps_per_s"], 4)
            summary[B] = line["cond_over_uncond"]
        print(json.dumps(line), flush=True)
    if summary:
        print(json.dumps({"cond_over_uncond": summary, "target": 0.97}), flush=True)


if __name__ == "__main__":
    main()
