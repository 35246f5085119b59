"""Steps/s of the stochastic sampling loop (eta = 1) against the deterministic one (eta = 0), for the unconditional and the
masked (label-inference) sampler, in one process, alternating.

The benched sampler shape (BASELINE configs[4]: DiffusionTransformer, 4 layers, d_model 512, T = 200, D = 300, bf16) and
100 steps; the masked samplers observe every column but the last 30.  Each timed call is a whole `sample()` between two
device synchronisations; the order of the samplers rotates from one repetition to the next.  `uncond_eta0_b` is a second
eta = 0 sampler with its own capture of the same step, the A / A control: how far two identical captured loops differ on
the box.  One JSON line per batch size, then one summary line.

    python tools/eta_sampler_rate.py [--batches 1 16 256] [--reps 20] [--only cond_eta1]

`--only cond_eta1 --batches 256 --reps 1` (or `uncond_eta1`) is the form to run under
`rocprofv3 --kernel-trace --stats -- python ...`."""
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
NAMES = ["uncond_eta0", "uncond_eta0_b", "uncond_eta1", "cond_eta0", "cond_eta1"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["all"] + NAMES, default="all")
    a = ap.parse_args()
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler, DDIMSampler
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)                               # bench.py::build_model
    model = DiffusionTransformer(D, T, d_model=512, num_heads=8, dim_feedforward=2048, num_layers=4, device=dev,
                                 compute_dtype=torch.bfloat16)
    mask = torch.ones(T, D, dtype=torch.bool)
    mask[:, D - FREE:] = False
    summary = {"uncond": {}, "cond": {}, "a_over_a": {}}
    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        x_T = torch.randn(B, T, D, generator=g).to(torch.bfloat16).to(dev)
        obs = torch.randn(B, T, D, generator=g).to(dev)

        def make(name):
            eta = 1.0 if name.endswith("eta1") else 0.0
            if name.startswith("cond"):
                smp = ConditionalDDIMSampler(model, S, eta=eta, seed=1)
                return lambda: smp.sample(x_T, obs, mask)
            smp = DDIMSampler(model, S, eta=eta, seed=1)
            return lambda: smp.sample(x_T)

        names = NAMES if a.only == "all" else [a.only]
        runs = {k: make(k) for k in names}
        for fn in runs.values():                      # capture + warm-up
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
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
        if a.only == "all":
            rate = lambda k: line[f"{k}_steps_per_s"]
            line["uncond_eta1_over_eta0"] = summary["uncond"][B] = round(rate("uncond_eta1") / rate("uncond_eta0"), 4)
            line["cond_eta1_over_eta0"] = summary["cond"][B] = round(rate("cond_eta1") / rate("cond_eta0"), 4)
            line["uncond_eta0_b_over_eta0"] = summary["a_over_a"][B] = round(rate("uncond_eta0_b") / rate("uncond_eta0"), 4)
        print(json.dumps(line), flush=True)
    if a.only == "all":
        print(json.dumps({"eta1_over_eta0": summary, "target": 0.97}), flush=True)


if __name__ == "__main__":
    main()
