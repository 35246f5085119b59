"""Steps/s of the benchmark's sampling loop with the x0 clip off, 'range' and 'dynamic' (diffusion/sampler.py, csrc/clip.hip),
in one process, alternating.

The flagship denoiser of the DDIM benchmark (DiffusionTransformer, 4 layers, d_model 512, D = 300, bf16) at T = 200, sampled
by the unmasked DDIMSampler as bench.py's DDIM leg does, so all 300 columns of all 200 frames are free: n = 60000 elements
per window, the largest selection `ib_x0_clip_dynamic` meets.  Every column is bounded at +-2 (an untrained denoiser's x0
leaves that range at the early steps, so the launch has stores to make).  Three loops per batch size B:
  off       x0_clip = None: the benchmark's loop, launch for launch
  range     one ib_x0_clip_range launch per step
  dynamic   one ib_x0_clip_dynamic launch per step (one workgroup per window: at B = 1 a single workgroup)
Each timed call is a whole `sample()` between two device synchronisations; the order rotates from one repetition to the next.
One JSON line per B.

    python tools/clip_rate.py [--batch 1 16 256] [--steps 100] [--reps 7]"""
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

T, D, BOUND = 200, 300, 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from inferbiomechanics_amd.diffusion.sampler import DDIMSampler, X0Clip
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = DiffusionTransformer(D, T, d_model=512, num_heads=8, dim_feedforward=2048, num_layers=4, device=dev,
                                 compute_dtype=torch.bfloat16)
    S = a.steps
    clip = lambda mode: X0Clip([-BOUND] * D, [BOUND] * D, mode=mode)
    for B in a.batch:
        z = torch.randn(B, T, D, generator=torch.Generator().manual_seed(B)).to(torch.bfloat16).to(dev)
        samplers = {"off": DDIMSampler(model, S), "range": DDIMSampler(model, S, x0_clip=clip("range")),
                    "dynamic": DDIMSampler(model, S, x0_clip=clip("dynamic"))}
        runs = {k: (lambda s=s: s.sample(z)) for k, s in samplers.items()}
        for fn in runs.values():                 # capture + warm-up
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
            line[f"{k}_ms_per_step"] = round(med * 1e3 / S, 4)
            line[f"{k}_steps_per_s"] = round(S / med, 1)
            line[f"{k}_spread_pct"] = round(100 * (max(ts) - min(ts)) / med, 1)
        for k in ("range", "dynamic"):
            line[f"{k}_over_off"] = round(line[f"{k}_steps_per_s"] / line["off_steps_per_s"], 4)
            line[f"{k}_extra_us_per_step"] = round((line[f"{k}_ms_per_step"] - line["off_ms_per_step"]) * 1e3, 1)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
