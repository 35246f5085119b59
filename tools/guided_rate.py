"""Steps/s of the guided sampling loop (classifier-free guidance, diffusion/sampler.py) against the unguided loop, in one
process, alternating.

The flagship denoiser of the DDIM benchmark (DiffusionTransformer, 4 layers, d_model 512, D = 300, bf16) at T = 200, with
cond_cols = 270 and cond_drop set, sampled by ConditionalDDIMSampler with observations = 'clean'.  Three loops per batch size B:
  guided        guidance = 1.5 at B windows: one denoiser evaluation over 2B windows per step + ib_cfg_combine + ib_cfg_mirror
  unguided      the same sampler without guidance at B windows
  unguided_2B   without guidance at 2B windows: the denoiser evaluation the guided loop pays for, without the seam
The expectation is guided = unguided_2B minus the two seam launches.  Each timed call is a whole `sample()` between two device
synchronisations; the order rotates from one repetition to the next.  One JSON line per B.  --no-guided leaves the guided loop
out, so the same file measures a tree that has no `guidance` keyword yet.

    python tools/guided_rate.py [--batch 16 256] [--steps 50] [--reps 7] [--no-guided]"""
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

T, D, FREE, G = 200, 300, 30, 1.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-guided", action="store_true")
    a = ap.parse_args()
    from inferbiomechanics_amd.diffusion.sampler import ConditionalDDIMSampler
    from inferbiomechanics_amd.models.DiffusionDenoisers import DiffusionTransformer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = DiffusionTransformer(D, T, d_model=512, num_heads=8, dim_feedforward=2048, num_layers=4, device=dev,
                                 compute_dtype=torch.bfloat16)
    model.cond_cols, model.cond_drop = D - FREE, 0.1
    mask = torch.zeros(T, D, dtype=torch.bool)
    mask[:, :D - FREE] = True
    S = a.steps
    for B in a.batch:
        g = torch.Generator().manual_seed(B)
        z = torch.randn(2 * B, T, D, generator=g).to(torch.bfloat16).to(dev)
        obs = torch.randn(2 * B, T, D, generator=g).to(dev)
        plain, plain2 = (ConditionalDDIMSampler(model, S, observations="clean") for _ in range(2))
        runs = {"unguided": lambda: plain.sample(z[:B], obs[:B], mask), "unguided_2B": lambda: plain2.sample(z, obs, mask)}
        if not a.no_guided:
            guided = ConditionalDDIMSampler(model, S, observations="clean", guidance=G)
            runs["guided"] = lambda: guided.sample(z[:B], obs[:B], mask)
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
        line = {"B": B, "T": T, "D": D, "cond_cols": D - FREE, "steps": S, "reps": a.reps}
        for k, ts in times.items():
            med = statistics.median(ts)
            line[f"{k}_ms_per_step"] = round(med * 1e3 / S, 4)
            line[f"{k}_steps_per_s"] = round(S / med, 1)
            line[f"{k}_spread_pct"] = round(100 * (max(ts) - min(ts)) / med, 1)
        if "guided" in times:
            line["guided_over_unguided_2B"] = round(line["guided_steps_per_s"] / line["unguided_2B_steps_per_s"], 4)
            line["guided_over_unguided"] = round(line["guided_steps_per_s"] / line["unguided_steps_per_s"], 4)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
