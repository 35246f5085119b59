"""Cost of the learning-rate schedule in the training step: the graph-replayed step of HipTrainer with the schedule off and
on (cosine, warmup 100, total 10^6, min ratio 0.1), in one process, alternating.

Two configurations: the headline transformer denoiser (BASELINE configs[2]: 4 layers, d_model 512, T = 50, D = 300,
bf16, B = 256) and the MLP denoiser (configs[1]: [512, 512], T = 50, D = 300, bf16, B = 256), both as bench.py builds
them, RMSprop as bench.py runs them.  Both trainers start at step `--start-step` (default 1000: past the warmup, so every
timed step is on the cosine decay, the schedule's dearest branch -- a double division and a double cos at the head of every
thread of every optimizer launch).  Each repetition times `--steps` replayed steps of each trainer between two device
synchronisations; the order of the two trainers alternates from one repetition to the next.  One JSON line per
configuration: median ms/step of each, the spread (min / max over repetitions) and the on / off ratio of the medians.

    python tools/lr_schedule_rate.py [--configs transformer mlp] [--reps 15] [--steps 50]

`--reps 1 --steps 20` is the form to run under `rocprofv3 --kernel-trace --stats -- python ...` (optimizer kernel times:
optim_kernel<SRC, EMA> is the schedule-off launch, optim_kernel<SRC, EMA, SchedArgs> the schedule-on one)."""
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

CONFIGS = {"transformer": ("transformer", 50, 300, 256), "mlp": ("mlp", 50, 300, 256)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["transformer", "mlp"], choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--start-step", type=int, default=1000)
    a = ap.parse_args()
    from bench import build_model, make_batches
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.lr_schedule import LrSchedule
    dev = torch.device("cuda", 0)
    sch = LrSchedule("cosine", 100, 1_000_000, 0.1)
    for name in a.configs:
        kind, T, D, B = CONFIGS[name]
        batch = make_batches(1, B, T, D, torch.bfloat16, dev, seed=0)[0]
        trainers = {}
        for label, schedule in (("off", None), ("on", sch)):
            model = build_model(kind, T, D, torch.bfloat16, dev)
            tr = trainers[label] = HipTrainer(model, "diffusion", "rmsprop", 1e-4, use_graph=True, lr_schedule=schedule)
            tr.steps_done = a.start_step
            tr.step_dev.fill_(a.start_step)
        for tr in trainers.values():                  # eager steps, capture, warm replays
            for _ in range(5):
                tr.step(batch)
        torch.cuda.synchronize()
        assert all(tr._rec is not None for tr in trainers.values())
        ms = {k: [] for k in trainers}
        order = list(trainers)
        for r in range(a.reps):
            for label in (order if r % 2 == 0 else order[::-1]):
                tr = trainers[label]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    tr.step(batch)
                torch.cuda.synchronize()
                ms[label].append((time.perf_counter() - t0) * 1e3 / a.steps)
        med = {k: statistics.median(v) for k, v in ms.items()}
        on = trainers["on"]
        assert int(on.step_dev.cpu()) == on.steps_done and on.current_lr() == sch.lr_at(1e-4, on.steps_done + 1)
        print(json.dumps({"config": name, "B": B, "T": T, "D": D, "params": on.flat.numel(), "reps": a.reps, "steps": a.steps,
                          "schedule": str(sch), "first_timed_step": a.start_step + 6,
                          "ms_per_step_off": round(med["off"], 4), "ms_per_step_on": round(med["on"], 4),
                          "spread_off": [round(min(ms["off"]), 4), round(max(ms["off"]), 4)],
                          "spread_on": [round(min(ms["on"]), 4), round(max(ms["on"]), 4)],
                          "ratio_on_off": round(med["on"] / med["off"], 4)}), flush=True)
        del trainers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
