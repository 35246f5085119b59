"""Cost of the decoupled weight decay in the training step: the graph-replayed step of HipTrainer with weight_decay 0 and
0.01, in one process, alternating.

Two configurations: the headline transformer denoiser (BASELINE configs[2]: 4 layers, d_model 512, T = 50, D = 300,
bf16, B = 256) and the MLP denoiser (configs[1]: [512, 512], T = 50, D = 300, bf16, B = 256), both as bench.py builds
them, RMSprop as bench.py runs them.  The decayed trainer's launches are the `_decay` entries: per quad a wave-uniform binary
search of the range table (device memory) ahead of the update, and one more multiply.  Each repetition times `--steps`
replayed steps of each trainer between two device synchronisations; the order of the two trainers alternates from one
repetition to the next.  One JSON line per configuration: median ms/step of each, the spread (min / max over repetitions)
and the on / off ratio of the medians.  Neither number says anything about loss or accuracy.

    python tools/weight_decay_rate.py [--configs transformer mlp] [--reps 15] [--steps 50] [--weight-decay 0.01]

`--reps 1 --steps 20` is the form to run under `rocprofv3 --kernel-trace --stats -- python ...` (optimizer kernel times:
optim_kernel<SRC, EMA> is the launch without decay, optim_kernel<SRC, EMA, DecayArgs> the decayed one)."""
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
    ap.add_argument("--weight-decay", type=float, default=0.01)
    a = ap.parse_args()
    from bench import build_model, make_batches
    from inferbiomechanics_amd.engine import HipTrainer
    dev = torch.device("cuda", 0)
    for name in a.configs:
        kind, T, D, B = CONFIGS[name]
        batch = make_batches(1, B, T, D, torch.bfloat16, dev, seed=0)[0]
        trainers = {}
        for label, wd in (("off", 0.0), ("on", a.weight_decay)):
            model = build_model(kind, T, D, torch.bfloat16, dev)
            trainers[label] = HipTrainer(model, "diffusion", "rmsprop", 1e-4, use_graph=True, weight_decay=wd)
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
        assert trainers["off"].decay_table is None and on.decay_table is not None and on.decay_table.n >= 1
        print(json.dumps({"config": name, "B": B, "T": T, "D": D, "params": on.flat.numel(), "reps": a.reps, "steps": a.steps,
                          "weight_decay": on.weight_decay, "decayed_tensors": len(on.decayed), "tensors": len(on.layout),
                          "ranges": on.decay_table.n,
                          "ms_per_step_off": round(med["off"], 4), "ms_per_step_on": round(med["on"], 4),
                          "spread_off": [round(min(ms["off"]), 4), round(max(ms["off"]), 4)],
                          "spread_on": [round(min(ms["on"]), 4), round(max(ms["on"]), 4)],
                          "ratio_on_off": round(med["on"] / med["off"], 4)}), flush=True)
        del trainers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
