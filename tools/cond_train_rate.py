"""Cost of conditional training (`train --cond-cols`) in the training step: the graph-replayed step of HipTrainer at
cond_cols = 0 and at cond_cols = 270 (label inference: feat_dim - 30), in one process, alternating.

Two configurations, as bench.py builds them, RMSprop as bench.py runs them:
  transformer  the headline denoiser (BASELINE configs[2]: 4 layers, d_model 512, T = 50, D = 300, bf16, B = 256).  Both
               arms run q_sample -> plan.forward -> loss -> plan.backward; at 270 the two conditional kernels stand in
               for q_sample / mse_loss_partial and move fewer bytes.
  mlp          the MLP denoiser (configs[1]: [512, 512], T = 50, D = 300, bf16, B = 256).  At 0 the step is the fused chain
               kernel, at 270 the per-op path (the chain kernel noises and scores every column), so this is chain against
               per-op; a third arm, cond_cols = 0 with the chain switched off, separates the path from the kernels.
Each repetition times `--steps` replayed steps of each trainer between two device synchronisations; the order of the arms
alternates from one repetition to the next.  One JSON line per configuration: median ms/step of each arm, the spread (min /
max over repetitions) and the ratios of the medians.

    python tools/cond_train_rate.py [--configs transformer mlp] [--reps 15] [--steps 50] [--cond-cols 270]"""
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
    ap.add_argument("--cond-cols", type=int, default=270)
    a = ap.parse_args()
    from bench import build_model, make_batches
    from inferbiomechanics_amd._tuning import tuning as TU
    from inferbiomechanics_amd.engine import HipTrainer
    dev = torch.device("cuda", 0)
    for name in a.configs:
        kind, T, D, B = CONFIGS[name]
        batch = make_batches(1, B, T, D, torch.bfloat16, dev, seed=0)[0]
        arms = [("c0", 0, False), (f"c{a.cond_cols}", a.cond_cols, False)]
        if kind == "mlp":
            arms.append(("c0_per_op", 0, True))
        trainers = {}
        for label, C, no_chain in arms:
            model = build_model(kind, T, D, torch.bfloat16, dev)
            tr = HipTrainer(model, "diffusion", "rmsprop", 1e-4, use_graph=True, cond_cols=C)
            old = TU.no_chain
            TU.no_chain = old or no_chain            # read while the step's launches are issued: eager steps + capture
            try:
                for _ in range(5):
                    tr.step(batch)
            finally:
                TU.no_chain = old
            torch.cuda.synchronize()
            assert tr._rec is not None
            trainers[label] = tr
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
        out = {"config": name, "B": B, "T": T, "D": D, "cond_cols": a.cond_cols, "reps": a.reps, "steps": a.steps}
        for k in order:
            out[f"ms_per_step_{k}"] = round(med[k], 4)
            out[f"spread_{k}"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out["ratio_cond_over_c0"] = round(med[order[1]] / med["c0"], 4)
        if "c0_per_op" in med:
            out["ratio_cond_over_c0_per_op"] = round(med[order[1]] / med["c0_per_op"], 4)
            out["paths"] = {"c0": "chain", order[1]: "per-op", "c0_per_op": "per-op"}
        print(json.dumps(out), flush=True)
        del trainers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
