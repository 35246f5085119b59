"""Cost of clipping to a global gradient norm in the training step: the graph-replayed step of HipTrainer in three forms, in
one process, alternating.

    off            max_grad_norm = 0: the step as ever (gradient sources summed by the optimizer, per-layer optimizer launches)
    materialised   max_grad_norm = 0 with the tuning switches no_opt_fuse + no_early_opt: the step FORM the clip needs (every
                   gradient reduced into memory, one optimizer launch at the end), without the norm pass and the clipped head
    on             max_grad_norm = --max-grad-norm: that form plus ib_grad_sumsq and the clipped launch

materialised / off is the cost of the step form, on / materialised that of the norm pass and the head.  Two configurations: the
headline transformer denoiser (BASELINE configs[2]) and the MLP denoiser (configs[1]), as bench.py builds them, RMSprop as
bench.py runs them.  Each repetition times `--steps` replayed steps of each trainer between two device synchronisations; the
order alternates from one repetition to the next.  One JSON line per configuration.

Then the device time of ib_grad_sumsq alone at each model's n, `--sumsq-reps` launches captured in a graph between two
events: "warm" over one buffer (it stays in the 256 MB last-level cache from launch to launch, as a gradient the backward has
just written may) and "cold" rotating over enough buffers to exceed it, against 4 n bytes at the achievable HBM rate.
Neither number says anything about loss or accuracy.

    python tools/grad_norm_rate.py [--configs transformer mlp] [--reps 15] [--steps 50] [--max-grad-norm 1.0]"""
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
HBM_TBS = 6.3            # achievable HBM rate of the MI355X (a float4 copy), TB/s; the 8 TB/s of the data sheet is not reached


def sumsq_us(n: int, cold: bool, reps: int, rounds: int = 3) -> float:
    """average device time (us) of one ib_grad_sumsq launch over n elements"""
    from inferbiomechanics_amd import hip
    k = min(160, max(2, -(-(768 << 20) // (4 * n)))) if cold else 1
    bufs = [torch.randn(n, device="cuda") for _ in range(k)]
    slots = torch.zeros(hip.grad_sumsq_slots(n), dtype=torch.float64, device="cuda")
    s = hip.new_stream()
    with torch.cuda.stream(s):
        for b in bufs[:2]:
            hip.grad_sumsq(b, slots)
        g = hip.Graph()
        g.begin()
        for i in range(reps):
            hip.grad_sumsq(bufs[i % k], slots)
        g.end()
        g.launch()
        e0, e1 = hip.Event(), hip.Event()
        e0.record()
        for _ in range(rounds):
            g.launch()
        e1.record()
        ms = e0.elapsed_ms(e1)
    torch.cuda.synchronize()
    return ms * 1e3 / (reps * rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["transformer", "mlp"], choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--sumsq-reps", type=int, default=200)
    a = ap.parse_args()
    from bench import build_model, make_batches
    from inferbiomechanics_amd._tuning import tuning as TU
    from inferbiomechanics_amd.engine import HipTrainer
    dev = torch.device("cuda", 0)
    for name in a.configs:
        kind, T, D, B = CONFIGS[name]
        batch = make_batches(1, B, T, D, torch.bfloat16, dev, seed=0)[0]
        trainers = {}
        for label, mgn, form in (("off", 0.0, False), ("materialised", 0.0, True), ("on", a.max_grad_norm, False)):
            model = build_model(kind, T, D, torch.bfloat16, dev)
            TU.no_opt_fuse = TU.no_early_opt = form           # read while the step is issued: until the graph is captured
            tr = trainers[label] = HipTrainer(model, "diffusion", "rmsprop", 1e-4, use_graph=True, max_grad_norm=mgn)
            for _ in range(5):                                # eager steps, capture, warm replays
                tr.step(batch)
            torch.cuda.synchronize()
            TU.no_opt_fuse = TU.no_early_opt = False
            assert tr._rec is not None
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
        n = on.flat.numel()
        out = {"config": name, "B": B, "T": T, "D": D, "params": n, "reps": a.reps, "steps": a.steps,
               "max_grad_norm": on.max_grad_norm, "grad_norm": on.grad_norm(), "clip_coef": on.clip_coef()}
        for k in order:
            out[f"ms_per_step_{k}"] = round(med[k], 4)
            out[f"spread_{k}"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out["ratio_materialised_off"] = round(med["materialised"] / med["off"], 4)
        out["ratio_on_materialised"] = round(med["on"] / med["materialised"], 4)
        out["ratio_on_off"] = round(med["on"] / med["off"], 4)
        print(json.dumps(out), flush=True)
        del trainers, on
        torch.cuda.empty_cache()
        floor = 4 * n / (HBM_TBS * 1e12) * 1e6
        warm, cold = sumsq_us(n, False, a.sumsq_reps), sumsq_us(n, True, a.sumsq_reps)
        print(json.dumps({"config": name, "kernel": "ib_grad_sumsq", "n": n, "bytes": 4 * n, "hbm_tb_per_s": HBM_TBS,
                          "floor_us": round(floor, 3), "warm_us": round(warm, 3), "cold_us": round(cold, 3),
                          "cold_tb_per_s": round(4 * n / cold * 1e-6, 3), "cold_fraction_of_hbm": round(floor / cold, 3),
                          "warm_tb_per_s": round(4 * n / warm * 1e-6, 3)}), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
