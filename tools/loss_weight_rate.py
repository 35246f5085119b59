"""Cost of weighting the diffusion loss by noise level in the training step: the graph-replayed step of HipTrainer with the
weight off and on, in one process, alternating.

    off       loss_weight = None: the step as ever
    per_op    (MLP denoiser only) loss_weight = None with the tuning switch no_chain: the per-op step the weighted MLP step
              takes, without the weighted launches
    on        loss_weight = LossWeight('min_snr', gamma): the weighted pair in the loss seam

Two configurations: the headline transformer denoiser (BASELINE configs[2]) and the MLP denoiser (configs[1]), as bench.py
builds them, RMSprop as bench.py runs them.  For the transformer on / off is the cost of the weighted pair against the plain
pair.  For the bf16 MLP denoiser on / off is the PRICE OF LEAVING THE CHAIN KERNEL (per_op / off) times that of the pair
(on / per_op): its one-launch step scores every row alike, so a weighted step takes the per-op path.  Each repetition times
`--steps` replayed steps of each trainer between two device synchronisations; the order alternates from one repetition to
the next.  One JSON line per configuration.

Then the device time of ib_mse_loss_weighted_partial next to ib_mse_loss_partial at M = 12800 rows of D = 300 bf16 columns
(row pitch 304), `--kernel-reps` launches captured in a graph between two events: "warm" over one set of buffers (23 MB: they
stay in the 256 MB last-level cache from launch to launch, as a prediction the forward has just written does) and "cold"
rotating over enough sets to exceed it, against the 3 M D elements each moves at the achievable HBM rate.
Neither number says anything about loss or accuracy.

    python tools/loss_weight_rate.py [--configs transformer mlp] [--reps 15] [--steps 50] [--gamma 5]"""
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


def partial_us(weighted: bool, cold: bool, reps: int, M: int = 12800, D: int = 300, T: int = 50, rounds: int = 3) -> float:
    """average device time (us) of one partial launch (dpred written) over M x D bf16 elements"""
    from inferbiomechanics_amd import hip
    bf = torch.bfloat16
    set_bytes = 3 * M * D * 2
    k = max(2, -(-(768 << 20) // set_bytes)) if cold else 1
    sets = [(torch.randn(M, 304, device="cuda").to(bf)[:, :D], torch.randn(M, D, device="cuda").to(bf),
             torch.zeros(M, 304, device="cuda", dtype=bf)[:, :D]) for _ in range(k)]
    t = torch.randint(0, 1000, (M // T,), device="cuda")
    wtab = torch.rand(1000, device="cuda")
    nbytes = hip.mse_loss_weighted_workspace_bytes(M * D) if weighted else hip.mse_loss_workspace_bytes(M * D)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

    def launch(i):
        pred, target, dpred = sets[i % k]
        if weighted:
            hip.mse_loss_weighted_partial(pred, target, ws, t, wtab, T, dpred=dpred)
        else:
            hip.mse_loss_partial(pred, target, ws, dpred=dpred)
    s = hip.new_stream()
    with torch.cuda.stream(s):
        launch(0)
        launch(1)
        g = hip.Graph()
        g.begin()
        for i in range(reps):
            launch(i)
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
    ap.add_argument("--gamma", type=float, default=5.0)
    ap.add_argument("--kernel-reps", type=int, default=200)
    a = ap.parse_args()
    from bench import build_model, make_batches
    from inferbiomechanics_amd._tuning import tuning as TU
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.loss_weight import LossWeight
    dev = torch.device("cuda", 0)
    for name in a.configs:
        kind, T, D, B = CONFIGS[name]
        batch = make_batches(1, B, T, D, torch.bfloat16, dev, seed=0)[0]
        forms = [("off", None, False)] + ([("per_op", None, True)] if kind == "mlp" else []) + \
            [("on", LossWeight("min_snr", gamma=a.gamma), False)]
        trainers = {}
        for label, lw, no_chain in forms:
            model = build_model(kind, T, D, torch.bfloat16, dev)
            TU.no_chain = no_chain                            # read while the step is issued: until the graph is captured
            tr = trainers[label] = HipTrainer(model, "diffusion", "rmsprop", 1e-4, use_graph=True, loss_weight=lw)
            for _ in range(5):                                # eager steps, capture, warm replays
                tr.step(batch)
            torch.cuda.synchronize()
            TU.no_chain = False
            assert tr._rec is not None or tr._pinned
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
        rep = on.level_loss()
        out = {"config": name, "B": B, "T": T, "D": D, "reps": a.reps, "steps": a.steps, "loss_weight": repr(on.loss_weight),
               "loss_weighted": rep["weighted"], "loss_unweighted": rep["unweighted"], "report_steps": rep["steps"]}
        for k in order:
            out[f"ms_per_step_{k}"] = round(med[k], 4)
            out[f"spread_{k}"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out["ratio_on_off"] = round(med["on"] / med["off"], 4)
        if "per_op" in med:
            out["ratio_per_op_off"] = round(med["per_op"] / med["off"], 4)
            out["ratio_on_per_op"] = round(med["on"] / med["per_op"], 4)
        print(json.dumps(out), flush=True)
        del trainers, on
        torch.cuda.empty_cache()
    M, D = 12800, 300
    moved = 3 * M * D * 2
    floor = moved / (HBM_TBS * 1e12) * 1e6
    for label, weighted in (("ib_mse_loss_partial", False), ("ib_mse_loss_weighted_partial", True)):
        warm, cold = partial_us(weighted, False, a.kernel_reps), partial_us(weighted, True, a.kernel_reps)
        print(json.dumps({"kernel": label, "M": M, "D": D, "dtype": "bf16", "bytes": moved, "hbm_tb_per_s": HBM_TBS,
                          "floor_us": round(floor, 3), "warm_us": round(warm, 3), "cold_us": round(cold, 3),
                          "cold_tb_per_s": round(moved / cold * 1e-6, 3), "cold_fraction_of_hbm": round(floor / cold, 3),
                          "warm_tb_per_s": round(moved / warm * 1e-6, 3)}), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
