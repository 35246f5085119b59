"""Cost of x0- / v-prediction: the graph-replayed training step of HipTrainer and the sampler's step with prediction 'eps' and
'v', in one process, alternating.  ('x0' launches the same kernels as 'v' with one operand fewer.)

    eps       prediction = 'eps': the step as ever
    per_op    (MLP denoiser only) 'eps' with the tuning switch no_chain: the per-op step a v MLP step takes, with the plain
              loss pair
    v         prediction = 'v': ib_mse_loss_pred_partial + ib_mse_loss_weighted_finalize in the loss seam

Training: the headline transformer denoiser (BASELINE configs[2]) and the MLP denoiser (configs[1]), as bench.py builds them,
RMSprop as bench.py runs them.  For the transformer v / eps is the cost of the new pair against the plain pair.  For the bf16
MLP denoiser v / eps is the PRICE OF LEAVING THE CHAIN KERNEL (per_op / eps) times that of the pair (v / per_op).  Each
repetition times `--steps` replayed steps of each trainer between two device synchronisations; the order alternates from one
repetition to the next.  One JSON line per configuration.

Sampling: DDIMSampler over the transformer denoiser, `--sample-steps` steps per call from the captured graph, at B = 1 / 16 /
256 windows: steps per second with 'eps' and with 'v' (one more launch per step, ib_pred_to_eps), alternating, and with a
second 'eps' sampler as the A / A control: two samplers with different buffers in one process differ by themselves.

Then the device time of ib_mse_loss_pred_partial (kind v: four tensors) next to ib_mse_loss_weighted_partial (three) at
M = 12800 rows of D = 300 bf16 columns (row pitch 304), `--kernel-reps` launches captured in a graph between two events:
"warm" over one set of buffers and "cold" rotating over enough sets to exceed the 256 MB last-level cache, against the bytes
each moves at the achievable HBM rate.  None of these numbers says anything about loss or accuracy.

    python tools/prediction_rate.py [--configs transformer mlp] [--reps 15] [--steps 50] [--batches 1 16 256]"""
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
HBM_TBS = 6.3            # achievable HBM rate of the MI355X (a float4 copy), TB/s, as tools/loss_weight_rate.py takes it


def partial_us(pred_kind, cold: bool, reps: int, M: int = 12800, D: int = 300, T: int = 50, rounds: int = 3) -> float:
    """average device time (us) of one partial launch (dpred written) over M x D bf16 elements: ib_mse_loss_weighted_partial
    (pred_kind None) or ib_mse_loss_pred_partial of that kind"""
    from inferbiomechanics_amd import hip
    bf = torch.bfloat16
    tensors = 3 if pred_kind is None else 4
    set_bytes = tensors * M * D * 2
    k = max(2, -(-(768 << 20) // set_bytes)) if cold else 1
    rnd = lambda: torch.randn(M, D, device="cuda").to(bf)
    sets = [(torch.randn(M, 304, device="cuda").to(bf)[:, :D], rnd(), rnd() if pred_kind else None,
             torch.zeros(M, 304, device="cuda", dtype=bf)[:, :D]) for _ in range(k)]
    t = torch.randint(0, 1000, (M // T,), device="cuda")
    wtab, utab, sa, sb = (torch.rand(1000, device="cuda") for _ in range(4))
    ws = torch.zeros(hip.mse_loss_weighted_workspace_bytes(M * D), dtype=torch.uint8, device="cuda")

    def launch(i):
        pred, eps, x0, dpred = sets[i % k]
        if pred_kind is None:
            hip.mse_loss_weighted_partial(pred, eps, ws, t, wtab, T, dpred=dpred)
        else:
            hip.mse_loss_pred_partial(pred, x0, eps, ws, t, wtab, utab, sa, sb, T, pred_kind, dpred=dpred)
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


def alternate(forms: dict, reps: int, run) -> dict:
    """{label: [ms per repetition]}: run(forms[label]) timed between two synchronisations, the order reversed every other time"""
    ms = {k: [] for k in forms}
    order = list(forms)
    for r in range(reps):
        for label in (order if r % 2 == 0 else order[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(forms[label])
            torch.cuda.synchronize()
            ms[label].append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["transformer", "mlp"], choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batches", nargs="*", type=int, default=[1, 16, 256])
    ap.add_argument("--sample-steps", type=int, default=50)
    ap.add_argument("--kernel-reps", type=int, default=200)
    a = ap.parse_args()
    from bench import build_model, make_batches
    from inferbiomechanics_amd._tuning import tuning as TU
    from inferbiomechanics_amd.diffusion.sampler import DDIMSampler
    from inferbiomechanics_amd.engine import HipTrainer
    dev = torch.device("cuda", 0)
    for name in a.configs:
        kind, T, D, B = CONFIGS[name]
        batch = make_batches(1, B, T, D, torch.bfloat16, dev, seed=0)[0]
        forms = [("eps", "eps", False)] + ([("per_op", "eps", True)] if kind == "mlp" else []) + [("v", "v", False)]
        trainers = {}
        for label, pred, no_chain in forms:
            model = build_model(kind, T, D, torch.bfloat16, dev)
            TU.no_chain = no_chain                            # read while the step is issued: until the graph is captured
            tr = trainers[label] = HipTrainer(model, "diffusion", "rmsprop", 1e-4, use_graph=True, prediction=pred)
            for _ in range(5):                                # eager steps, capture, warm replays
                tr.step(batch)
            torch.cuda.synchronize()
            TU.no_chain = False
            assert tr._rec is not None or tr._pinned

        def steps(tr):
            for _ in range(a.steps):
                tr.step(batch)
        ms = {k: [m / a.steps for m in v] for k, v in alternate(trainers, a.reps, steps).items()}
        med = {k: statistics.median(v) for k, v in ms.items()}
        rep = trainers["v"].level_loss()
        out = {"config": name, "B": B, "T": T, "D": D, "reps": a.reps, "steps": a.steps, "loss_v": rep["weighted"],
               "eps_mse_v": rep["unweighted"], "report_steps": rep["steps"]}
        for k in trainers:
            out[f"ms_per_step_{k}"] = round(med[k], 4)
            out[f"spread_{k}"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out["ratio_v_eps"] = round(med["v"] / med["eps"], 4)
        if "per_op" in med:
            out["ratio_per_op_eps"] = round(med["per_op"] / med["eps"], 4)
            out["ratio_v_per_op"] = round(med["v"] / med["per_op"], 4)
        print(json.dumps(out), flush=True)
        del trainers
        torch.cuda.empty_cache()
    if a.batches:
        kind, T, D, _ = CONFIGS["transformer"]
        samplers = {}
        for label, pred in (("eps", "eps"), ("v", "v"), ("eps_again", "eps")):      # a second eps sampler: the A / A control
            model = build_model(kind, T, D, torch.bfloat16, dev)
            model.prediction = pred
            model.eval()
            samplers[label] = DDIMSampler(model, a.sample_steps, use_graph=True)
        for B in a.batches:
            x_T = torch.randn(B, T, D, device=dev)
            for s in samplers.values():                       # a new batch size: the eager step, the capture, warm replays
                s.sample(x_T)
                s.sample(x_T)
            ms = alternate(samplers, a.reps, lambda s: s.sample(x_T))
            rate = {k: [a.sample_steps / (m * 1e-3) for m in v] for k, v in ms.items()}
            med = {k: statistics.median(v) for k, v in rate.items()}
            print(json.dumps({"sampler": "DDIMSampler", "B": B, "T": T, "D": D, "sample_steps": a.sample_steps, "reps": a.reps,
                              "steps_per_s_eps": round(med["eps"], 1), "steps_per_s_v": round(med["v"], 1),
                              "steps_per_s_eps_again": round(med["eps_again"], 1),
                              "spread_eps": [round(min(rate["eps"]), 1), round(max(rate["eps"]), 1)],
                              "spread_v": [round(min(rate["v"]), 1), round(max(rate["v"]), 1)],
                              "spread_eps_again": [round(min(rate["eps_again"]), 1), round(max(rate["eps_again"]), 1)],
                              "ratio_v_eps": round(med["v"] / med["eps"], 4),
                              "ratio_eps_again_eps": round(med["eps_again"] / med["eps"], 4),
                              "us_per_step_v_minus_eps": round(1e6 / med["v"] - 1e6 / med["eps"], 2)}), flush=True)
        del samplers
        torch.cuda.empty_cache()
    M, D = 12800, 300
    for label, pred_kind, tensors in (("ib_mse_loss_weighted_partial", None, 3), ("ib_mse_loss_pred_partial[x0]", "x0", 3),
                                      ("ib_mse_loss_pred_partial[v]", "v", 4)):
        moved = tensors * M * D * 2
        floor = moved / (HBM_TBS * 1e12) * 1e6
        warm, cold = partial_us(pred_kind, False, a.kernel_reps), partial_us(pred_kind, True, a.kernel_reps)
        print(json.dumps({"kernel": label, "M": M, "D": D, "dtype": "bf16", "bytes": moved, "hbm_tb_per_s": HBM_TBS,
                          "floor_us": round(floor, 3), "warm_us": round(warm, 3), "cold_us": round(cold, 3),
                          "cold_tb_per_s": round(moved / cold * 1e-6, 3), "cold_fraction_of_hbm": round(floor / cold, 3),
                          "warm_tb_per_s": round(moved / warm * 1e-6, 3)}), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
