"""Cost of the velocity term of the diffusion loss (HipTrainer(velocity_loss=...), `train --velocity-loss`): the graph-replayed
training step with the term off and on, in one process, alternating.

    off       velocity_loss = None: the step as ever (prediction 'v': ib_mse_loss_pred_partial in the loss seam)
    per_op    (MLP denoiser only) off with the tuning switch no_chain: the per-op step an MLP step with the term takes
    on        velocity_loss = VelocityLoss(1.0): ib_vel_loss_partial + ib_vel_loss_finalize in the loss seam

Cases: the headline transformer denoiser (BASELINE configs[2]) at prediction eps and v, and the MLP denoiser (configs[1]) at
eps, as bench.py builds them, RMSprop as bench.py runs them.  For the bf16 MLP denoiser on / off is the PRICE OF LEAVING THE
CHAIN KERNEL (per_op / off) times that of the new pair (on / per_op).  Each repetition times `--steps` replayed steps of each
trainer between two device synchronisations; the order alternates from one repetition to the next.  One JSON line per case.

Then the device time of ib_vel_loss_partial next to ib_mse_loss_pred_partial on the same buffers, kinds eps and v, at M = 12800
rows (256 windows of 50 frames) of D = 300 bf16 columns (row pitch 304), `--kernel-reps` launches captured in a graph between
two events: "warm" over one set of buffers and "cold" rotating over enough sets to exceed the 256 MB last-level cache.  Derived,
not measured: at chunk length FC the new kernel reads at most (FC + 2) / FC times the bytes of ib_mse_loss_pred_partial (one
halo frame on each side of every chunk of FC).  None of these numbers says anything about loss or accuracy.

    python tools/velocity_loss_rate.py [--cases transformer_eps transformer_v mlp_eps] [--reps 15] [--steps 50]"""
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

CASES = {"transformer_eps": ("transformer", "eps"), "transformer_v": ("transformer", "v"), "mlp_eps": ("mlp", "eps")}
T, D, B = 50, 300, 256


def partial_us(entry: str, kind: str, cold: bool, reps: int, M: int = B * T, rounds: int = 3) -> float:
    """average device time (us) of one partial launch (dpred written) over M x D bf16 elements: entry 'pred'
    (ib_mse_loss_pred_partial) or 'vel' (ib_vel_loss_partial), both of `kind`, over the same buffers"""
    from inferbiomechanics_amd import hip
    bf = torch.bfloat16
    set_bytes = 4 * M * D * 2
    k = max(2, -(-(768 << 20) // set_bytes)) if cold else 1
    g0 = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda: torch.randn(M, D, device="cuda", generator=g0).to(bf)
    sets = [(torch.randn(M, 304, device="cuda", generator=g0).to(bf)[:, :D], rnd(), rnd(),
             torch.zeros(M, 304, device="cuda", dtype=bf)[:, :D]) for _ in range(k)]
    t = torch.randint(0, 1000, (M // T,), device="cuda", generator=g0)
    wtab, utab, vtab, xtab, sa, sb = (torch.rand(1000, device="cuda", generator=g0) for _ in range(6))
    nbytes = hip.vel_loss_workspace_bytes(M, D, T) if entry == "vel" else hip.mse_loss_weighted_workspace_bytes(M * D)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")

    def launch(i):
        pred, eps, x0, dpred = sets[i % k]
        if entry == "vel":
            hip.vel_loss_partial(pred, x0, eps, ws, t, wtab, utab, vtab, xtab, sa, sb, T, kind, dpred=dpred)
        else:
            hip.mse_loss_pred_partial(pred, x0, eps, ws, t, wtab, utab, sa, sb, T, kind, dpred=dpred)
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
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--kernel-reps", type=int, default=200)
    a = ap.parse_args()
    from bench import build_model, make_batches
    from inferbiomechanics_amd import hip
    from inferbiomechanics_amd._tuning import tuning as TU
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.velocity_loss import VelocityLoss
    dev = torch.device("cuda", 0)
    for name in a.cases:
        kind, pred = CASES[name]
        batch = make_batches(1, B, T, D, torch.bfloat16, dev, seed=0)[0]
        forms = [("off", None, False)] + ([("per_op", None, True)] if kind == "mlp" else []) + [("on", VelocityLoss(1.0), False)]
        trainers = {}
        for label, vl, no_chain in forms:
            model = build_model(kind, T, D, torch.bfloat16, dev)
            TU.no_chain = no_chain                            # read while the step is issued: until the graph is captured
            tr = trainers[label] = HipTrainer(model, "diffusion", "rmsprop", 1e-4, use_graph=True, prediction=pred,
                                              velocity_loss=vl)
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
        rep = trainers["on"].level_loss()
        out = {"case": name, "B": B, "T": T, "D": D, "prediction": pred, "reps": a.reps, "steps": a.steps,
               "loss_on": rep["weighted"], "mse_on": rep["mse"], "velocity_on": rep["velocity"],
               "x0_velocity_on": rep["x0_velocity"], "report_steps": rep["steps"]}
        for k in trainers:
            out[f"ms_per_step_{k}"] = round(med[k], 4)
            out[f"spread_{k}"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out["ratio_on_off"] = round(med["on"] / med["off"], 4)
        out["us_on_minus_off"] = round((med["on"] - med["off"]) * 1e3, 2)
        if "per_op" in med:
            out["ratio_per_op_off"] = round(med["per_op"] / med["off"], 4)
            out["ratio_on_per_op"] = round(med["on"] / med["per_op"], 4)
        print(json.dumps(out), flush=True)
        del trainers
        torch.cuda.empty_cache()
    FC = hip.vel_loss_frame_chunk()
    for kind, tensors in (("eps", 3), ("v", 4)):
        row = {"kernels": "ib_vel_loss_partial / ib_mse_loss_pred_partial", "kind": kind, "M": B * T, "D": D, "T": T,
               "dtype": "bf16", "frame_chunk": FC, "pred_bytes": tensors * B * T * D * 2,
               "derived_read_bound": f"(FC + 2) / FC = {(FC + 2) / FC:.3f} of the bytes ib_mse_loss_pred_partial reads"}
        for cold in (False, True):
            for entry in ("pred", "vel"):
                row[f"{entry}_{'cold' if cold else 'warm'}_us"] = round(partial_us(entry, kind, cold, a.kernel_reps), 3)
                torch.cuda.empty_cache()
        row["ratio_warm"] = round(row["vel_warm_us"] / row["pred_warm_us"], 3)
        row["ratio_cold"] = round(row["vel_cold_us"] / row["pred_cold_us"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
