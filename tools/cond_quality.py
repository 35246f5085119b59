"""Does training on clean conditioning columns help label inference?  A synthetic linear-Gaussian window set in the layout
of the regression windows (the input keys of a frame ~ N(0, I), 147 columns at the defaults; the 30 label columns
cop | force | torque | wrench = inputs W + 0.05 n with one fixed W, n ~ N(0, I)) and the same small transformer denoiser
trained twice from the same seed for the same number of steps on device-drawn batches: once unconditional
(cond_cols = 0, labels inferred by replacement: observations forward-noised at every step), once with
cond_cols = D - 30 (observations pinned clean).

What runs is what `train` and `analyze` run, called as functions: the registry's model (get_model), HipTrainer.step_drawn
over a DeviceMotionCache of the MotionWindowView matrices, cli.train.save_checkpoint, then a FRESH model filled by
load_latest_checkpoint (which restores cond_cols) and DiffusionLabelPredictor over DataLoader batches of held-out windows,
as AnalyzeCommand.run_diffusion drives it.  The command line itself is not used: its --synthetic-windows draw the labels
independently of the inputs, so there is nothing to infer in them, and this window set exists only here.  The figure is
the RMSE of the predictor's outputs against the noise-free labels inputs W, next to the RMSE of predicting 0 (the labels'
own RMS); `analyze`'s report (RegressionLossEvaluator) is not used either, it reports per-key losses in other units.
One JSON line.

    python tools/cond_quality.py [--steps 3000] [--sample-steps 50] [--dtype fp32] [--sampler ddim]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch.utils.data import DataLoader, Dataset  # noqa: E402


class LinearGaussianWindows(Dataset):
    """SyntheticWindowDataset's item layout with labels that depend on the inputs: labels = inputs W + noise n"""

    def __init__(self, num_windows, frames, W, seed, noise=0.05, num_dofs=23, history_width=15):
        from inferbiomechanics_amd.data.AddBiomechanicsDataset import input_key_widths
        self.num_windows, self.frames, self.W, self.seed, self.noise = num_windows, frames, W, seed, noise
        self.num_dofs, self.num_contact_bodies, self.output_data_format = num_dofs, 2, 'all_frames'
        self.widths = input_key_widths(num_dofs, history_width)

    def __len__(self):
        return self.num_windows

    def clean(self, inputs):
        from inferbiomechanics_amd.data.AddBiomechanicsDataset import INPUT_KEY_ORDER
        return torch.cat([inputs[k] for k in INPUT_KEY_ORDER], dim=-1) @ self.W

    def __getitem__(self, index):
        from inferbiomechanics_amd.data.AddBiomechanicsDataset import INPUT_KEY_ORDER, LOSS_KEY_ORDER, LOSS_KEY_WIDTHS
        g = torch.Generator().manual_seed(self.seed * 1000003 + index)
        inputs = {k: torch.randn(self.frames, w, generator=g) for k, w in zip(INPUT_KEY_ORDER, self.widths)}
        y = self.clean(inputs) + self.noise * torch.randn(self.frames, 30, generator=g)
        labels, c = {}, 0
        for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
            labels[k] = y[:, c:c + w].contiguous()
            c += w
        return inputs, labels, 0, index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--train-windows", type=int, default=4096)
    ap.add_argument("--test-windows", type=int, default=256)
    ap.add_argument("--sample-steps", type=int, default=50)
    ap.add_argument("--sampler", choices=["ddim", "dpmpp2m"], default="ddim")
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from inferbiomechanics_amd.cli.abstract_command import AbstractCommand
    from inferbiomechanics_amd.cli.train import save_checkpoint
    from inferbiomechanics_amd.data.AddBiomechanicsDataset import LOSS_KEY_ORDER, MotionWindowView
    from inferbiomechanics_amd.data.WindowCache import DeviceMotionCache
    from inferbiomechanics_amd.engine import HipTrainer
    from inferbiomechanics_amd.models.DiffusionLabelPredictor import DiffusionLabelPredictor
    dev = torch.device("cuda", 0)
    dt = torch.float32 if a.dtype == "fp32" else torch.bfloat16
    T = a.window
    n_in = sum(LinearGaussianWindows(1, T, None, 0).widths)
    D = n_in + 30
    W = torch.randn(n_in, 30, generator=torch.Generator().manual_seed(1234)) / n_in ** 0.5
    train_set = LinearGaussianWindows(a.train_windows, T, W, seed=0)
    test_set = LinearGaussianWindows(a.test_windows, T, W, seed=1)
    view = MotionWindowView(train_set)
    train = torch.stack([view[i] for i in range(len(view))])
    cmd = AbstractCommand()
    build = lambda: cmd.get_model(23, 2, "diffusion-transformer", device=dev, compute_dtype=dt, feat_dim=D, window=T,
                                  d_model=128, num_heads=4, dim_feedforward=256, num_layers=2).to(dev)
    out = {"D": D, "cond_cols": n_in, "window": T, "train_steps": a.steps, "batch": a.batch, "sampler": a.sampler,
           "sample_steps": a.sample_steps, "dtype": a.dtype, "test_windows": a.test_windows}
    for label, C in (("unconditional", 0), ("cond_cols", n_in)):
        torch.manual_seed(a.seed)                       # same initial weights, same device-drawn (t, eps) sequence
        model = build()
        model.cond_cols = C
        tr = HipTrainer(model, "diffusion", "adam", 1e-3, cond_cols=C)
        cache = DeviceMotionCache(train, dev, dt)
        batches = list(cache.batches(a.batch))
        for i in range(a.steps):
            tr.step_drawn(cache, batches[i % len(batches)])
        out[f"final_train_loss_{label}"] = round(tr.loss_value(), 5)
        with tempfile.TemporaryDirectory() as ck:
            save_checkpoint(ck, 0, a.steps, model, tr)
            del tr, model
            model = build()                             # what analyze does: a fresh model, the checkpoint decides the mode
            cmd.load_latest_checkpoint(model, checkpoint_dir=ck)
        assert model.cond_cols == C
        model.eval()
        pred = DiffusionLabelPredictor(model, a.sample_steps, seed=7, solver=a.sampler)
        sq = ref = n = 0.0
        i = 0
        for inputs, labels, _subj, _trial in DataLoader(test_set, batch_size=64, shuffle=False):
            got = pred(inputs, labels, draw=i)
            y = torch.cat([got[k].float().cpu() for k in LOSS_KEY_ORDER], dim=-1)
            clean = test_set.clean(inputs)
            sq += float((y - clean).double().pow(2).sum())
            ref += float(clean.double().pow(2).sum())
            n += clean.numel()
            i += clean.shape[0]
        assert pred.sampler.observations == ("clean" if C else "noised")
        out["label_rms"] = round((ref / n) ** 0.5, 4)
        out[f"label_rmse_{label}"] = round((sq / n) ** 0.5, 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
