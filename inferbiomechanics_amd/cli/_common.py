"""Flag groups and factories shared by the train / analyze / visualize commands.  Flag names and defaults
are the reference's (src/cli/train.py:24-69, analyze.py:23-47, visualize.py:21-56); the additive flags
(`--device` on train, `--synthetic-windows`, `--compute-dtype`, `--max-steps`, `--eager`) are new."""
import argparse
import logging
import os
from typing import Optional

import torch

from ..data.AddBiomechanicsDataset import (AddBiomechanicsDataset, MotionWindowView, SyntheticMotionWindows,
                                               SyntheticWindowDataset)


LABEL_NAMES = ('cop', 'force', 'torque', 'wrench')       # LOSS_KEY_ORDER, as the reports name the keys


def add_component_flags(p: argparse.ArgumentParser, train_defaults: bool):
    d6 = list(range(6)) if train_defaults else None
    p.add_argument('--predict-grf-components', type=int, nargs='+', default=d6 if train_defaults else [1],
                   help='Which grf components to train.')
    p.add_argument('--predict-cop-components', type=int, nargs='*', default=d6 if train_defaults else [],
                   help='Which cop components to train.')
    p.add_argument('--predict-moment-components', type=int, nargs='*', default=d6 if train_defaults else [],
                   help='Which moment components to train.')
    p.add_argument('--predict-wrench-components', type=int, nargs='*',
                   default=list(range(12)) if train_defaults else [], help='Which wrench components to train.')


def add_additive_flags(p: argparse.ArgumentParser, device_default: str = 'gpu'):
    p.add_argument('--device', type=str, default=device_default,
                   help="Where to run: 'gpu' (HIP kernels on the local MI355X). 'cpu' is refused: no CPU path.")
    p.add_argument('--synthetic-windows', type=int, default=0,
                   help='Use N seeded synthetic windows per split instead of .b3d files (no nimblephysics needed).')
    p.add_argument('--compute-dtype', type=str, default='fp32', choices=['fp32', 'bf16'],
                   help='Storage type of activations/weights in the kernels (fp32 = parity mode).')
    p.add_argument('--feat-dim', type=int, default=300, help='[diffusion models] features per frame.')


def dtype_of(args) -> torch.dtype:
    return torch.bfloat16 if getattr(args, 'compute_dtype', 'fp32') == 'bf16' else torch.float32


def is_diffusion(model_type: str) -> bool:
    return model_type.startswith('diffusion')


def open_dataset(args, split: str, history_len: int, stride: int, output_data_format: str, geometry: Optional[str]):
    """`.b3d` windows through data/AddBiomechanicsDataset.py (needs the nimblephysics wheel at run time), or seeded
    synthetic windows with the same per-item layout.  The diffusion models see a window as one [F, D] matrix
    (`MotionWindowView`: the model-input channels and the four label blocks of every frame side by side)."""
    n = getattr(args, 'synthetic_windows', 0)
    model_type = getattr(args, 'model_type', 'feedforward')
    if n > 0:
        seed = {'train': 0, 'dev': 1, 'test': 2}.get(split, 3)
        if is_diffusion(model_type):
            return SyntheticMotionWindows(n, window=history_len // stride if stride > 1 else history_len,
                                          feat=args.feat_dim, seed=seed)
        return SyntheticWindowDataset(n, history_len, stride, output_data_format=output_data_format, seed=seed,
                                      history_width=30 if model_type == 'groundlink' else 0)   # root_history_len = 10
    path = os.path.abspath(os.path.join(args.dataset_home, split))
    try:
        from ..data.AddBiomechanicsDataset import _nimble
        _nimble()
    except ImportError:
        raise SystemExit(f"Reading {path} needs the `nimblephysics` .b3d loader, which is not installed. "
                         f"Pass --synthetic-windows N to run the hot path on seeded synthetic windows.")
    # the reference call (train.py:141-148, analyze.py:82-88, visualize.py:94-101)
    dataset = AddBiomechanicsDataset(path, history_len, geometry, device=torch.device('cpu'), stride=stride,
                                     output_data_format=output_data_format,
                                     testing_with_short_dataset=bool(getattr(args, 'short', False)),
                                     skip_loading_skeletons=not getattr(args, 'compute_report', False)
                                     and getattr(args, 'command', 'train') == 'train')
    if is_diffusion(model_type):
        return MotionWindowView(dataset)
    return dataset


def pick_device(args) -> torch.device:
    from .. import hip
    if hip._dry_run:                      # tests/test_plumbing_cpu.py only
        return torch.device('cpu')
    if str(args.device) == 'cpu':
        raise SystemExit("--device cpu: this build has no CPU path (the reference's PyTorch-CPU path is the "
                         "reference itself). Use --device gpu.")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: the HIP path needs an MI355X")
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if os.environ.get('IB_BENCH_REHEARSAL') == '1':      # several ranks on a one-GPU box (control-flow rehearsal over gloo)
        local = 0
    torch.cuda.set_device(local)
    return torch.device('cuda', local)


GUIDANCE_HELP = ('classifier-free guidance strength S of the sampler: the noise prediction becomes '
                 'eps_c + S (eps_c - eps_u), eps_u the prediction with the conditioning columns zeroed. Needs a checkpoint '
                 'of `train --cond-cols N --cond-drop P` with P > 0. 0 = off.')


RESAMPLE_HELP = ('RePaint resampling of the masked loop (Lugmayr et al. 2022): after denoising, the state is diffused back '
                 'J levels with fresh noise and denoised again, --resample-times R times in all at every J-th level, so the '
                 'free columns harmonise with the observed ones. Needs --sample-eta 0 and --sampler ddim, J in 1 .. '
                 '--sample-steps - 1; costs about R times the denoiser evaluations. Its effect on label accuracy of trained '
                 'checkpoints is unmeasured. 0 = off.')


def add_resample_flags(p, scope: str):
    """--resample-jump J --resample-times R of analyze / visualize; the defaults 0 / 1 mean off"""
    p.add_argument('--resample-jump', type=int, default=0, help=f'[{scope}] ' + RESAMPLE_HELP)
    p.add_argument('--resample-times', type=int, default=1,
                   help=f'[{scope}] visits of every jump point of --resample-jump (1 = the plain loop).')


def checked_resample(args, steps: int, eta: float, solver: str):
    """--resample-jump / --resample-times of analyze / visualize -> (J, R), or None when off"""
    J, R = int(getattr(args, 'resample_jump', 0)), int(getattr(args, 'resample_times', 1))
    if J == 0 and R == 1:
        return None
    if R < 1:
        raise SystemExit(f"--resample-times {R} must be >= 1")
    if not 1 <= J <= steps - 1:
        raise SystemExit(f"--resample-jump {J} must be in 1 .. --sample-steps - 1 = {steps - 1} (a jump goes back J of the "
                         f"loop's steps); 0 with --resample-times 1 turns resampling off")
    if eta > 0.0:
        raise SystemExit(f"--resample-jump needs --sample-eta 0, got {eta}: the step noise of an eta > 0 loop is keyed by the "
                         f"step index, so a revisited step would repeat its draw")
    if solver != 'ddim':
        raise SystemExit(f"--resample-jump needs --sampler ddim, got {solver}: the multistep history of a second-order "
                         f"solver is invalid after a jump")
    return (J, R)


INTERVAL_HELP = ('report order statistics of the posterior ensemble: the central interval of nominal coverage L (0 < L < 1) of '
                 'every label, from the Weibull (type 6) quantiles of the --num-samples members. Needs --num-samples >= 2; K '
                 'members cover at most (K - 1) / (K + 1), the report states what a calibrated ensemble of that size attains. '
                 'Default: off.')


def add_interval_flag(p, scope: str):
    """--interval L of analyze / visualize; the default None means off"""
    p.add_argument('--interval', type=float, default=None, help=f'[{scope}] ' + INTERVAL_HELP)


def checked_interval(args, num_samples: int):
    """--interval L of analyze / visualize -> L, or None when off"""
    L = getattr(args, 'interval', None)
    if L is None:
        return None
    L = float(L)
    if not 0.0 < L < 1.0:
        raise SystemExit(f"--interval {L} must lie strictly between 0 and 1 (the interval's nominal coverage)")
    if num_samples < 2:
        raise SystemExit(f"--interval needs --num-samples >= 2, got {num_samples}: an interval is made of the order statistics "
                         f"of an ensemble")
    return L


X0_CLIP_HELP = ('keep the x0 the sampler predicts at every step inside the range each label column took in the training '
                'windows (`train --record-range`): `range` clamps it to the recorded [min, max], `dynamic` is dynamic '
                'thresholding (Saharia et al. 2022) in units of each column\'s half range, the --x0-clip-quantile of one '
                'window. Its effect on label accuracy of trained checkpoints is unmeasured. Default: off.')


def add_x0_clip_flags(p, scope: str):
    """--x0-clip {off,range,dynamic} --x0-clip-quantile P --x0-clip-margin M of analyze / visualize"""
    p.add_argument('--x0-clip', type=str, default='off', choices=['off', 'range', 'dynamic'], help=f'[{scope}] ' + X0_CLIP_HELP)
    p.add_argument('--x0-clip-quantile', type=float, default=0.995,
                   help=f'[{scope}] the quantile P in (0, 1] of --x0-clip dynamic (nearest rank over one window).')
    p.add_argument('--x0-clip-margin', type=float, default=0.0,
                   help=f'[{scope}] widen every column\'s recorded range by M times its half width on both sides (M >= 0).')


def checked_x0_clip(args, model):
    """--x0-clip of analyze / visualize, once the checkpoint is loaded -> an X0Clip over the 30 label columns (the recorded
    range of each, widened by the margin), or None when off"""
    mode = getattr(args, 'x0_clip', 'off')
    if mode == 'off':
        return None
    P, M = float(getattr(args, 'x0_clip_quantile', 0.995)), float(getattr(args, 'x0_clip_margin', 0.0))
    if not 0.0 < P <= 1.0:
        raise SystemExit(f"--x0-clip-quantile {P} must lie in (0, 1]")
    if not M >= 0.0:
        raise SystemExit(f"--x0-clip-margin {M} must be >= 0 (it widens the recorded range)")
    r = getattr(model, 'column_range', None)
    if r is None:
        raise SystemExit(f"--x0-clip {mode} takes its bounds from the column ranges recorded in training: this checkpoint has "
                         f"none (train it with `train --record-range`)")
    from ..diffusion.sampler import X0Clip
    from ..models.DiffusionLabelPredictor import LABEL_WIDTH
    r = torch.as_tensor(r, dtype=torch.float64)[-LABEL_WIDTH:]
    half = (r[:, 1] - r[:, 0]) / 2.0
    return X0Clip((r[:, 0] - M * half).tolist(), (r[:, 1] + M * half).tolist(), mode=mode, quantile=P)


def checked_guidance(args, model) -> float:
    """--guidance S of analyze / visualize, once the checkpoint is loaded: refused for a denoiser that never saw the null
    condition"""
    s = float(getattr(args, 'guidance', 0.0))
    if s != 0.0 and not float(getattr(model, 'cond_drop', 0.0)) > 0.0:
        raise SystemExit(f"--guidance {s} needs a denoiser trained with condition dropout (`train --cond-drop P`, P > 0): this "
                         f"checkpoint's cond_drop is 0, so it has no unconditional prediction to guide away from")
    return s
