"""`main.py analyze` -- batch-size-1 evaluation over the dev split, then the train split (drop-in for
src/cli/analyze.py:49-242): same flags/defaults (:23-47; --predict-grf-components [1] only), loads the
latest checkpoint from <checkpoint-dir>/<model-type>/, runs model forward + loss evaluator under no_grad,
appends one row per window to dev_analysis.csv / train_analysis.csv, prints the averaged report.
Forward and loss run on the HIP kernels (batch 1 is launch-latency bound; no backward here)."""
import argparse
import csv
import logging
import os

import torch
from torch.utils.data import DataLoader

from ..data.AddBiomechanicsDataset import LOSS_KEY_ORDER
from ..diffusion.ensemble import calibrated_coverage
from ..loss.RegressionLossEvaluator import RegressionLossEvaluator
from ._common import (GUIDANCE_HELP, LABEL_NAMES, add_additive_flags, add_component_flags, add_interval_flag,
                      add_resample_flags, add_x0_clip_flags, checked_guidance, checked_interval, checked_resample,
                      checked_x0_clip, dtype_of, is_diffusion, open_dataset, pick_device)
from .abstract_command import AbstractCommand


class AnalyzeCommand(AbstractCommand):
    def __init__(self):
        super().__init__()

    def register_subcommand(self, subparsers: argparse._SubParsersAction):
        p = subparsers.add_parser('analyze', help='Evaluate the performance of a model on dataset.')
        p.add_argument('--dataset-home', type=str, default='../data', help='The path to the AddBiomechanics dataset.')
        p.add_argument('--model-type', type=str, default='feedforward', help='The model to evaluate.')
        p.add_argument('--no-wandb', action='store_true', default=False, help='Do not log to Weights and Biases.')
        p.add_argument('--output-data-format', type=str, default='all_frames', choices=['all_frames', 'last_frame'])
        p.add_argument('--checkpoint-dir', type=str, default='../checkpoints')
        p.add_argument('--geometry-folder', type=str, default=None)
        p.add_argument('--history-len', type=int, default=50)
        p.add_argument('--stride', type=int, default=5)
        p.add_argument('--hidden-dims', type=int, nargs='+', default=[512, 512])
        p.add_argument('--activation', type=str, default='sigmoid')
        p.add_argument('--short', type=bool, default=False)
        p.add_argument('--data-loading-workers', type=int, default=3)
        add_component_flags(p, train_defaults=False)
        add_additive_flags(p)
        p.add_argument('--max-windows', type=int, default=0, help='Stop each split after this many windows (0 = all).')
        p.add_argument('--sample-steps', type=int, default=100,
                       help='[diffusion models] DDIM steps of the masked sampler that infers the label columns.')
        p.add_argument('--sample-seed', type=int, default=0,
                       help='[diffusion models] seed of the start noise (window i of a split draws from (seed, i)).')
        p.add_argument('--sample-batch', type=int, default=1,
                       help='[diffusion models] windows per sampler call; still one CSV row per window.')
        p.add_argument('--sample-eta', type=float, default=0.0,
                       help='[diffusion models] eta of the sampler: 0 = deterministic DDIM, 1 = DDPM ancestral sampling.')
        p.add_argument('--num-samples', type=int, default=1,
                       help='[diffusion models] posterior samples per window; the mean is evaluated, the spread reported.')
        p.add_argument('--sampler', type=str, default='ddim', choices=['ddim', 'dpmpp2m', 'dpmpp2m_sde'],
                       help='[diffusion models] update of the sampling loop: first-order DDIM, or DPM-Solver++(2M), second '
                            'order with one denoiser evaluation per step, like DDIM (deterministic: needs --sample-eta 0), '
                            'or dpmpp2m_sde, its stochastic form (SDE-DPM-Solver++(2M)): takes --sample-eta > 0 and '
                            '--num-samples > 1; use it with --sample-spacing logsnr.')
        p.add_argument('--sample-spacing', type=str, default='time', choices=['time', 'logsnr'],
                       help='[diffusion models] sampling grid: uniform in the timestep, or uniform in log-SNR (no need for '
                            '--sample-steps to divide the training steps; the grid for few-step dpmpp2m / dpmpp2m_sde sampling).')
        p.add_argument('--guidance', type=float, default=0.0, help='[diffusion models] ' + GUIDANCE_HELP)
        add_resample_flags(p, 'diffusion models')
        add_interval_flag(p, 'diffusion models')
        add_x0_clip_flags(p, 'diffusion models')
        p.add_argument('--use-ema', action='store_true', default=False,
                       help='Evaluate the EMA weights of the checkpoint (`train --ema-decay`) instead of its last weights.')

    def run(self, args: argparse.Namespace):
        if 'command' in args and args.command != 'analyze':
            return False
        checkpoint_dir = os.path.join(os.path.abspath(args.checkpoint_dir), args.model_type)
        os.makedirs(checkpoint_dir, exist_ok=True)
        device = pick_device(args)
        geometry = self.ensure_geometry(args.geometry_folder)
        if is_diffusion(args.model_type):
            return self.run_diffusion(args, checkpoint_dir, device, geometry)
        model = None
        for split, csv_name in (('dev', 'dev_analysis.csv'), ('train', 'train_analysis.csv')):
            logging.info(f'## Loading {split} dataset:')
            dataset = open_dataset(args, split, args.history_len, args.stride, args.output_data_format, geometry)
            if model is None:
                model = self.get_model(dataset.num_dofs, dataset.num_contact_bodies, args.model_type,
                                       history_len=args.history_len, hidden_dims=args.hidden_dims,
                                       activation=args.activation, stride=args.stride, batchnorm=False, dropout=False,
                                       dropout_prob=0.0, root_history_len=10,
                                       output_data_format=args.output_data_format, device=device,
                                       compute_dtype=dtype_of(args)).to(device)
                self.load_latest_checkpoint(model, checkpoint_dir=checkpoint_dir, use_ema=getattr(args, 'use_ema', False))
                model.eval()
            evaluator = RegressionLossEvaluator(dataset=dataset, split=split, device=device)
            loader = DataLoader(dataset, batch_size=1, shuffle=False, num_workers=args.data_loading_workers)
            compute_report = bool(getattr(dataset, 'skeletons', None))   # inverse dynamics needs nimble skeletons
            n = len(loader)
            with torch.no_grad(), open(os.path.join(checkpoint_dir, csv_name), 'a') as f:
                writer = None
                for i, (inputs, labels, subj, trial) in enumerate(loader):
                    outputs = model(inputs)
                    evaluator(inputs, outputs, labels, subj, trial, args, compute_report=compute_report)
                    stats = {"sub_name": window_subject(dataset, subj), "trial_name": window_trial(dataset, subj, trial)}
                    writer = writer or csv.DictWriter(f, fieldnames=stats.keys())
                    writer.writerow(stats)
                    last = (i == n - 1) or (args.max_windows and i + 1 >= args.max_windows)
                    if (i + 1) % 100 == 0 or last:
                        logging.info(f'  - Batch {i + 1}/{n}')
                    if (i + 1) % 1000 == 0 or last:
                        evaluator.print_report(args, reset=False, log_to_wandb=not args.no_wandb)
                    if last:
                        break
            print(f'Final {split} results:')
            evaluator.print_report(log_to_wandb=False)
        return True

    def run_diffusion(self, args: argparse.Namespace, checkpoint_dir: str, device, geometry) -> bool:
        """the diffusion denoisers: the label columns of every window are inferred by the masked DDIM sampler
        (models/DiffusionLabelPredictor.py) from the observed input columns, then evaluated, written and reported exactly
        as the regression models' outputs are"""
        from ..models.DiffusionLabelPredictor import DiffusionLabelPredictor
        if args.sample_batch < 1 or args.sample_steps < 1:
            raise SystemExit("--sample-batch and --sample-steps must be >= 1")
        eta, num_samples = getattr(args, 'sample_eta', 0.0), getattr(args, 'num_samples', 1)
        if not 0.0 <= eta <= 1.0 or num_samples < 1:
            raise SystemExit("--sample-eta must be in [0, 1] and --num-samples >= 1")
        solver, spacing = getattr(args, 'sampler', 'ddim'), getattr(args, 'sample_spacing', 'time')
        if solver == 'dpmpp2m' and eta > 0.0:
            raise SystemExit("--sampler dpmpp2m is deterministic: it needs --sample-eta 0")
        resample = checked_resample(args, args.sample_steps, eta, solver)
        interval = checked_interval(args, num_samples)
        predictor = None
        for split, csv_name in (('dev', 'dev_analysis.csv'), ('train', 'train_analysis.csv')):
            logging.info(f'## Loading {split} dataset:')
            view = self.diffusion_view(args, split, geometry)
            dataset = view.dataset
            if predictor is None:
                model = self.diffusion_model(args, view, device)
                self.load_latest_checkpoint(model, checkpoint_dir=checkpoint_dir, use_ema=getattr(args, 'use_ema', False))
                model.eval()
                predictor = DiffusionLabelPredictor(model, args.sample_steps, seed=args.sample_seed,
                                                    output_data_format=args.output_data_format, eta=eta,
                                                    num_samples=num_samples, solver=solver, spacing=spacing,
                                                    guidance=checked_guidance(args, model), resample=resample,
                                                    interval=interval, x0_clip=checked_x0_clip(args, model))
            evaluator = RegressionLossEvaluator(dataset=dataset, split=split, device=device)
            loader = DataLoader(dataset, batch_size=args.sample_batch, shuffle=False, num_workers=args.data_loading_workers)
            compute_report = bool(getattr(dataset, 'skeletons', None))
            n = len(dataset)
            if args.max_windows:
                n = min(n, args.max_windows)
            i = 0
            spread = EnsembleSpread() if num_samples > 1 else None
            calibration = EnsembleCalibration(num_samples, interval) if interval is not None else None
            with torch.no_grad(), open(os.path.join(checkpoint_dir, csv_name), 'a') as f:
                writer = None
                for inputs, labels, subj, trial in loader:
                    outputs = predictor(inputs, labels, draw=i)
                    if spread is not None:
                        spread.add(outputs, predictor.last_std, labels, min(len(subj), n - i))
                    if calibration is not None:
                        calibration.add(predictor.last_interval, predictor.last_crps, predictor.last_rank,
                                        predictor.last_inside, min(len(subj), n - i))
                    for b in range(min(len(subj), n - i)):
                        one = lambda d: {k: v[b:b + 1] for k, v in d.items()}
                        evaluator(one(inputs), one(outputs), one(labels), subj[b:b + 1], trial[b:b + 1], args,
                                  compute_report=compute_report)
                        stats = {"sub_name": window_subject(dataset, subj[b:b + 1]),
                                 "trial_name": window_trial(dataset, subj[b:b + 1], trial[b:b + 1])}
                        writer = writer or csv.DictWriter(f, fieldnames=stats.keys())
                        writer.writerow(stats)
                        i += 1
                        if i % 100 == 0 or i == n:
                            logging.info(f'  - Batch {i}/{n}')
                        if i % 1000 == 0 or i == n:
                            evaluator.print_report(args, reset=False, log_to_wandb=not args.no_wandb)
                    if i >= n:
                        break
            print(f'Final {split} results:')
            evaluator.print_report(log_to_wandb=False)
            if spread is not None:
                print(spread.line(split, num_samples))
            if calibration is not None:
                print(calibration.line(split))
                print(calibration.histogram_line(split))
        return True


class EnsembleSpread:
    """per label key, over the windows of a split: the mean of the ensemble's per-element standard deviation and the RMS
    error of the ensemble mean against the labels (report bookkeeping on the host, in float64)"""

    def __init__(self):
        self.n = {}
        self.std_sum = {}
        self.sq_sum = {}

    def add(self, mean, std, labels, windows: int):
        for k in mean:
            m, s, y = (t[:windows].detach().cpu().double() for t in (mean[k], std[k], labels[k]))
            self.n[k] = self.n.get(k, 0) + m.numel()
            self.std_sum[k] = self.std_sum.get(k, 0.0) + float(s.sum())
            self.sq_sum[k] = self.sq_sum.get(k, 0.0) + float(((m - y) ** 2).sum())

    def line(self, split: str, num_samples: int) -> str:
        parts = [f'{k}: mean std {self.std_sum[k] / self.n[k]:.6g}, RMS err of mean {(self.sq_sum[k] / self.n[k]) ** 0.5:.6g}'
                 for k in self.n]
        return f'Ensemble spread ({split}, {num_samples} samples per window): ' + '; '.join(parts)


class EnsembleCalibration:
    """per label key, over the windows of a split, from the predictor's order statistics (hip.ensemble_order): how often the
    label lies inside the level-L interval, the interval's mean width, the mean fair CRPS, and the histogram of the label's
    rank among the K members (K + 1 bins; flat for a calibrated ensemble).  Report bookkeeping on the host, in float64 and
    int."""

    def __init__(self, num_samples: int, level: float):
        self.K, self.level = int(num_samples), float(level)
        self.names = dict(zip(LOSS_KEY_ORDER, LABEL_NAMES))
        self.n = {}
        self.inside = {}
        self.width_sum = {}
        self.crps_sum = {}
        self.hist = {}

    def add(self, interval, crps, rank, inside, windows: int):
        for k in crps:
            lo, hi, c = (t[:windows].detach().cpu().double() for t in (interval['lo'][k], interval['hi'][k], crps[k]))
            r, hit = rank[k][:windows].detach().cpu().long(), inside[k][:windows].detach().cpu().long()
            self.n[k] = self.n.get(k, 0) + c.numel()
            self.inside[k] = self.inside.get(k, 0) + int(hit.sum())
            self.width_sum[k] = self.width_sum.get(k, 0.0) + float((hi - lo).sum())
            self.crps_sum[k] = self.crps_sum.get(k, 0.0) + float(c.sum())
            counts = torch.bincount(r.reshape(-1), minlength=self.K + 1).tolist()
            self.hist[k] = [a + b for a, b in zip(self.hist.get(k, [0] * (self.K + 1)), counts)]

    def line(self, split: str) -> str:
        cal = calibrated_coverage(self.level, self.K)
        parts = [f'{self.names.get(k, k)}: coverage {self.inside[k] / self.n[k]:.4f} (calibrated ensemble: {cal:.4f}), mean width '
                 f'{self.width_sum[k] / self.n[k]:.6g}, CRPS {self.crps_sum[k] / self.n[k]:.6g}' for k in self.n]
        return f'Ensemble calibration ({split}, {self.K} samples per window, level {self.level:g}): ' + '; '.join(parts)

    def histogram_line(self, split: str) -> str:
        return f'Rank histogram ({split}): ' + '; '.join(f"{self.names.get(k, k)}: [{' '.join(str(c) for c in self.hist[k])}]"
                                                           for k in self.hist)


def window_subject(dataset, subj) -> str:
    i = int(subj[0]) if len(subj) else 0
    if hasattr(dataset, 'subject_paths'):
        return os.path.basename(dataset.subject_paths[i])
    return f"synthetic_subject_{i}"


def window_trial(dataset, subj, trial) -> str:
    j = int(trial[0]) if len(trial) else 0
    if hasattr(dataset, 'subjects'):
        return str(dataset.subjects[int(subj[0])].getTrialName(j))
    return f"window_{j}"
