"""`main.py visualize` -- flag surface of src/cli/visualize.py:21-56 kept; the body of the reference command
is a nimblephysics NimbleGUI browser playback (:126-258), which is third-party GUI code outside the GPU hot
path.  What IS on the path -- a batch-1 model forward + loss evaluation per tick
(:157-200) -- is run here over the first windows of the split and printed, so a checkpoint can be inspected
without the GUI.

`--trial-frames F` (diffusion-transformer checkpoints) is the command-line route to stitched trial sampling
(models/DiffusionLabelPredictor.predict_trial): F consecutive frames of a trial, read at the dataset's frame stride, are
labelled as ONE sequence of overlapping windows and printed next to the labels the per-window sampler gives on disjoint
windows of the same frames.  With `--sample-eta E --num-samples K` (E > 0 or K > 1) both are posterior ensembles
(predict_trial_ensemble, and the per-window predictor with the same eta and K): the labels printed are the members' means,
and one more line per trial and label key reports the mean standard deviation over the K members.  `--sampler dpmpp2m`
runs both loops with DPM-Solver++(2M); it is deterministic and refuses E > 0 or K > 1.  `--sampler dpmpp2m_sde` is its
stochastic form and takes both; it belongs with `--sample-spacing logsnr`."""
import argparse
import os

import torch

from ..loss.RegressionLossEvaluator import RegressionLossEvaluator
from ..data.AddBiomechanicsDataset import LOSS_KEY_ORDER
from ..diffusion.schedule import STITCH_BLENDS, stitch_layout
from ._common import (GUIDANCE_HELP, LABEL_NAMES, add_additive_flags, add_component_flags, add_interval_flag,
                      add_resample_flags, add_x0_clip_flags, checked_guidance, checked_interval, checked_resample,
                      checked_x0_clip, dtype_of, is_diffusion, open_dataset, pick_device)
from .abstract_command import AbstractCommand
from .analyze import window_subject, window_trial



class VisualizeCommand(AbstractCommand):
    def __init__(self):
        super().__init__()

    def register_subcommand(self, subparsers: argparse._SubParsersAction):
        p = subparsers.add_parser('visualize', help='Visualize the performance of a model on dataset.')
        p.add_argument('--dataset-home', type=str, default='../data')
        p.add_argument('--model-type', type=str, default='feedforward')
        p.add_argument('--output-data-format', type=str, default='all_frames', choices=['all_frames', 'last_frame'])
        p.add_argument('--checkpoint-dir', type=str, default='../checkpoints')
        p.add_argument('--geometry-folder', type=str, default=None)
        p.add_argument('--history-len', type=int, default=50)
        p.add_argument('--stride', type=int, default=5)
        p.add_argument('--dropout', action='store_true')
        p.add_argument('--dropout-prob', type=float, default=0.5)
        p.add_argument('--hidden-dims', type=int, nargs='+', default=[512, 512])
        p.add_argument('--batchnorm', action='store_true')
        p.add_argument('--activation', type=str, default='sigmoid')
        p.add_argument('--batch-size', type=int, default=32)
        p.add_argument('--short', action='store_true')
        add_component_flags(p, train_defaults=True)
        add_additive_flags(p)
        p.add_argument('--num-frames', type=int, default=8, help='How many windows to evaluate and print.')
        p.add_argument('--use-ema', action='store_true', default=False,
                       help='Load the EMA weights of the checkpoint (`train --ema-decay`) instead of its last weights.')
        p.add_argument('--trial-frames', type=int, default=0,
                       help='[diffusion-transformer] label this many consecutive frames of a trial (at the frame stride) as '
                            'one stitched sequence and print them next to the per-window labels; --num-frames trials.')
        p.add_argument('--trial-hop', type=int, default=None,
                       help='[--trial-frames] frames between the starts of the overlapping windows (default: window // 2).')
        p.add_argument('--trial-blend', type=str, default='ramp', choices=list(STITCH_BLENDS),
                       help='[--trial-frames] how the windows that cover a frame are blended.')
        p.add_argument('--sample-steps', type=int, default=100, help='[--trial-frames] steps of the sampling loop.')
        p.add_argument('--sample-seed', type=int, default=0, help='[--trial-frames] seed of the start noise.')
        p.add_argument('--sample-eta', type=float, default=0.0,
                       help='[--trial-frames] eta of the sampler: 0 = deterministic DDIM, 1 = DDPM ancestral sampling.')
        p.add_argument('--num-samples', type=int, default=1,
                       help='[--trial-frames] posterior samples per trial and per window; the means are printed and the '
                            'spread over the members reported.')
        p.add_argument('--sampler', type=str, default='ddim', choices=['ddim', 'dpmpp2m', 'dpmpp2m_sde'],
                       help='[--trial-frames] update of both sampling loops: first-order DDIM, DPM-Solver++(2M) '
                            '(deterministic: needs --sample-eta 0 and --num-samples 1), or dpmpp2m_sde, its stochastic form '
                            '(takes --sample-eta > 0 and --num-samples > 1; use it with --sample-spacing logsnr).')
        p.add_argument('--guidance', type=float, default=0.0, help='[--trial-frames] ' + GUIDANCE_HELP)
        add_resample_flags(p, '--trial-frames')
        add_interval_flag(p, '--trial-frames')
        add_x0_clip_flags(p, '--trial-frames')
        p.add_argument('--sample-spacing', type=str, default='time', choices=['time', 'logsnr'],
                       help='[--trial-frames] sampling grid of both loops: uniform in the timestep, or uniform in log-SNR '
                            '(the grid for few-step dpmpp2m / dpmpp2m_sde sampling).')

    def run(self, args: argparse.Namespace):
        if 'command' in args and args.command != 'visualize':
            return False
        try:
            import nimblephysics  # noqa: F401
            have_gui = True
        except ImportError:
            have_gui = False
        checkpoint_dir = os.path.join(os.path.abspath(args.checkpoint_dir), args.model_type)
        device = pick_device(args)
        if getattr(args, 'trial_frames', 0):
            return self.run_trials(args, checkpoint_dir, device)
        dataset = open_dataset(args, 'test', args.history_len, args.stride, args.output_data_format,
                               self.ensure_geometry(args.geometry_folder))
        model = self.get_model(dataset.num_dofs, dataset.num_contact_bodies, args.model_type,
                               history_len=args.history_len, stride=args.stride, hidden_dims=args.hidden_dims,
                               activation=args.activation, batchnorm=args.batchnorm, dropout=args.dropout,
                               dropout_prob=args.dropout_prob, root_history_len=10,
                               output_data_format=args.output_data_format, device=device,
                               compute_dtype=dtype_of(args)).to(device)
        self.load_latest_checkpoint(model, checkpoint_dir=checkpoint_dir, use_ema=getattr(args, 'use_ema', False))
        model.eval()
        evaluator = RegressionLossEvaluator(dataset=dataset, split='test', device=device)
        if not have_gui:
            print("nimblephysics is not installed: the NimbleGUI playback is unavailable; printing per-window "
                  "predictions vs labels instead.")
        with torch.no_grad():
            for frame in range(min(args.num_frames, len(dataset))):
                inputs, labels, subj, trial = dataset[frame]
                inputs = {k: v.unsqueeze(0) for k, v in inputs.items()}
                labels = {k: v.unsqueeze(0) for k, v in labels.items()}
                outputs = model(inputs)
                loss = evaluator(inputs, outputs, labels, [subj], [trial], args)
                print(f"window {frame}: loss {float(loss):.6f}")
        evaluator.print_report(args)
        return True

    def run_trials(self, args: argparse.Namespace, checkpoint_dir: str, device) -> bool:
        """--trial-frames F: for each of the first --num-frames trials (trial k starts at window k F of the split) the four
        label blocks of its F frames from predict_trial, and from the per-window sampler on the disjoint windows at 0, T,
        2 T, ... plus a last one ending on the last frame (a frame takes the first window that covers it).  Per frame one
        row with the force block of both; per trial and label key the RMS error of both against the labels, their RMS
        difference, and for the force block the mean jump |x[f] - x[f - 1]| across the per-window boundaries.  With
        --sample-eta > 0 or --num-samples > 1 both are ensemble means (predict_trial_ensemble; the per-window predictor with
        the same eta and K), and one more line per trial and label key gives the mean standard deviation over the members --
        and, with --interval L, the mean width of the level-L interval of both (DiffusionLabelPredictor, interval)."""
        from ..models.DiffusionLabelPredictor import DiffusionLabelPredictor
        F = int(args.trial_frames)
        if not is_diffusion(args.model_type):
            raise SystemExit("--trial-frames labels a trial with a diffusion denoiser: pass --model-type diffusion-transformer")
        if args.sample_steps < 1 or args.num_frames < 1:
            raise SystemExit("--sample-steps and --num-frames must be >= 1")
        eta, num_samples = float(getattr(args, 'sample_eta', 0.0)), int(getattr(args, 'num_samples', 1))
        if not 0.0 <= eta <= 1.0 or num_samples < 1:
            raise SystemExit("--sample-eta must be in [0, 1] and --num-samples >= 1")
        solver = getattr(args, 'sampler', 'ddim')
        resample = checked_resample(args, args.sample_steps, eta, solver)
        interval = checked_interval(args, num_samples)
        # a resampled loop keys its re-noise draws by trial id, so it takes the ensemble path (at eta = 0, also at K = 1)
        ensemble = eta > 0.0 or num_samples > 1 or resample is not None and resample[1] > 1
        if solver == 'dpmpp2m' and ensemble:
            raise SystemExit("--sampler dpmpp2m is deterministic: it needs --sample-eta 0 and --num-samples 1")
        view = self.diffusion_view(args, 'test', self.ensure_geometry(args.geometry_folder))
        dataset = view.dataset
        model = self.diffusion_model(args, view, device)
        T = getattr(model, 'window', None)
        if T is None:
            raise SystemExit(f"--trial-frames needs a denoiser with a window (--model-type diffusion-transformer); "
                             f"{args.model_type} has none")
        self.load_latest_checkpoint(model, checkpoint_dir=checkpoint_dir, use_ema=getattr(args, 'use_ema', False))
        model.eval()
        hop = T // 2 if args.trial_hop is None else int(args.trial_hop)
        try:
            W = stitch_layout(F, T, hop, args.trial_blend)[0].numel()
            start, cover = stitch_layout(F, T, T, 'uniform')[:2]        # the disjoint windows of the per-window sampler
        except ValueError as e:
            raise SystemExit(f"--trial-frames / --trial-hop: {e}")
        predictor = DiffusionLabelPredictor(model, args.sample_steps, seed=args.sample_seed,
                                            output_data_format=args.output_data_format, eta=eta, num_samples=num_samples,
                                            solver=solver, spacing=getattr(args, 'sample_spacing', 'time'),
                                            guidance=checked_guidance(args, model), resample=resample, interval=interval,
                                            x0_clip=checked_x0_clip(args, model))
        gather = start.long()[:, None] + torch.arange(T)[None, :]      # [Wd, T] trial frames of the disjoint windows
        w0 = cover[:, 0].long()
        t0 = torch.arange(F) - start.long()[w0]
        seams = start[1:].long()
        done = 0
        for k in range(args.num_frames):
            index = k * F
            if index >= len(dataset):
                break
            try:
                inputs, labels, subj, trial = dataset.read_trial(index, F)
            except ValueError as e:
                print(f"trial {k}: skipped ({e})")
                continue
            inputs = {key: v.unsqueeze(0) for key, v in inputs.items()}
            if ensemble:
                stitched = predictor.predict_trial_ensemble(inputs, hop=hop, blend=args.trial_blend, draw=k)
                stitched_std, stitched_iv = predictor.last_std, predictor.last_interval
            else:
                stitched = predictor.predict_trial(inputs, hop=hop, blend=args.trial_blend, draw=k)
            windows = predictor({key: v[0, gather] for key, v in inputs.items()}, draw=k * gather.shape[0])
            windows_std = predictor.last_std if ensemble else None
            windows_iv = predictor.last_interval
            print(f"trial {k} ({window_subject(dataset, [subj])} / {window_trial(dataset, [subj], [trial])}): {F} frames, "
                  f"stitched as {W} windows of {T} every {hop} frames ({args.trial_blend}) | {gather.shape[0]} disjoint windows")
            print(f"{'frame':>5} {'win':>3}  {'stitched force':<48} | per-window force")
            fmt = lambda row: ' '.join(f'{float(v):+7.3f}' for v in row)
            sf = stitched[LOSS_KEY_ORDER[1]][0].cpu()
            wf = windows[LOSS_KEY_ORDER[1]].cpu()[w0, t0]
            for f in range(F):
                print(f"{f:>5} {int(w0[f]):>3}  {fmt(sf[f])} | {fmt(wf[f])}")
            rms = lambda d: float(d.double().pow(2).mean().sqrt())
            for name, key in zip(LABEL_NAMES, LOSS_KEY_ORDER):
                s, w, y = stitched[key][0].cpu(), windows[key].cpu()[w0, t0], labels[key].float()
                print(f"trial {k} {name:>6}: RMS err stitched {rms(s - y):.6f}, per-window {rms(w - y):.6f}, "
                      f"RMS stitched - per-window {rms(s - w):.6f}")
            if ensemble:
                for name, key in zip(LABEL_NAMES, LOSS_KEY_ORDER):
                    ss, ws = stitched_std[key][0].cpu(), windows_std[key].cpu()[w0, t0]
                    widths = ""
                    if interval is not None:
                        width = lambda iv: (iv['hi'][key] - iv['lo'][key]).cpu().double()
                        widths = (f"; mean width of the {interval:g} interval stitched {float(width(stitched_iv)[0].mean()):.6f}, "
                                  f"per-window {float(width(windows_iv)[w0, t0].mean()):.6f}")
                    print(f"trial {k} {name:>6}: mean std over {num_samples} samples stitched {float(ss.double().mean()):.6f}, "
                          f"per-window {float(ws.double().mean()):.6f}{widths}")
            if seams.numel():
                jump = lambda x: float((x[seams] - x[seams - 1]).abs().mean())
                print(f"trial {k}  force: mean jump across the {seams.numel()} per-window boundaries: stitched {jump(sf):.6f}, "
                      f"per-window {jump(wf):.6f}")
            done += 1
        if not done:
            raise SystemExit(f"--trial-frames {F}: no trial of the split holds {F} frames at stride {args.stride}")
        return True
