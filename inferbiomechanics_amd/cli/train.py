"""`main.py train` -- the DDP training driver (drop-in for src/cli/train.py).

Flags and defaults are the reference's (train.py:24-69).  Control flow kept: per epoch a no-grad dev
evaluation, a barrier, then the training loop with a report every 1000 batches and a rank-0 checkpoint
``<checkpoint-dir>/epoch_{E}_batch_{i}.pt`` holding {'epoch', 'model_state_dict', 'optimizer_state_dict'}
(train.py:201-291).  What differs is the loop BODY: ``zero_grad -> model -> loss -> backward -> step``
(train.py:240-284) is one fused launch sequence (engine.HipTrainer): HIP kernels, gradients in one flat
buffer, RCCL all-reduce in buckets overlapped with the backward, one optimizer launch, hipGraph replay, no
per-step host sync (the reference syncs 8x per step through `.item()` and uploads to wandb every step).

Reference defects fixed on the way: undefined DEV / mp / time (train.py:136,152,212), no
--device flag, checkpoint keys saved with DDP's `module.` prefix, checkpoint dir join that drops the model
type, `git_hash` storing the function object; wandb is optional.
"""
import argparse
import logging
import os
import time
from datetime import timedelta
from typing import Dict, List

import torch
import torch.distributed as dist
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler as DS

from ..engine import HipTrainer
from ..loss.DiffusionLossEvaluator import DiffusionLossEvaluator
from ..loss.RegressionLossEvaluator import RegressionLossEvaluator
from ._common import (add_additive_flags, add_component_flags, dtype_of, is_diffusion, open_dataset, pick_device)
from .abstract_command import MODEL_TYPES, AbstractCommand
from .utilities import get_git_hash, has_uncommitted_changes

DEV = 'dev'   # the dev split directory (analyze.py:80); the reference train.py uses an undefined name here


class TrainCommand(AbstractCommand):
    last_run_stats = None        # {"epoch", "steps", "seconds", "windows_per_s"} of the last finished training epoch

    def __init__(self):
        super().__init__()

    def register_subcommand(self, subparsers: argparse._SubParsersAction):
        p = subparsers.add_parser('train', help='Train a model on the AddBiomechanics dataset')
        p.add_argument('--dataset-home', type=str, default='../data', help='The path to the AddBiomechanics dataset.')
        p.add_argument('--no-wandb', action='store_true', default=False, help='Do not log this run to Weights and Biases.')
        p.add_argument('--model-type', type=str, default='feedforward', choices=MODEL_TYPES, help='The model to train.')
        p.add_argument('--output-data-format', type=str, default='all_frames', choices=['all_frames', 'last_frame'],
                       help='Output for all frames in a window or only the last frame.')
        p.add_argument('--checkpoint-dir', type=str, default='../checkpoints',
                       help='Where checkpoints are saved; training resumes from the latest one in this directory.')
        p.add_argument('--geometry-folder', type=str, default=None, help='Path to the Geometry folder with bone mesh data.')
        p.add_argument('--history-len', type=int, default=50, help='The number of timesteps of context in the inputs.')
        p.add_argument('--stride', type=int, default=5, help='The timestep gap between frames in the context window.')
        p.add_argument('--learning-rate', type=float, default=1e-4, help='The learning rate for weight updates.')
        p.add_argument('--dropout', action='store_true', help='Apply dropout?')
        p.add_argument('--dropout-prob', type=float, default=0.5, help='Dropout prob')
        p.add_argument('--hidden-dims', type=int, nargs='+', default=[512, 512], help='Hidden dims across layers.')
        p.add_argument('--batchnorm', action='store_true', help='Apply batchnorm?')
        p.add_argument('--activation', type=str, default='sigmoid', help='Which activation func?')
        p.add_argument('--epochs', type=int, default=10, help='The number of epochs to run training for.')
        p.add_argument('--opt-type', type=str, default='rmsprop', help='The optimizer used to adapt the weights.')
        p.add_argument('--batch-size', type=int, default=64, help='The batch size (per process).')
        p.add_argument('--short', action='store_true', help='Use very short datasets to test quickly.')
        p.add_argument('--data-loading-workers', type=int, default=1, help='Worker processes that load data.')
        add_component_flags(p, train_defaults=True)
        p.add_argument('--trial-filter', type=str, nargs='+', default=[""], help='What kind of trials to train/test on.')
        p.add_argument('--compute-report', action='store_true', default=False,
                       help='Compute inverse dynamics reports during loss evaluation.')
        add_additive_flags(p)
        p.add_argument('--max-steps', type=int, default=0, help='Stop each epoch after this many batches (0 = all).')
        p.add_argument('--report-every', type=int, default=1000, help='Batches between reports / checkpoints.')
        p.add_argument('--eager', action='store_true',
                       help='Reference-style loop (autograd node + torch.optim + torch DDP) instead of the fused trainer.')
        p.add_argument('--no-graph', action='store_true', help='Do not replay the step from hipGraphs.')
        p.add_argument('--bucket-mb', type=float, default=13.0, help='Gradient all-reduce bucket size (MiB).')
        p.add_argument('--window-cache', type=str, default=None,
                       help='Packed-window file (data/WindowCache.py): loaded if it exists, else built from the training '
                            'set and saved; training then runs from an on-device window cache (one gather launch per '
                            'batch instead of the DataLoader pipeline).  Regression models: packed-window file '
                            '(data/WindowCache.py); diffusion models: a .npy of [N, T, D] motion windows, and the '
                            "step's timesteps / noise are drawn on the device by the same launch; the word `hbm` with "
                            '--synthetic-windows draws the synthetic windows straight into HBM (no file).')
        p.add_argument('--max-dev-steps', type=int, default=0,
                       help='Evaluate at most this many dev batches before each epoch (0 = follow --max-steps).')
        p.add_argument('--loss-every', type=int, default=1,
                       help='[diffusion, --window-cache] keep the device-resident loss of every Nth step for the report.')
        p.add_argument('--seed', type=int, default=None,
                       help='torch.manual_seed for this run (initial weights, dropout masks, diffusion noise).')
        p.add_argument('--ema-decay', type=float, default=0.0,
                       help='Keep an exponential moving average of the weights with this decay, advanced inside the fused '
                            'optimizer launches and saved in the checkpoints (0 = off; 0.999-0.9999 are usual). '
                            '`analyze --use-ema` / `visualize --use-ema` then load it. Not with --eager.')
        p.add_argument('--cond-cols', type=int, default=0,
                       help='[diffusion] Train a denoiser conditioned on the first N columns of every frame: they enter the '
                            'network clean at every noise level, only the other columns are noised and scored. For label '
                            'inference N = feat_dim - 30; `analyze` / `visualize` read N from the checkpoint. 0 = '
                            'unconditional.')
        p.add_argument('--cond-drop', type=float, default=0.0,
                       help='[diffusion, with --cond-cols] Classifier-free guidance training: with probability P a window\'s '
                            'conditioning columns reach the denoiser all zero (the null condition), decided on the device per '
                            'step and window. `analyze --guidance S` / `visualize --guidance S` then sample with the guided '
                            'noise prediction. 0 = off; 0.1-0.2 are usual. Not with --eager.')
        p.add_argument('--record-range', action='store_true', default=False,
                       help='[diffusion, with --window-cache] Record the minimum and maximum every column takes in the '
                            'training windows (one pass over the device-resident cache) and save them in the checkpoints; '
                            '`analyze --x0-clip` / `visualize --x0-clip` take their bounds from there. A resumed run keeps '
                            'the checkpoint\'s record. Default: off.')
        p.add_argument('--standardize', action='store_true', default=False,
                       help='[diffusion] Train on per-column standardised windows z = (x - mean) / scale: the mean and the '
                            'population standard deviation of every column are taken over the training windows when the '
                            'window cache is built (--window-cache; one more pass over its fp32 source) and saved in the '
                            'checkpoints; `analyze` / `visualize` read them from there and give labels in raw units. A '
                            'resumed run keeps the checkpoint\'s statistics (and may then run with --eager); it must be '
                            'given the flag again. With --record-range the range is taken over the standardised table: the '
                            'bounds of --x0-clip are in the sampler\'s units. Default: off.')
        p.add_argument('--no-ema-warmup', action='store_true',
                       help='Use --ema-decay from the first step (default: min(decay, (1 + step) / (10 + step))).')
        p.add_argument('--lr-schedule', choices=['constant', 'linear', 'cosine'], default='constant',
                       help='What the learning rate does after the warmup: stay at --learning-rate, or decay to '
                            '--lr-min-ratio times it at step --lr-total-steps along a line or a half cosine, and stay there. '
                            'The rate of a step is computed inside the fused optimizer launches from the device step counter. '
                            'Not with --eager.')
        p.add_argument('--lr-warmup-steps', type=int, default=0,
                       help='Raise the rate linearly over the first N optimizer steps: step s <= N runs at s / N times '
                            '--learning-rate (0 = no warmup).')
        p.add_argument('--lr-total-steps', type=int, default=0,
                       help='The step at which a linear / cosine decay ends (0 = --epochs x batches per epoch on this rank, '
                            'honouring --max-steps). A resumed run must give the same schedule: pass this explicitly when '
                            '--epochs changes.')
        p.add_argument('--lr-min-ratio', type=float, default=0.0,
                       help='The rate a decay ends at, as a fraction of --learning-rate, in [0, 1].')
        p.add_argument('--weight-decay', type=float, default=0.0,
                       help='Decoupled weight decay (AdamW with --opt-type adam; any --opt-type): each step multiplies the '
                            'weight matrices and embedding tables (parameters with 2 or more dimensions; not biases or '
                            'normalisation gains / offsets) by 1 - rate x W before the update, inside the fused optimizer '
                            'launches, at the rate of that step. Saved in the checkpoints; a resumed run must give the same '
                            'value. Not with --eager. Default: 0 (off).')
        p.add_argument('--max-grad-norm', type=float, default=0.0,
                       help='Clip the gradient to this global L2 norm (torch.nn.utils.clip_grad_norm_): the norm is taken on '
                            'the device and the coefficient applied inside the fused optimizer launch, with no host read per '
                            'step. The step then updates all parameters in one launch behind the last gradient instead of '
                            'per layer. "inf" measures the norm without clipping. Saved in the checkpoints; a resumed run must '
                            'give the same value. Not with --eager. Default: 0 (off).')
        p.add_argument('--loss-weight', type=str, default='off', choices=['off', 'uniform', 'min-snr'],
                       help='Diffusion models: weight each window\'s eps-MSE by its noise level inside the loss launch of the '
                            'fused step. "min-snr" is Min-SNR-gamma (Hang et al. 2023), w_t = min(1, gamma / SNR_t) for '
                            'eps-prediction; "uniform" optimises the unweighted loss through the same launches and exists '
                            'for its report: the periodic report lines then show the unweighted eps-MSE beside the optimised '
                            'loss and its mean per band of noise level. The bf16 MLP denoiser then leaves its one-launch chain '
                            'kernel for the per-op step. Saved in the checkpoints; a resumed run must give the same value. '
                            'Not with --eager. Default: off.')
        p.add_argument('--min-snr-gamma', type=float, default=5.0,
                       help='gamma of --loss-weight min-snr, > 0. Default: 5.')
        p.add_argument('--prediction', type=str, default='eps', choices=['eps', 'x0', 'v'],
                       help='Diffusion models: what the denoiser predicts. "eps" is the noise; "x0" the clean window; "v" is '
                            'sqrt(ab) eps - sqrt(1 - ab) x0 (Salimans & Ho 2022). With x0 or v the target is formed inside the '
                            'loss launch of the fused step, the samplers convert the output into a noise prediction with one '
                            'more launch per step, --loss-weight min-snr takes the form of that prediction, and the reports keep '
                            'showing the eps-MSE, overall and per band of noise level. The bf16 MLP denoiser then leaves its '
                            'one-launch chain kernel for the per-op step. Saved in the checkpoints; a resumed run must give the '
                            'same value. Not with --eager. Default: eps.')
        p.add_argument('--velocity-loss', type=float, default=0.0,
                       help='Diffusion models: weight LAMBDA > 0 of a velocity term in the loss, the squared error of the '
                            'frame-to-frame difference of the predicted clean window (the geometric loss of MDM, Tevet et al. '
                            '2023), weighted per noise level by min(SNR_t, gamma). It is computed inside the loss launch of '
                            'the fused step under every --prediction; the report lines show the term and the velocity error in '
                            'x0 units beside the other numbers. The bf16 MLP denoiser then leaves its one-launch chain kernel '
                            'for the per-op step. Saved in the checkpoints; a resumed run must give the same value. Not with '
                            '--eager. Default: 0 (off).')
        p.add_argument('--velocity-gamma', type=float, default=5.0,
                       help='gamma of --velocity-loss, > 0; inf weights by the plain SNR. Default: 5.')

    # ------------------------------------------------------------------------------------------
    def run(self, args: argparse.Namespace):
        if 'command' in args and args.command != 'train':
            return False
        model_type: str = args.model_type
        checkpoint_dir: str = os.path.join(os.path.abspath(args.checkpoint_dir), model_type)   # as analyze.py:57
        history_len, stride = args.history_len, args.stride
        log_to_wandb: bool = not args.no_wandb
        diffusion = is_diffusion(model_type)

        check_ema_args(args)
        check_lr_schedule(args)
        check_weight_decay_args(args)
        check_max_grad_norm_args(args)
        loss_weight = resolve_loss_weight(args)
        prediction = resolve_prediction(args)
        velocity_loss = resolve_velocity_loss(args)
        check_cond_cols(model_type, getattr(args, 'cond_cols', 0))
        check_cond_drop(args)
        check_record_range(args)
        check_standardize(args)
        if getattr(args, 'seed', None) is not None:
            torch.manual_seed(args.seed)
        geometry = self.ensure_geometry(args.geometry_folder)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC for RCCL (before the first HIP call)
        from .. import ddp_probe
        ddp_probe.prepare_env()                                      # preconditions of captured collectives (ddp_probe.py)
        device = pick_device(args)
        world_size = int(os.environ.get('WORLD_SIZE', '1'))
        distributed = world_size > 1
        if distributed:
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            if os.environ.get('IB_BENCH_REHEARSAL') == '1':
                dist.init_process_group(backend="gloo", timeout=timedelta(hours=1))
            else:
                dist.init_process_group(backend="nccl", timeout=timedelta(hours=1), device_id=device)   # RCCL (train.py:99)
        rank = dist.get_rank() if distributed else 0
        print(f"Running on {world_size} GPUs.")
        print(f"Current device being used for model training and loss evaluation: {device}.")
        if has_uncommitted_changes():
            logging.error("UNCOMMITTED CHANGES IN REPO! This will make it hard to replicate this experiment later")

        wandb = None
        if log_to_wandb:
            try:
                import wandb as _wandb
                wandb = _wandb
                config = dict(args.__dict__)
                config["git_hash"] = get_git_hash()
                group = os.getenv('WANDB_RUN_GROUP', f'ddp_{wandb.util.generate_id()}')
                wandb.init(project="addbiomechanics-baseline", config=config, group=group)
            except ImportError:
                logging.warning("wandb is not installed: continuing without uploads (same as --no-wandb)")
                log_to_wandb = False

        print("Initializing training set...")
        train_dataset = open_dataset(args, 'train', history_len, stride, args.output_data_format, geometry)
        print("Initializing dev set...")
        dev_dataset = open_dataset(args, DEV, history_len, stride, args.output_data_format, geometry)
        # DistributedSampler(shuffle=False, drop_last=True): rank r takes indices r, r+world, ... (train.py:143,149)
        mk = lambda ds: DataLoader(ds, batch_size=args.batch_size, shuffle=False, num_workers=args.data_loading_workers,
                                   persistent_workers=args.data_loading_workers > 0, pin_memory=True, drop_last=diffusion,
                                   sampler=DS(ds, num_replicas=world_size, rank=rank, shuffle=False, drop_last=True))
        train_dataloader, dev_dataloader = mk(train_dataset), mk(dev_dataset)

        print("Initializing model...")
        window = history_len // stride if stride > 1 else history_len
        model = self.get_model(getattr(train_dataset, 'num_dofs', 23), getattr(train_dataset, 'num_contact_bodies', 2),
                               model_type, history_len=history_len, stride=stride, hidden_dims=args.hidden_dims,
                               activation=args.activation, batchnorm=args.batchnorm, dropout=args.dropout,
                               dropout_prob=args.dropout_prob, root_history_len=10,
                               output_data_format=args.output_data_format, device=device, compute_dtype=dtype_of(args),
                               feat_dim=getattr(train_dataset, 'feat', args.feat_dim), window=window).to(device)
        if not any(p.requires_grad for p in model.parameters()):
            print("No parameters to optimize. Skipping training loop.")
            return False

        cond_cols = getattr(args, 'cond_cols', 0) if diffusion else 0
        cond_drop = float(getattr(args, 'cond_drop', 0.0)) if diffusion else 0.0
        if diffusion:
            check_cond_cols(model_type, cond_cols, feat_dim=model.feat_dim)
            model.cond_cols = cond_cols
            model.cond_drop = cond_drop
            model.prediction = prediction
            train_eval, dev_eval = DiffusionLossEvaluator('train', cond_cols), DiffusionLossEvaluator(DEV, cond_cols)
        else:
            train_eval = RegressionLossEvaluator(dataset=train_dataset, split='train', device=device)
            dev_eval = RegressionLossEvaluator(dataset=dev_dataset, split=DEV, device=device)

        trainer, optimizer, ddp_model = None, None, model
        if args.eager:
            if distributed:
                from torch.nn.parallel import DistributedDataParallel as DDP
                model.ensure_packed()
                ddp_model = DDP(model, device_ids=[device.index], output_device=device.index)
            optimizer = make_torch_optimizer(args.opt_type, model.parameters(), args.learning_rate)
        else:
            # batches per epoch on this rank, as the loop below will find them: the sampler's share (drop_last), whole batches
            # only for the denoisers and from a window cache, cut at --max-steps
            share = len(train_dataset) // world_size
            whole = diffusion or bool(args.window_cache)
            per_epoch = share // args.batch_size if whole else -(-share // args.batch_size)
            lr_schedule = resolve_lr_schedule(args, min(per_epoch, args.max_steps) if args.max_steps else per_epoch)
            if lr_schedule is not None:
                print(f"Learning-rate schedule: {lr_schedule} over a base rate of {args.learning_rate:g}")
            trainer = HipTrainer(model, "diffusion" if diffusion else "regression", args.opt_type, args.learning_rate,
                                 args=args, use_graph=not args.no_graph, bucket_mb=args.bucket_mb,
                                 ema_decay=getattr(args, 'ema_decay', 0.0),
                                 ema_warmup=not getattr(args, 'no_ema_warmup', False), cond_cols=cond_cols,
                                 cond_drop=cond_drop, lr_schedule=lr_schedule,
                                 weight_decay=getattr(args, 'weight_decay', 0.0),
                                 max_grad_norm=getattr(args, 'max_grad_norm', 0.0), loss_weight=loss_weight,
                                 prediction=prediction, velocity_loss=velocity_loss)
            if trainer.velocity_loss is not None:
                print(f"Velocity loss on the predicted x0: {trainer.velocity_loss}; the reports show the term and the velocity "
                      f"error in x0 units beside the optimised loss")
            if trainer.prediction != 'eps':
                print(f"The denoiser predicts {trainer.prediction}; the reports show the eps-MSE its output implies beside the "
                      f"optimised loss, and its mean per band of noise level")
            if trainer.loss_weight is not None:
                print(f"Loss weighting by noise level: {trainer.loss_weight}; the reports show the unweighted eps-MSE beside "
                      f"the optimised loss, and its mean per band of noise level")
            if trainer.clip:
                print(f"Gradient clipping: global L2 norm at most {trainer.max_grad_norm:g}, taken and applied on the device "
                      f"(one optimizer launch over the whole buffer per step)")
            if trainer.weight_decay > 0:
                print(f"Weight decay {trainer.weight_decay:g} (decoupled) on {len(trainer.decayed)} of "
                      f"{len(trainer.layout)} parameter tensors")

        if getattr(args, 'loss_every', 1) < 1:
            raise SystemExit("--loss-every must be >= 1")
        if args.window_cache == 'hbm' and not (diffusion and getattr(args, 'synthetic_windows', 0) > 0):
            raise SystemExit("--window-cache hbm names the device-resident synthetic table: it needs a diffusion model type "
                             "and --synthetic-windows N (a cache FILE takes a path)")
        from ..hip import HipError
        try:
            epoch_checkpoint, _ = self.load_latest_checkpoint(model, optimizer=trainer if trainer is not None else optimizer,
                                                              checkpoint_dir=checkpoint_dir)
        except HipError as exc:
            if "loss weighting" in str(exc):
                raise SystemExit(f"{checkpoint_dir}: {exc}. Resume with the same --loss-weight / --min-snr-gamma or use "
                                 f"another --checkpoint-dir") from None
            if "checkpoint's prediction" in str(exc):
                raise SystemExit(f"{checkpoint_dir}: {exc}. Resume with the same --prediction or use another "
                                 f"--checkpoint-dir") from None
            if "checkpoint's velocity loss" in str(exc):
                raise SystemExit(f"{checkpoint_dir}: {exc}. Resume with the same --velocity-loss / --velocity-gamma or use "
                                 f"another --checkpoint-dir") from None
            if "gradient-norm clip" in str(exc):
                raise SystemExit(f"{checkpoint_dir}: {exc}. Resume with the same --max-grad-norm or use another "
                                 f"--checkpoint-dir") from None
            if "weight decay" in str(exc):
                raise SystemExit(f"{checkpoint_dir}: {exc}. Resume with the same --weight-decay or use another "
                                 f"--checkpoint-dir") from None
            if "learning-rate schedule" not in str(exc):
                raise
            raise SystemExit(f"{checkpoint_dir}: {exc}. Resume with the same --lr-schedule / --lr-warmup-steps / "
                             f"--lr-min-ratio and pass --lr-total-steps explicitly (0 derives it from --epochs and "
                             f"--max-steps, which may have changed), or use another --checkpoint-dir") from None
        if diffusion and model.cond_cols != cond_cols:       # the checkpoint's value: a resumed run keeps training that model
            raise SystemExit(f"the checkpoint in {checkpoint_dir} was trained with --cond-cols {model.cond_cols}, this run "
                             f"asks for {cond_cols}: resume with the same value or use another --checkpoint-dir")
        if diffusion and model.prediction != prediction:
            raise SystemExit(f"the checkpoint in {checkpoint_dir} was trained with --prediction {model.prediction}, this run "
                             f"asks for {prediction}: resume with the same value or use another --checkpoint-dir")
        if diffusion and model.cond_drop != cond_drop:
            raise SystemExit(f"the checkpoint in {checkpoint_dir} was trained with --cond-drop {model.cond_drop}, this run "
                             f"asks for {cond_drop}: resume with the same value or use another --checkpoint-dir")
        # the checkpoint is read before the cache is built: a resumed run hands its statistics to the cache
        standardize = diffusion and getattr(args, 'standardize', False)
        column_stats = model.column_stats if diffusion else None
        if diffusion and (column_stats is not None) != standardize and (epoch_checkpoint >= 0 or not standardize):
            was, now = ("with", "without") if column_stats is not None else ("without", "with")
            raise SystemExit(f"the checkpoint in {checkpoint_dir} was trained {was} --standardize, this run is {now} it: its "
                             f"weights are for the other units; resume with the same choice or use another --checkpoint-dir")
        check_standardize(args, have_stats=column_stats is not None)
        cache = None
        if args.window_cache and trainer is not None:
            from ..data.WindowCache import DeviceMotionCache, DeviceWindowCache, PackedWindows, wait_for_file
            # rank 0 packs and writes (atomically: temporary file + rename); the other ranks POLL for the finished file and
            # only then enter the barrier -- packing a full training set can outlast the process group's collective timeout
            # (~10 min under RCCL), so no collective may span it; none of them can open a file that is still being written
            in_hbm = diffusion and args.window_cache == 'hbm' and getattr(args, 'synthetic_windows', 0) > 0
            # the failure marker carries this launch's id (every rank of a torchrun launch sees the same one): the marker a
            # previous, failed launch left behind has another name and is never mistaken for this run's
            run_id = os.environ.get("TORCHELASTIC_RUN_ID", "none") + "." + os.environ.get("MASTER_PORT", "0")
            failed_marker = f"{args.window_cache}.failed.{run_id}"
            if in_hbm:
                pass                  # synthetic windows are drawn straight into HBM below: no file, no host pass
            elif not os.path.exists(args.window_cache) and rank == 0:
                print(f"Packing {len(train_dataset)} training windows into {args.window_cache} ...")
                try:
                    if diffusion:
                        save_motion_windows(train_dataset, args.window_cache)
                    else:
                        PackedWindows.from_dataset(train_dataset, workers=args.data_loading_workers).save(args.window_cache)
                except BaseException as exc:      # the waiting ranks poll for this instead of sitting out their timeout
                    with open(failed_marker, "w") as f:
                        f.write(repr(exc))
                    raise
            if distributed and not in_hbm:
                wait_for_file(args.window_cache, float(os.environ.get("IB_WINDOW_CACHE_WAIT_S", 6 * 3600)),
                              failed=failed_marker)
                dist.barrier()
            if in_hbm:
                cache = DeviceMotionCache.synthetic(len(train_dataset), window, train_dataset.feat, device,
                                                    model.compute_dtype, seed=0, standardize=standardize,
                                                    stats=column_stats)
            elif diffusion:
                import numpy as np
                cache = DeviceMotionCache(torch.from_numpy(np.load(args.window_cache, mmap_mode='r')), device,
                                          model.compute_dtype, stats=column_stats, standardize=standardize)
            else:
                cache = DeviceWindowCache(PackedWindows.load(args.window_cache), device)
            print(f"[rank={rank}] window cache: {len(cache)} windows, "
                  f"{cache.table.numel() * cache.table.element_size() / 2**20:.1f} MiB in HBM")

        if standardize and model.column_stats is None:       # a new run: the statistics the cache was built with
            model.column_stats = cache.column_stats.cpu()
        if diffusion and getattr(args, 'record_range', False) and model.column_range is None:
            # asked for and not in the checkpoint (a resumed run keeps the checkpoint's record): one pass over the cache
            model.column_range = cache.column_range().cpu()
        from .. import hip
        noise_seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        std = None                                           # (mean, inv) on the device: every raw window goes through them
        if standardize:
            st = model.column_stats.to(device)
            std = (st[:, 0].contiguous(), hip.inv_scale(st[:, 1].contiguous()))

        def standardized(x0, dtype):
            """raw windows x0 [B, T, D] (host or device) -> z = (x0 - mean) * inv on the device in `dtype`: standardised in
            fp32 and rounded once, as the window cache's table is (hip.column_affine)"""
            xf = x0.to(device, torch.float32).contiguous()
            return hip.column_affine(xf, torch.empty(tuple(xf.shape), dtype=dtype, device=device), std[0], std[1],
                                     mode=hip.STANDARDIZE)

        def device_batch(x0, stream_id, draw):
            """x0 [B, T, D] (host or device) -> (x0, t, eps) on the device in the model's dtype; t / eps from the
            counter-based generator (csrc/noise.hip), counter `draw`: the dev-set evaluation and the --eager loop draw like
            the fused trainer does, nothing random is made on the host.  Two counters: the dev set's starts at 0 before
            every epoch (the same noise every time: comparable reports); the --eager training loop's is the global step
            epoch * batches-per-epoch + i, which only ever increases and is right again after a resume -- a window meets
            fresh (t, eps) in every epoch, as with the host generator of the reference-style loop"""
            xd = x0.to(device, model.compute_dtype).contiguous() if std is None else standardized(x0, model.compute_dtype)
            ed = torch.empty_like(xd)
            td = torch.empty(xd.shape[0], dtype=torch.int64, device=device)
            hip.diffusion_draw(noise_seed, step=int(draw), stream_id=stream_id, eps=ed, t=td,
                               num_train_steps=model.num_train_steps)
            return xd, td, ed

        def noise_batch(xd, ed, td, tabs, xt):
            """x_t of the dev-set evaluation and the --eager loop: conditioning columns clean when --cond-cols N > 0.  No
            condition dropout here (--cond-drop is the fused trainer's): the dev loss reported is the conditional one"""
            if cond_cols:
                hip.q_sample_cond(xd, ed, td, tabs.sqrt_ab, tabs.sqrt_1mab, xt, cond_cols)
            else:
                hip.q_sample(xd, ed, td, tabs.sqrt_ab, tabs.sqrt_1mab, xt)

        adopted = False
        prev_stream = None
        for epoch in range(epoch_checkpoint + 1, args.epochs):
            dev_dataloader.sampler.set_epoch(epoch)
            train_dataloader.sampler.set_epoch(epoch)
            print(f'[rank={rank}] Evaluating Dev Set Before Epoch {epoch}')
            with torch.no_grad():
                model.eval()
                for i, batch in enumerate(dev_dataloader):
                    if diffusion:
                        xd, td, ed = device_batch(batch, 0x80000000 | rank, i)   # the same noise before every epoch
                        tabs = model.tables(device)
                        xt = torch.empty_like(xd)
                        noise_batch(xd, ed, td, tabs, xt)
                        out = model(xt, td)
                        if prediction != 'eps':      # the report stays the eps-MSE: the noise prediction the output implies
                            hip.pred_to_eps(xt, out, td, tabs.sqrt_ab, tabs.sqrt_1mab, tabs.inv_sqrt_1mab, prediction)
                        dev_eval(out, ed)
                    else:
                        inputs, labels, subj, trial = batch
                        dev_eval(inputs, model(inputs), labels, subj, trial, args, compute_report=args.compute_report)
                    if (args.max_dev_steps or args.max_steps) and i + 1 >= (args.max_dev_steps or args.max_steps):
                        break
                print(f'[rank={rank}] Dev Set Evaluation: ')
                dev_eval.print_report(args, log_to_wandb=log_to_wandb) if not diffusion else dev_eval.print_report()
            if distributed:
                dist.barrier()
            print(f'[rank={rank}] Running Training Epoch {epoch}')
            model.train()
            if trainer is not None and not adopted:
                prev_stream = trainer.adopt_stream()   # the loop's device work runs on the trainer's stream: no per-step hand-over
                adopted = True
            if cache is not None:
                train_batches = list(cache.batches(args.batch_size, rank=rank, world=world_size))
            else:
                train_batches = train_dataloader
            n_batches = len(train_batches)
            t_epoch, steps_epoch = time.perf_counter(), 0
            for i, batch in enumerate(train_batches):
                steps_epoch += 1
                if cache is not None and diffusion:
                    loss = trainer.step_drawn(cache, batch)           # gather + draw + fused step: all on the device
                    if (i + 1) % args.loss_every == 0:
                        train_eval.losses.append(loss.detach().clone())
                elif cache is not None:
                    trainer.step_windows(cache, batch)
                    train_eval.record_result(trainer.result)
                elif diffusion:
                    if trainer is not None:
                        loss = trainer.step_x0(batch.to(device, non_blocking=True) if std is None
                                               else standardized(batch, torch.float32))
                        train_eval.losses.append(loss.detach().clone())
                    else:
                        optimizer.zero_grad()
                        tabs = model.tables(device)
                        xd, td, ed = device_batch(batch, rank, epoch * n_batches + i)
                        xt = torch.empty_like(xd)
                        noise_batch(xd, ed, td, tabs, xt)
                        loss = train_eval(ddp_model(xt, td), ed)
                        loss.backward()
                        optimizer.step()
                else:
                    inputs, labels, subj, trial = batch
                    if trainer is not None:
                        trainer.step((inputs, labels))
                        train_eval.record_result(trainer.result)
                    else:
                        optimizer.zero_grad()
                        loss = train_eval(inputs, ddp_model(inputs), labels, subj, trial, args,
                                          compute_report=args.compute_report and (i % 100 == 0))
                        loss.backward()
                        optimizer.step()
                last = (i == n_batches - 1) or (args.max_steps and i + 1 >= args.max_steps)
                if (i + 1) % 100 == 0 or last:
                    logging.info(f'  - [rank={rank}] Batch {i + 1}/{n_batches}')
                if (i + 1) % args.report_every == 0 or last:
                    logging.info(f'[rank={rank}] Batch {i} Training Set Evaluation: ')
                    train_eval.print_report(args, reset=False) if not diffusion else train_eval.print_report(reset=False)
                    if trainer is not None and trainer._sched_args():
                        print(f"[rank={rank}] learning rate {trainer.current_lr():.6g} at step {trainer.steps_done + 1}")
                    if trainer is not None and trainer.level_accum is not None:
                        rep = trainer.level_loss(reset=True)        # since the last report line
                        if rep["steps"]:
                            how = trainer.loss_weight if trainer.loss_weight is not None else "unweighted"
                            how = how if trainer.prediction == "eps" else f"{trainer.prediction}-prediction, {how}"
                            print(f"[rank={rank}] optimised loss {rep['weighted']:.6g} ({how}), unweighted "
                                  f"eps-MSE {rep['unweighted']:.6g} over {rep['steps']} steps")
                            print(f"[rank={rank}] eps-MSE per noise-level band: {format_level_report(rep)}")
                            if trainer.velocity_loss is not None:
                                print(f"[rank={rank}] weighted MSE term {rep['mse']:.6g}, velocity term {rep['velocity']:.6g} "
                                      f"({trainer.velocity_loss}), x0 velocity error {rep['x0_velocity']:.6g}")
                                print(f"[rank={rank}] x0 velocity error per noise-level band: "
                                      f"{format_level_report({'bands': rep['x0_velocity_bands']})}")
                    if trainer is not None and trainer.clip:
                        print(f"[rank={rank}] gradient norm {trainer.grad_norm():.6g}, clip coefficient {trainer.clip_coef():.6g}")
                    if rank == 0:
                        save_checkpoint(checkpoint_dir, epoch, i, model, trainer if trainer is not None else optimizer)
                if last:
                    break
            if device.type == 'cuda':
                torch.cuda.synchronize(device)
            dt_epoch = time.perf_counter() - t_epoch
            TrainCommand.last_run_stats = {"epoch": epoch, "steps": steps_epoch, "seconds": dt_epoch,
                                           "windows_per_s": steps_epoch * args.batch_size * world_size / max(dt_epoch, 1e-9)}
            print(f"[rank={rank}] epoch {epoch}: {steps_epoch} steps in {dt_epoch:.3f} s = "
                  f"{self.last_run_stats['windows_per_s']:.0f} windows/s (all ranks, reports and checkpoints included)")
            logging.info('-' * 80)
            logging.info(f'[rank={rank}] Epoch {epoch}/{args.epochs} Training Set Evaluation: ')
            train_eval.print_report(args, log_to_wandb=log_to_wandb) if not diffusion else train_eval.print_report()
            if trainer is not None and trainer._sched_args():
                print(f"[rank={rank}] epoch {epoch}: learning rate {trainer.current_lr():.6g} at step {trainer.steps_done + 1}")
            logging.info('-' * 80)

        if prev_stream is not None:                 # in-process callers (tests, tools) get their stream back
            torch.cuda.current_stream().synchronize()
            torch.cuda.set_stream(prev_stream)
        if wandb is not None:
            wandb.finish()
        if distributed:
            dist.destroy_process_group()
        return True


def save_motion_windows(dataset, path: str, chunk: int = 4096):
    """the [N, T, D] motion windows of a data set as one float32 .npy (written under a temporary name, then renamed)"""
    import numpy as np
    n = len(dataset)
    first = dataset[0]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f"{path}.tmp.{os.getpid()}.npy"
    out = np.lib.format.open_memmap(tmp, mode='w+', dtype=np.float32, shape=(n,) + tuple(first.shape))
    for i in range(n):
        out[i] = dataset[i].to(torch.float32).numpy()
    out.flush()
    del out
    os.replace(tmp, path)


def check_ema_args(args: argparse.Namespace):
    """--ema-decay D: D in [0, 1); the EMA lives in the fused optimizer launches, so --eager (torch.optim) has none"""
    d = getattr(args, 'ema_decay', 0.0)
    if not 0.0 <= d < 1.0:
        raise SystemExit(f"--ema-decay must lie in [0, 1) (0 = off, 0.999-0.9999 are usual), got {d}")
    if d > 0 and getattr(args, 'eager', False):
        raise SystemExit("--ema-decay needs the fused trainer: --eager runs torch.optim, which keeps no EMA of the weights")


def check_weight_decay_args(args: argparse.Namespace):
    """--weight-decay W: finite and >= 0; the decay is applied inside the fused optimizer launches, so --eager (torch.optim
    with only lr set) has none"""
    wd = getattr(args, 'weight_decay', 0.0)
    if not 0.0 <= wd < float('inf'):                    # NaN fails the comparison
        raise SystemExit(f"--weight-decay must be finite and >= 0, got {wd}")
    if wd > 0 and getattr(args, 'eager', False):
        raise SystemExit("--weight-decay needs the fused trainer: --eager runs torch.optim with only the rate set")


def check_max_grad_norm_args(args: argparse.Namespace):
    """--max-grad-norm X: >= 0 and not NaN (0: off, inf: measure only); the norm is taken and applied inside the fused step, so
    --eager (torch.optim with only the rate set) has none"""
    x = getattr(args, 'max_grad_norm', 0.0)
    if not x >= 0.0:                                    # NaN fails the comparison
        raise SystemExit(f"--max-grad-norm must be >= 0 and not NaN, got {x}")
    if x > 0 and getattr(args, 'eager', False):
        raise SystemExit("--max-grad-norm needs the fused trainer: --eager runs torch.optim with only the rate set")


def resolve_loss_weight(args: argparse.Namespace):
    """--loss-weight {off,uniform,min-snr} / --min-snr-gamma G -> a loss_weight.LossWeight, or None for off.  A diffusion model
    type; the weight is applied inside the fused step's loss launch, so --eager (the evaluator's plain eps-MSE) has none"""
    from ..loss_weight import LossWeight, check_gamma
    kind = getattr(args, 'loss_weight', 'off') or 'off'
    if kind == 'off':
        return None
    if not is_diffusion(args.model_type):
        raise SystemExit(f"--loss-weight weights the diffusion loss by noise level: it needs a diffusion model type, got "
                         f"{args.model_type}")
    if getattr(args, 'eager', False):
        raise SystemExit("--loss-weight needs the fused trainer: the weight is applied inside its loss launch, --eager has none")
    if kind == 'uniform':
        return LossWeight('uniform')
    try:
        return LossWeight('min_snr', gamma=check_gamma(getattr(args, 'min_snr_gamma', 5.0)))
    except ValueError as exc:
        raise SystemExit(f"--min-snr-gamma: {exc}") from None


def resolve_prediction(args: argparse.Namespace) -> str:
    """--prediction {eps,x0,v}.  x0 / v need a diffusion model type and the fused trainer: the target is formed inside its loss
    launch, --eager (the evaluator's plain eps-MSE) has none"""
    kind = getattr(args, 'prediction', 'eps') or 'eps'
    if kind == 'eps':
        return kind
    if not is_diffusion(args.model_type):
        raise SystemExit(f"--prediction sets what a diffusion denoiser predicts: it needs a diffusion model type, got "
                         f"{args.model_type}")
    if getattr(args, 'eager', False):
        raise SystemExit("--prediction needs the fused trainer: the target is formed inside its loss launch, --eager has none")
    return kind


def resolve_velocity_loss(args: argparse.Namespace):
    """--velocity-loss LAMBDA / --velocity-gamma G -> a velocity_loss.VelocityLoss, or None for 0 (off).  A diffusion model
    type; the term is computed inside the fused step's loss launch, so --eager (the evaluator's plain eps-MSE) has none"""
    lam = getattr(args, 'velocity_loss', 0.0) or 0.0
    if lam == 0.0:
        return None
    if not is_diffusion(args.model_type):
        raise SystemExit(f"--velocity-loss scores the frame differences of a diffusion denoiser's predicted x0: it needs a "
                         f"diffusion model type, got {args.model_type}")
    if getattr(args, 'eager', False):
        raise SystemExit("--velocity-loss needs the fused trainer: the term is computed inside its loss launch, --eager has none")
    from ..velocity_loss import VelocityLoss
    try:
        return VelocityLoss(lam, gamma=getattr(args, 'velocity_gamma', 5.0))
    except ValueError as exc:
        raise SystemExit(f"--velocity-loss / --velocity-gamma: {exc}") from None


def format_level_report(rep: dict) -> str:
    """one line of the band means of trainer.level_loss(): `t lo-hi mean` per band, `-` where no window fell in it"""
    return "  ".join(f"t {lo}-{hi - 1} {'-' if mean is None else format(mean, '.6g')}" for lo, hi, mean in rep["bands"]
                     if hi > lo)


def check_lr_schedule(args: argparse.Namespace):
    """--lr-schedule / --lr-warmup-steps / --lr-total-steps / --lr-min-ratio: the rate is computed inside the fused optimizer
    launches, so --eager (torch.optim at one rate) has none; what can be refused before the data is opened is refused here"""
    kind, w = getattr(args, 'lr_schedule', 'constant'), getattr(args, 'lr_warmup_steps', 0)
    T, m = getattr(args, 'lr_total_steps', 0), getattr(args, 'lr_min_ratio', 0.0)
    if not 0.0 <= m <= 1.0:
        raise SystemExit(f"--lr-min-ratio must lie in [0, 1], got {m}")
    if w < 0 or T < 0:
        raise SystemExit(f"--lr-warmup-steps and --lr-total-steps must be >= 0, got {w} and {T}")
    if (kind != 'constant' or w > 0) and getattr(args, 'eager', False):
        raise SystemExit("--lr-schedule / --lr-warmup-steps need the fused trainer: --eager runs torch.optim at one rate")
    if kind != 'constant' and T > 0 and T <= w:
        raise SystemExit(f"--lr-schedule {kind} needs --lr-total-steps > --lr-warmup-steps, got {T} and {w}")


def resolve_lr_schedule(args: argparse.Namespace, batches_per_epoch: int):
    """the LrSchedule of the flags, or None for a constant rate without warmup.  --lr-total-steps 0: --epochs x
    batches_per_epoch (this rank's, --max-steps honoured by the caller)"""
    from ..lr_schedule import LrSchedule, active
    check_lr_schedule(args)
    kind, w = getattr(args, 'lr_schedule', 'constant'), getattr(args, 'lr_warmup_steps', 0)
    T = getattr(args, 'lr_total_steps', 0) or int(args.epochs) * int(batches_per_epoch)
    if kind != 'constant' and T <= w:
        raise SystemExit(f"--lr-schedule {kind} needs more steps in all than --lr-warmup-steps {w}: --epochs x batches per "
                         f"epoch gives {T}; train longer, warm up for fewer steps or pass --lr-total-steps")
    return active(LrSchedule(kind, w, T if kind != 'constant' else 0, getattr(args, 'lr_min_ratio', 0.0)))


def check_cond_cols(model_type: str, cond_cols: int, feat_dim: int = None):
    """--cond-cols N: diffusion model types only, N in 0 .. feat_dim - 1 (feat_dim is known once the data set is open)"""
    if cond_cols and not is_diffusion(model_type):
        raise SystemExit(f"--cond-cols conditions a diffusion denoiser on its first columns: model type '{model_type}' "
                         f"has none (diffusion-mlp / diffusion-transformer do)")
    if cond_cols < 0 or (feat_dim is not None and cond_cols >= feat_dim):
        hi = "feat_dim - 1" if feat_dim is None else str(feat_dim - 1)
        raise SystemExit(f"--cond-cols must lie in 0 .. {hi} (at least one column has to stay free), got {cond_cols}")


def check_cond_drop(args: argparse.Namespace):
    """--cond-drop P: P in [0, 1], with a diffusion model type and --cond-cols N > 0; the drop is decided inside the fused
    trainer's noising launch, so --eager has none"""
    p = getattr(args, 'cond_drop', 0.0)
    if not 0.0 <= p <= 1.0:
        raise SystemExit(f"--cond-drop must lie in [0, 1] (0 = off, 0.1-0.2 are usual), got {p}")
    if p > 0 and not (is_diffusion(args.model_type) and getattr(args, 'cond_cols', 0) > 0):
        raise SystemExit("--cond-drop drops the conditioning columns of a conditional denoiser: it needs a diffusion model "
                         "type and --cond-cols N > 0")
    if p > 0 and getattr(args, 'eager', False):
        raise SystemExit("--cond-drop needs the fused trainer: the drop is decided inside its noising launch, --eager has none")


def check_record_range(args: argparse.Namespace):
    """--record-range: a diffusion model type trained from the device-resident window cache, whose table the range kernel
    reads (--window-cache; the fused trainer: --eager builds no cache)"""
    if not getattr(args, 'record_range', False):
        return
    if not is_diffusion(args.model_type):
        raise SystemExit(f"--record-range records the column ranges of a diffusion denoiser's training windows: model type "
                         f"'{args.model_type}' has none")
    if not getattr(args, 'window_cache', None) or getattr(args, 'eager', False):
        raise SystemExit("--record-range reads the device-resident window cache: it needs --window-cache (`hbm` with "
                         "--synthetic-windows, or a file) and the fused trainer (not --eager)")


def check_standardize(args: argparse.Namespace, have_stats: bool = None):
    """--standardize: a diffusion model type; the statistics come from the checkpoint a run resumes (have_stats; --eager is
    fine then) or, on a new run, from the pass that builds the window cache (--window-cache and the fused trainer).
    have_stats None: before the checkpoint is read, the model type alone is checked"""
    if not getattr(args, 'standardize', False):
        return
    if not is_diffusion(args.model_type):
        raise SystemExit(f"--standardize standardises the windows of a diffusion denoiser: model type '{args.model_type}' "
                         f"has none (the regression models take raw inputs)")
    if have_stats is False and (not getattr(args, 'window_cache', None) or getattr(args, 'eager', False)):
        raise SystemExit("--standardize takes the column statistics from the pass that builds the window cache: a run with no "
                         "checkpoint to take them from needs --window-cache (`hbm` with --synthetic-windows, or a file) and "
                         "the fused trainer (not --eager)")


def make_torch_optimizer(opt_type: str, params, lr: float):
    table = {'adagrad': torch.optim.Adagrad, 'adam': torch.optim.Adam, 'sgd': torch.optim.SGD,
             'rmsprop': torch.optim.RMSprop, 'adadelta': torch.optim.Adadelta, 'adamax': torch.optim.Adamax}
    if opt_type not in table:
        logging.error('Invalid optimizer type: ' + opt_type)
        assert (False)
    return table[opt_type](params, lr=lr)


def save_checkpoint(checkpoint_dir: str, epoch: int, batch: int, model, opt):
    """file grammar of train.py:271-278; keys are saved WITHOUT DDP's `module.` prefix.  A trainer with an EMA adds
    'ema_state_dict' (the model's state dict over the EMA weights) and 'ema' ({'decay', 'warmup'}); without one the file
    holds the three reference keys only.  A denoiser trained with --cond-cols N > 0 adds 'cond_cols': N, one trained with
    --cond-drop P > 0 'cond_drop': P, one trained with --prediction x0 / v 'prediction': the kind, one trained with
    --record-range 'column_range': fp32 [feat_dim, 2], one trained with --standardize 'column_stats': fp32 [feat_dim, 2] =
    per column (mean, scale).  With both, column_range is taken over the standardised table: it is in the units the sampler
    works in, the units of the x0 clip's bounds."""
    os.makedirs(checkpoint_dir, exist_ok=True)
    path = f"{checkpoint_dir}/epoch_{epoch}_batch_{batch}.pt"
    osd = opt.optimizer_state_dict() if hasattr(opt, 'optimizer_state_dict') else opt.state_dict()
    ckpt = {'epoch': epoch,
            'model_state_dict': {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
            'optimizer_state_dict': osd}
    if getattr(model, 'cond_cols', 0):
        ckpt['cond_cols'] = int(model.cond_cols)
    if getattr(model, 'cond_drop', 0.0) > 0:
        ckpt['cond_drop'] = float(model.cond_drop)
    if getattr(model, 'prediction', 'eps') != 'eps':
        ckpt['prediction'] = str(model.prediction)
    if getattr(model, 'column_range', None) is not None:
        ckpt['column_range'] = torch.as_tensor(model.column_range, dtype=torch.float32).detach().cpu().clone()
    if getattr(model, 'column_stats', None) is not None:
        ckpt['column_stats'] = torch.as_tensor(model.column_stats, dtype=torch.float32).detach().cpu().clone()
    if getattr(opt, 'ema', None) is not None:
        ckpt['ema_state_dict'] = opt.ema_state_dict()
        ckpt['ema'] = {'decay': opt.ema_decay, 'warmup': opt.ema_warmup}
    torch.save(ckpt, path)
    return path
