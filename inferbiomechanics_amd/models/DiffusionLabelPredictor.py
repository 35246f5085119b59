"""[BUILD-DEFINED] Ground-contact labels inferred from observed motion with a trained diffusion denoiser.

A window is the denoiser's ``[F, D]`` matrix (``MotionWindowView.matrix``): the frame's model-input channels, then the
30 label channels cop | force | torque | wrench (``LOSS_KEY_ORDER``, widths 6 / 6 / 6 / 12).  The input columns of
every frame are observed, the label columns are free, and the masked DDIM loop (``ConditionalDDIMSampler``) fills them
in.  The result is the reference regression models' outputs dict, so the same ``RegressionLossEvaluator``, CSV rows and
report apply.  With ``eta > 0`` the loop is stochastic and with ``num_samples = K > 1`` every window is sampled K times:
the outputs are then the ensemble mean and ``last_std`` the per-element spread (``ib_ensemble_stats``)."""
from typing import Dict, Optional

import torch

from .. import hip
from ..data.AddBiomechanicsDataset import INPUT_KEY_ORDER, LOSS_KEY_ORDER, LOSS_KEY_WIDTHS, MotionWindowView
from ..diffusion.ensemble import interval_levels
from ..diffusion.sampler import ConditionalDDIMSampler, StitchedDDIMSampler, StochasticStitchedSampler, X0Clip

LABEL_WIDTH = sum(LOSS_KEY_WIDTHS)          # 30: the label block at the end of every frame's row


def label_mask(frames: int, feat: int) -> torch.Tensor:
    """[F, D] bool: True on the observed input columns, False on the last 30 (label) columns"""
    if feat <= LABEL_WIDTH:
        raise ValueError(f"a window row of {feat} columns has no room for the {LABEL_WIDTH} label columns")
    m = torch.ones(frames, feat, dtype=torch.bool)
    m[:, feat - LABEL_WIDTH:] = False
    return m


class DiffusionLabelPredictor:
    """``predictor(inputs) -> outputs``: inputs is the reference's batched input dict ``{key: [B, F, c]}``; outputs holds
    the four ``LOSS_KEY_ORDER`` keys as fp32 ``[B, F, C]``.  Window b of a call draws its start noise z from
    (seed, draw + b), so a window's result does not depend on how windows are batched into calls.  With num_samples = K,
    window i = draw + b is replicated K times inside the sampler batch (B K rows); member k has window id i K + k for both its
    start draw and its step noise (eta > 0), the outputs are the members' mean and ``last_std`` their unbiased standard
    deviation, in the same four-key layout (None on the default eta = 0, K = 1 path, which is the single deterministic
    trajectory).  solver / spacing choose the sampler's update and grid (diffusion/sampler.py); 'dpmpp2m_sde' is the
    second-order solver that takes eta > 0 and ensembles.  A denoiser trained on
    clean conditioning columns (model.cond_cols > 0, `train --cond-cols`; it must be feat_dim - 30) gets its observations
    pinned clean at every step (ConditionalDDIMSampler, observations = 'clean'); at 0 they are forward-noised as before.
    guidance = S != 0 is classifier-free guidance of strength S in every sampler the predictor builds (windows, trials,
    ensembles): the noise prediction becomes eps_c + S (eps_c - eps_u).  It needs a denoiser trained with `train --cond-drop`
    (model.cond_drop > 0, read when the predictor is built) on clean conditioning columns.
    resample = (jump, times) is RePaint resampling of the masked loop (diffusion/sampler.py; eta = 0 and solver 'ddim' only):
    every call then takes the id path, member ids from ``member_ids`` also at K = 1 -- they key the re-noise draws, so a
    window's labels do not depend on batching --, and num_samples = K > 1 gives an ensemble at eta = 0 (mean and
    ``last_std``).  What it does to label accuracy on trained checkpoints is unmeasured.
    interval = L (0 < L < 1, needs num_samples >= 2) adds the order statistics of the ensemble, one ``hip.ensemble_order``
    launch over the 30 label columns after ``ib_ensemble_stats``: ``last_interval`` = {'lo', 'median', 'hi'}, each in the
    four-key layout of ``last_std`` -- the Weibull (type 6) quantiles at (1 - L) / 2, 0.5, (1 + L) / 2
    (diffusion/ensemble.py) -- and, for a call that is given labels, ``last_crps`` (fair ensemble CRPS per element),
    ``last_rank`` (members below the label, 0 .. K) and ``last_inside`` (label inside [lo, hi]), the last two uint8.  The
    outputs and ``last_std`` do not change by a bit.  With the default None nothing is launched and all four stay None.
    x0_clip = X0Clip(lo, hi, mode, quantile) (diffusion/sampler.py) keeps the x0 every step predicts inside per-column
    bounds in every sampler the predictor builds; the bounds are given for the 30 label columns (they are then infinite on
    the columns in front of them) or for all feat_dim columns -- the observed columns are skipped by the mask anyway.  What
    it does to label accuracy on trained checkpoints is unmeasured.
    A denoiser trained on standardised windows (model.column_stats = fp32 [D, 2] per column (mean, scale), `train
    --standardize`; read per call, like cond_cols) is sampled in its own units: the observation matrix goes to the model's
    device and is standardised over all D columns by one ``ib_column_affine`` launch, the sampler's result (compute dtype)
    is de-standardised by one more into an fp32 [B K, F, D] tensor -- bf16 would quantise an offset column again -- and
    everything behind that (the label split, ``ib_ensemble_stats``, ``ib_ensemble_order`` against raw labels) runs on it
    unchanged, in raw units.  The bounds of x0_clip are then in the sampler's units, z = (x - mean) / scale: the units of
    the checkpoint's column_range when `train --record-range --standardize` recorded it.  The null condition of a guided
    step (zeros) is then the column mean."""

    def __init__(self, model, num_sample_steps: int = 100, seed: int = 0, output_data_format: str = 'all_frames',
                 use_graph: bool = True, eta: float = 0.0, num_samples: int = 1, solver: str = 'ddim',
                 spacing: str = 'time', guidance: float = 0.0, resample=None, interval: Optional[float] = None,
                 x0_clip: Optional[X0Clip] = None):
        if output_data_format != 'all_frames':
            raise ValueError("DiffusionLabelPredictor: the diffusion models need --output-data-format all_frames")
        if not 0.0 <= float(eta) <= 1.0:
            raise ValueError(f"DiffusionLabelPredictor: eta must be in [0, 1], got {eta}")
        if int(num_samples) != num_samples or num_samples < 1:
            raise ValueError(f"DiffusionLabelPredictor: num_samples must be an integer >= 1, got {num_samples}")
        if interval is not None:
            interval_levels(interval)                                  # ValueError unless 0 < L < 1
            if num_samples < 2:
                raise ValueError(f"DiffusionLabelPredictor: interval = {interval} is made of the order statistics of an "
                                 f"ensemble, it needs num_samples >= 2 (got {num_samples})")
        self.interval = None if interval is None else float(interval)
        self.last_interval: Optional[Dict[str, Dict[str, torch.Tensor]]] = None
        self.last_crps: Optional[Dict[str, torch.Tensor]] = None
        self.last_rank: Optional[Dict[str, torch.Tensor]] = None
        self.last_inside: Optional[Dict[str, torch.Tensor]] = None
        self.model, self.seed = model, int(seed)
        self.eta, self.num_samples = float(eta), int(num_samples)
        self.last_std: Optional[Dict[str, torch.Tensor]] = None
        self.guidance = float(guidance)
        self.x0_clip = self._wide_clip(x0_clip, int(getattr(model, 'feat_dim', 0)))
        # `observations` is set again by every call (_checks); a guided sampler is built for the only kind it takes
        self.sampler = ConditionalDDIMSampler(model, num_sample_steps, use_graph=use_graph, eta=self.eta, seed=self.seed,
                                              solver=solver, spacing=spacing, guidance=self.guidance,
                                              observations='clean' if self.guidance != 0.0 else 'noised', resample=resample,
                                              x0_clip=self.x0_clip)
        self.resample = self.sampler._resampling()       # (jump, times), or None for the plain loop
        self._mask = None                    # label_mask of the last (F, D): one tensor, so the sampler checks it once
        self._trial = None                   # ((hop, blend), StitchedDDIMSampler, mask_cols) of the last predict_trial
        self._trial_ens = None               # the same of the last predict_trial_ensemble, a StochasticStitchedSampler
        self._stats = None                   # (model.column_stats it was made from, mean, scale, inv on the model's device)

    @staticmethod
    def _wide_clip(x0_clip: Optional[X0Clip], feat: int) -> Optional[X0Clip]:
        """the clip over all `feat` columns: bounds given for the 30 label columns get -inf / +inf in front of them"""
        if x0_clip is None:
            return None
        if not isinstance(x0_clip, X0Clip):
            raise ValueError(f"DiffusionLabelPredictor: x0_clip must be None or an X0Clip, got {type(x0_clip).__name__}")
        n = len(x0_clip.lo)
        if n == feat:
            return x0_clip
        if n != LABEL_WIDTH or feat <= LABEL_WIDTH:
            raise ValueError(f"DiffusionLabelPredictor: x0_clip holds bounds for {n} columns; give them for the {LABEL_WIDTH} "
                             f"label columns or for all feat_dim = {feat}")
        pad = feat - LABEL_WIDTH
        return X0Clip((float('-inf'),) * pad + x0_clip.lo, (float('inf'),) * pad + x0_clip.hi, x0_clip.mode, x0_clip.quantile)

    def _label_mask(self, frames: int, feat: int) -> torch.Tensor:
        if self._mask is None or tuple(self._mask.shape) != (frames, feat):
            self._mask = label_mask(frames, feat)
        return self._mask

    def member_ids(self, draw: int, batch: int):
        """window ids of the sampler rows of a call: member k of window i = draw + b is i K + k"""
        K = self.num_samples
        return [(draw + b) * K + k for b in range(batch) for k in range(K)]

    @staticmethod
    def window_matrix(inputs: Dict[str, torch.Tensor]) -> torch.Tensor:
        """[B, F, D] fp32: MotionWindowView.matrix of the batch with the label columns zeroed"""
        ref = inputs[INPUT_KEY_ORDER[0]]
        B, F = ref.shape[0], ref.shape[1]
        zeros = {k: torch.zeros(B, F, w, dtype=torch.float32, device=ref.device) for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS)}
        return MotionWindowView.matrix(inputs, zeros)

    @staticmethod
    def split_labels(x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """[B, F, D] window matrices -> {cop, force, torque, wrench: fp32 [B, F, C]} from the last 30 columns"""
        out, c = {}, x.shape[-1] - LABEL_WIDTH
        for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
            out[k] = x[:, :, c:c + w].to(torch.float32).contiguous()
            c += w
        return out

    def _checks(self, inputs: Dict[str, torch.Tensor], what: str):
        """the checks of a batch of windows (`what` = 'window': F must be the denoiser's window) or of trials ('trial': F at
        least that) -> (obs [B, F, D], the kind of observation table the denoiser was trained for)"""
        obs = self.window_matrix(inputs)
        B, F, D = obs.shape
        T = int(getattr(self.model, 'window', F))
        if D != self.model.feat_dim:
            raise ValueError(f"a {what} row has {D} columns but the denoiser was built for feat_dim = {self.model.feat_dim}")
        if what == 'window' and F != T:
            raise ValueError(f"a window has {F} frames but the denoiser was built for window = {T}")
        if F < T:
            raise ValueError(f"a trial of {F} frames is shorter than the denoiser's window of {T} frames")
        C = int(getattr(self.model, 'cond_cols', 0))
        if C and C != D - LABEL_WIDTH:
            raise ValueError(f"the denoiser was trained with cond_cols = {C}; label inference observes the {D - LABEL_WIDTH} "
                             f"input columns of a {D}-column row, so it needs cond_cols = {D - LABEL_WIDTH} (or 0)")
        return obs, 'clean' if C else 'noised'      # read per call: a checkpoint may be loaded after __init__

    @staticmethod
    def _split_block(x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """[B, F, 30] (any dtype) -> the four-key layout, dtype kept"""
        out, c = {}, 0
        for k, w in zip(LOSS_KEY_ORDER, LOSS_KEY_WIDTHS):
            out[k] = x[:, :, c:c + w].contiguous()
            c += w
        return out

    def _order(self, x: torch.Tensor, labels: Optional[Dict[str, torch.Tensor]]):
        """the order statistics of the members x [B, K, F, D] over the label columns (one launch) -> last_interval and, with
        labels, last_crps / last_rank / last_inside"""
        B, K, F, D = x.shape
        truth = None
        if labels is not None:
            truth = torch.cat([labels[k].to(device=x.device, dtype=torch.float32) for k in LOSS_KEY_ORDER], dim=2).contiguous()
            if tuple(truth.shape) != (B, F, LABEL_WIDTH):
                raise ValueError(f"DiffusionLabelPredictor: the labels make a block of {tuple(truth.shape)}, the ensemble's "
                                 f"label block is {(B, F, LABEL_WIDTH)}")
        res = hip.ensemble_order(x, (D - LABEL_WIDTH, LABEL_WIDTH), self.interval, truth)
        self.last_interval = {k: self._split_block(res[k]) for k in ('lo', 'median', 'hi')}
        if truth is not None:
            self.last_crps, self.last_rank, self.last_inside = (self._split_block(res[k]) for k in ('crps', 'rank', 'inside'))

    def _column_stats(self):
        """(mean, scale, inv) fp32 [D] on the model's device, or None: model.column_stats, read per call"""
        stats = getattr(self.model, 'column_stats', None)
        if stats is None:
            return None
        if self._stats is None or self._stats[0] is not stats:
            self.model.ensure_packed()
            dev = self.model._flat.device
            st = torch.as_tensor(stats, dtype=torch.float32)
            if tuple(st.shape) != (self.model.feat_dim, 2):
                raise ValueError(f"DiffusionLabelPredictor: model.column_stats must be fp32 [feat_dim, 2] = "
                                 f"[{self.model.feat_dim}, 2] (mean, scale), got {tuple(st.shape)}")
            mean, scale = (st[:, j].contiguous().to(dev) for j in (0, 1))
            self._stats = (stats, mean, scale, hip.inv_scale(scale))
        return self._stats[1:]

    def _sample(self, sampler, obs: torch.Tensor, mask: torch.Tensor, draw: int, ids_name: Optional[str], labels=None):
        """_sample_units in the denoiser's units: with model.column_stats, obs is standardised on the way in and the
        sampler's result de-standardised into fp32 on the way out (one launch each); without, nothing is launched"""
        stats = self._column_stats()
        if stats is None:
            return self._sample_units(sampler, obs, mask, draw, ids_name, labels, lambda x: x)
        mean, scale, inv = stats
        raw = obs.to(device=mean.device, dtype=torch.float32).contiguous()
        obs = hip.column_affine(raw, torch.empty_like(raw), mean, inv, mode=hip.STANDARDIZE)

        def to_raw(x):
            out = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
            return hip.column_affine(x.contiguous(), out, mean, scale, mode=hip.DESTANDARDIZE)
        return self._sample_units(sampler, obs, mask, draw, ids_name, labels, to_raw)

    def _sample_units(self, sampler, obs: torch.Tensor, mask: torch.Tensor, draw: int, ids_name: Optional[str], labels,
                      to_raw):
        """the labels of obs [B, F, D] from `sampler`, a masked one.  ids_name None: row b starts from the draw
        (seed, draw + b) and follows its one deterministic trajectory.  Otherwise it is the id keyword of the sampler's
        sample(): every row is replicated K times, the member ids (member_ids) key both the start draws and the step noise,
        and the result is the members' mean, with their standard deviation in last_std (ib_ensemble_stats)."""
        B, F, D = obs.shape
        K = self.num_samples
        self.last_interval = self.last_crps = self.last_rank = self.last_inside = None
        if ids_name is None:
            z = torch.cat([sampler.draw_start(1, F, D, self.seed, draw + b) for b in range(B)])
            return self.split_labels(to_raw(sampler.sample(z, obs, mask)))
        ids = self.member_ids(draw, B)
        z = torch.cat([sampler.draw_start(1, F, D, self.seed, i) for i in ids])
        members = obs.unsqueeze(1).expand(B, K, F, D).reshape(B * K, F, D)
        x = to_raw(sampler.sample(z, members, mask, **{ids_name: ids}))
        mean, std = hip.ensemble_stats(x.view(B, K, F, D))
        self.last_std = self.split_labels(std)
        if self.interval is not None:
            self._order(x.view(B, K, F, D), labels)
        return self.split_labels(mean)

    @staticmethod
    def _kept(kept, key, make):
        """`kept` = (key, trial sampler, mask_cols) if it is the one for key = (hop, blend, D), else a new one.  One sampler
        is kept per kind, with one layout and one captured step: another hop, blend or trial length replaces them, so a
        service fed trials of many lengths holds the tables and the graph of the last one only"""
        if kept is not None and kept[0] == key:
            return kept
        return key, make(), label_mask(1, key[2])[0].contiguous()

    @torch.no_grad()
    def __call__(self, inputs: Dict[str, torch.Tensor], labels: Optional[Dict[str, torch.Tensor]] = None,
                 draw: int = 0) -> Dict[str, torch.Tensor]:
        F = inputs[INPUT_KEY_ORDER[0]].shape[1]
        if labels is not None:
            for k in LOSS_KEY_ORDER:
                if labels[k].shape[1] != F:
                    raise ValueError("DiffusionLabelPredictor: labels must be 'all_frames' (one row per input frame)")
        obs, self.sampler.observations = self._checks(inputs, 'window')
        single = self.num_samples == 1 and self.eta == 0.0 and self.resample is None
        return self._sample(self.sampler, obs, self._label_mask(F, obs.shape[2]), draw, None if single else 'window_ids', labels)

    @torch.no_grad()
    def predict_trial(self, inputs: Dict[str, torch.Tensor], hop: Optional[int] = None, blend: str = 'ramp',
                      draw: int = 0) -> Dict[str, torch.Tensor]:
        """Labels of whole trials: inputs is ``{key: [N, F, c]}`` with F >= model.window consecutive frames (at the
        dataset's frame stride); the trial is denoised as overlapping windows stitched into one sequence
        (``StitchedDDIMSampler``: a window every ``hop`` frames, default window // 2, blended by ``blend``), so every frame
        gets one answer and there are no seams.  Returns the four ``LOSS_KEY_ORDER`` outputs as fp32 ``[N, F, C]``.  Trial b
        draws its start noise from (seed, draw + b).  Deterministic: needs eta = 0 and num_samples = 1."""
        if self.resample is not None:
            raise ValueError(f"predict_trial: resample = {self.resample} needs trial ids for its re-noise draws and the "
                             f"deterministic stitched sampler takes none: use predict_trial_ensemble, which runs it at eta = 0")
        if self.eta != 0.0 or self.num_samples != 1:
            raise ValueError(f"predict_trial: stitched sampling is deterministic, it needs eta = 0 and num_samples = 1 (got "
                             f"eta = {self.eta}, num_samples = {self.num_samples})")
        obs, kind = self._checks(inputs, 'trial')
        s = self.sampler
        self._trial = self._kept(self._trial, (hop, blend, obs.shape[2]), lambda: StitchedDDIMSampler(
            self.model, s.S, hop=hop, blend=blend, use_graph=s.use_graph, solver=s.solver, spacing=s.spacing, seed=self.seed,
            observations=s.observations, guidance=self.guidance, x0_clip=self.x0_clip))
        _, sampler, mask_cols = self._trial
        sampler.observations = kind
        return self._sample(sampler, obs, mask_cols, draw, None)

    @torch.no_grad()
    def predict_trial_ensemble(self, inputs: Dict[str, torch.Tensor], hop: Optional[int] = None, blend: str = 'ramp',
                               draw: int = 0, labels: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """Posterior ensembles of whole trials: as ``predict_trial`` with the predictor's own ``eta`` and ``num_samples`` = K
        (``StochasticStitchedSampler``, solver 'ddim' or 'dpmpp2m_sde').  Trial i = draw + b is replicated K times inside the sampler batch;
        member k has trial id i K + k for both its start draw and its step noise.  Returns the members' mean as the four
        ``LOSS_KEY_ORDER`` outputs, fp32 ``[N, F, C]``, and sets ``last_std`` to their unbiased standard deviation in the
        same layout (0 for K = 1), summed in member order (``ib_ensemble_stats``).  labels ({key: [N, F, c]}, optional) are
        scored when the predictor has an ``interval`` (``last_crps``, ``last_rank``, ``last_inside``)."""
        if self.sampler.solver not in ('ddim', 'dpmpp2m_sde'):
            raise ValueError(f"predict_trial_ensemble: the stochastic stitched loop is DDIM / DDPM or 'dpmpp2m_sde', solver "
                             f"{self.sampler.solver!r} is deterministic")
        obs, kind = self._checks(inputs, 'trial')
        s = self.sampler
        self._trial_ens = self._kept(self._trial_ens, (hop, blend, obs.shape[2]), lambda: StochasticStitchedSampler(
            self.model, s.S, eta=self.eta, hop=hop, blend=blend, use_graph=s.use_graph, spacing=s.spacing, seed=self.seed,
            solver=s.solver, observations=s.observations, guidance=self.guidance, resample=self.resample,
            x0_clip=self.x0_clip))
        _, sampler, mask_cols = self._trial_ens
        sampler.observations = kind
        return self._sample(sampler, obs, mask_cols, draw, 'trial_ids', labels)
