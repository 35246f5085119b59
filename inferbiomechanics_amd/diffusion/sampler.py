"""[BUILD-DEFINED] DDIM / DDPM sampling loop: N denoiser evaluations + updates; eta = 0 is the
deterministic DDIM loop, eta in (0, 1] adds the noise term sigma z' (eta = 1 with as many sampling steps as training steps:
DDPM ancestral sampling), drawn inside the update kernel from a counter-based generator keyed by (seed, window id, step).
solver = 'dpmpp2m' swaps the first-order DDIM update for DPM-Solver++(2M), a second-order multistep update with the same work
per step (one denoiser evaluation and one update launch; it keeps the previous step's data prediction in an fp32 buffer), and
spacing = 'logsnr' runs either solver on a grid uniform in log-SNR instead of in t (schedule.sample_timesteps) -- the pair
that needs far fewer steps for the same accuracy (docs/EXPERIMENTS.md).  solver = 'dpmpp2m_sde' is that solver's stochastic form
(SDE-DPM-Solver++(2M)) for eta in (0, 1]: the same work per step, the step noise drawn inside the update kernel as in the
first-order eta > 0 loop (ib_sde_dpmpp_step, csrc/sde.hip); at eta = 0 it runs the 'dpmpp2m' launches.  It belongs with
spacing = 'logsnr'.

One denoise step = {time-embedding gather, denoiser forward plan, DDIM update, counter++}.  The step index
lives in DEVICE memory (an int32 counter the update kernel reads), and the update kernel also writes the next
step's timestep vector, so ONE captured hipGraph of a single step can be replayed for every step of the loop
with no host involvement between steps (BASELINE config 5).

How the four classes share one loop.  The public sample() of a class checks its arguments and states the call as one frozen
record, SampleCall: the window batch's shape, how it splits into trials, the ids, the observation cut into windows with its
[T, D] mask (or none), the trial layout (or none).  The record is passed down as an argument; nothing about a call is kept
on the sampler, so a call that is refused leaves it as it was.  DDIMSampler owns everything below sample(): the signature
and the buffers of the captured step (_prepare), the masked start state (_start_masked), the loop, and the ONE choice of
the update launch (_launch_update):

    layout   solver order   eta > 0   entry point (with observations)
    no       1              no        ib_ddim_step            (ib_ddim_cond_step)
    no       1              yes       ib_ddim_step_noise      (ib_ddim_cond_step_noise)
    no       2              no        ib_dpmpp_step           (ib_dpmpp_cond_step)
    no       2              yes       ib_sde_dpmpp_step over [B, 1, T, ld] with the one-window layout (masked operands or none)
    yes      1              no        ib_stitch_ddim_step                    "
    yes      1              yes       ib_stitch_ddim_step_noise              "
    yes      2              no        ib_stitch_dpmpp_step                   "
    yes      2              yes       ib_sde_dpmpp_step                      "

(order 2 with eta > 0 is 'dpmpp2m_sde'; 'dpmpp2m_sde' at eta = 0 is an eta = 0 row).

Classifier-free guidance (guidance = s != 0; the three masked classes, observations = 'clean', a denoiser trained with
`train --cond-drop`) changes none of those rows: it is a seam around them, in _prepare and _step_launches alone.  The state
and the noise buffer hold 2B windows, the B of the call and their twins under the null condition (all-zero conditioning
columns, never written after allocation).  One step = {forward over the 2B windows, ib_cfg_combine: the first half of the
noise buffer becomes eps_c + s (eps_c - eps_u), the row's update launch over the first half exactly as without guidance,
ib_cfg_mirror: the free columns and the timesteps of the first half copied to the second, counter++} (csrc/cfg.hip).  At
guidance = 0 none of it exists: the launches, buffers, signature and bits are the unguided loop's.

RePaint resampling (resample = (jump, times); ConditionalDDIMSampler and, by keyword, StochasticStitchedSampler; eta = 0 and
solver 'ddim'; Lugmayr et al. 2022) changes no step either.  The masked loop of an unconditional denoiser is the replacement
method, and it is biased: the free elements are denoised as if the pinned ones had been generated with them.  The loop
therefore walks schedule.resample_walk instead of 0 .. S-1: a 'step' is the step above, the captured graph replayed
unchanged; a 'jump' diffuses the state back `jump` levels (ib_resample_renoise, csrc/resample.hip: fresh noise keyed by
(seed, id, visit) at the free elements, the observed ones pinned to their level) and takes the device counter back with it,
two launches on the sampler's stream between replays (_jump_launches; a guided loop mirrors after it).  What a jump reads --
the jump table, the ids, the one-window layout -- is passed at every call and is no part of the captured step or its
signature, so the setting may change between calls on one capture.  Off (None, or times = 1) nothing of it exists.  One
exception to "changes no step": a resampled loop over ONE-WINDOW trials (F == T) updates with the per-window entry
(ib_ddim_cond_step; _one_window_step), which makes it ConditionalDDIMSampler(resample=...) bit for bit at every row pitch;
that choice is part of the signature, so there the step is captured again when the setting goes on or off.

The x0 clip (x0_clip = X0Clip(lo, hi, mode, quantile); all four classes) changes none of those rows either: like guidance it
is a seam around them, one launch in _step_launches between the denoiser's forward and the row's update launch (in the
guided step after ib_cfg_combine, over the first half), and nowhere else.  Every step reconstructs the data prediction
x0 = (x_t - sigma_t eps) / alpha_t; the launch keeps it inside per-column bounds -- 'range': clamped to [lo_c, hi_c]
(ib_x0_clip_range); 'dynamic': dynamic thresholding (Saharia et al. 2022) in per-column units, the `quantile` of |u|,
u = (x0 - centre_c) / half_width_c, taken over the free bounded elements of ONE [T, ld] window (ib_x0_clip_dynamic) -- and
rewrites eps to the prediction that reconstructs the clipped x0, nothing else, so every update row, eta, observations,
layouts, resampling and the second-order solvers' history follow by themselves.  In the stitched samplers a window is each
overlapping window on its own, before the update kernel blends the predictions.  Observed elements (the mask), columns
without finite bounds hi > lo and pad columns are never counted and never changed.  With None no buffer, launch or
signature entry exists: the loop is the unclipped one bit for bit and launch for launch.  What the clip does to label
accuracy on trained checkpoints is unmeasured.

What the model predicts (model.prediction: 'eps', 'x0' or 'v'; prediction.py, `train --prediction`; all four classes) is one
more seam of the same kind: every row above takes a noise prediction, so for an x0 / v model one launch (ib_pred_to_eps,
csrc/predict.hip) directly after the forward -- in the guided step after ib_cfg_combine, over the first half: the conversion
is affine in the output with the same x_t on the free columns and the guidance weights sum to 1, so the two commute up to
rounding -- rewrites the output into the noise prediction it implies at the windows' levels t_vec, before the clip and the
update.  Solvers, eta, stitching, resampling, the clip and standardisation follow unchanged.  The kind is part of the
signature.  For 'eps' no launch, table or signature entry exists.  What x0 / v prediction does to label accuracy on trained
checkpoints is unmeasured."""
from dataclasses import dataclass
from typing import Optional, Sequence, Union

import torch

from .. import hip
from ..plans import ParamSource
from ..prediction import check_kind
from .schedule import (CLIP_MODES, OBSERVATIONS, check_resample, check_sampler_settings, clip_rank, clip_tables,
                       resample_walk, stitch_layout)


@dataclass(frozen=True)
class X0Clip:
    """The x0 clip of a sampling loop (the module docstring): bounds lo[D] <= hi[D] per column of the window row (-inf /
    +inf: no bound; a column with lo == hi is not bounded either), mode 'range' or 'dynamic', and the quantile in (0, 1] of
    'dynamic' (nearest rank over one window's free bounded elements, schedule.clip_rank; unused by 'range').  Frozen and
    hashable: the bounds are kept as tuples of floats."""
    lo: tuple
    hi: tuple
    mode: str = "range"
    quantile: float = 0.995

    def __post_init__(self):
        lo = tuple(float(v) for v in torch.as_tensor(self.lo, dtype=torch.float64).reshape(-1).tolist())
        hi = tuple(float(v) for v in torch.as_tensor(self.hi, dtype=torch.float64).reshape(-1).tolist())
        clip_tables(lo, hi)                                            # the refusals of the bounds
        if self.mode not in CLIP_MODES:
            raise ValueError(f"X0Clip: mode must be one of {CLIP_MODES}, got {self.mode!r}")
        if not 0.0 < float(self.quantile) <= 1.0:
            raise ValueError(f"X0Clip: quantile must be in (0, 1], got {self.quantile}")
        object.__setattr__(self, "lo", lo)
        object.__setattr__(self, "hi", hi)
        object.__setattr__(self, "quantile", float(self.quantile))


@dataclass(frozen=True)
class SampleCall:
    """One sample() call: B windows of [T, D] (state rows pitched to Dp) that are N trials of W windows each -- a
    per-window loop is N = B, W = 1.  ids: the noise ids as given (None: 0 .. N-1), one per trial.  observed [B, T, D] and
    mask [T, D] (True / non-zero: observed) come together or not at all; lay: the trial layout's tables, None for a
    per-window loop."""
    B: int
    T: int
    D: int
    Dp: int
    N: int
    W: int
    ids: Union[None, Sequence[int], torch.Tensor] = None
    observed: Optional[torch.Tensor] = None
    mask: Optional[torch.Tensor] = None
    lay: Optional[dict] = None


def _checked_ids(given, count: int, noun: str) -> torch.Tensor:
    """the call's `noun` ids (default 0 .. count-1) as the int64 host tensor the device buffer 'win' is filled from"""
    ids = torch.arange(count, dtype=torch.int64) if given is None else \
        torch.as_tensor(given, dtype=torch.int64).reshape(-1).cpu()
    if ids.numel() != count:
        raise ValueError(f"{noun}_ids must hold one id per {noun} ({count}), got {ids.numel()}")
    if count and (int(ids.min()) < 0 or int(ids.max()) >= 1 << 32):
        raise ValueError(f"{noun}_ids must be in 0 .. 2^32 - 1 (one word of the generator's counter)")
    return ids


def _cut(lay: dict, trial: torch.Tensor) -> torch.Tensor:
    """[N, F, D] -> [N * W, T, D]: every window's frames (plumbing: an index, no arithmetic)"""
    N, F, D = trial.shape
    gather = lay["gather"].to(trial.device)
    return trial[:, gather].reshape(N * lay["W"], gather.shape[1], D)


def _join(lay: dict, windows: torch.Tensor, N: int) -> torch.Tensor:
    """[N * W, T, D] -> [N, F, D] from each frame's first copy"""
    w = windows.view(N, lay["W"], windows.shape[1], windows.shape[2])
    return w[:, lay["w0"].to(w.device), lay["t0"].to(w.device)].contiguous()


class DDIMSampler:
    def __init__(self, model, num_sample_steps: int = 100, use_graph: bool = True, eta: float = 0.0,
                 seed: Optional[int] = None, solver: str = "ddim", spacing: str = "time",
                 x0_clip: Optional[X0Clip] = None):
        """eta in [0, 1]; seed (default: torch's initial seed) keys the step noise of an eta > 0 loop; solver 'ddim',
        'dpmpp2m' (deterministic: eta = 0 only) or 'dpmpp2m_sde' (its stochastic form; eta = 0 runs 'dpmpp2m'); spacing
        'time' or 'logsnr', the sampling grid; x0_clip: an X0Clip keeps every step's predicted x0 inside per-column bounds
        (the module docstring), None (the default) is the loop without it"""
        check_sampler_settings(eta, solver, spacing)
        if x0_clip is not None and not isinstance(x0_clip, X0Clip):
            raise ValueError(f"x0_clip must be None or an X0Clip, got {type(x0_clip).__name__}")
        self.x0_clip = x0_clip
        self._clip_n = None                  # (mask, (version, T, bounds), n) of the last count of free bounded elements
        self.model, self.S = model, num_sample_steps
        self.eta = float(eta)
        self.solver, self.spacing = solver, spacing
        self.seed = (int(torch.initial_seed()) if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF
        self.use_graph = use_graph and not hip._dry_run
        self._graph: Optional[hip.Graph] = None
        self._stream = None
        self._sig = None
        self._bufs = {}

    guidance = 0.0                           # the classes that take observations set it (classifier-free guidance)
    resample = None                          # (jump, times): the classes that take observations and ids set it
    _takes_ids = True                        # sample() takes the ids that key a call's draws

    def _resampling(self, c: Optional[SampleCall] = None):
        """(jump, times) of a resampled loop, None for the plain one (resample None or times == 1), with the refusals of
        the setting -- at construction (c None) and again at every call, since the attributes may be changed between calls"""
        r = check_resample(self.resample, self.S)
        if r is None:
            return None
        if not self._takes_ids:
            raise ValueError(f"{type(self).__name__} takes no trial ids, and the ids key the re-noise draws of a resampled "
                             f"loop: use StochasticStitchedSampler(eta=0, resample={tuple(r)})")
        if self.eta > 0.0:
            raise ValueError(f"resample = {r} needs eta = 0, got eta = {self.eta}: the step noise of the update kernels is "
                             f"keyed by the step index, so a revisited step would repeat its draw")
        if self._second():
            raise ValueError(f"resample = {r} needs solver 'ddim', got {self.solver!r}: the multistep history of a "
                             f"second-order solver is invalid after a jump")
        if c is not None and c.observed is None:
            raise ValueError(f"resample = {r} needs observations: without them there is nothing to harmonise with")
        return r

    def _check_guidance(self, guidance: float, observations: str):
        """the constructor's check of `guidance` for the classes that take observations"""
        g = float(guidance)
        if g != g or g in (float("inf"), float("-inf")):
            raise ValueError(f"guidance must be finite, got {guidance}")
        if g != 0.0:
            if observations != "clean":
                raise ValueError(f"guidance = {g} needs observations='clean' (the loop of a denoiser trained on clean "
                                 f"conditioning columns), got observations={observations!r}")
            if not float(getattr(self.model, "cond_drop", 0.0)) > 0.0:
                raise ValueError(f"guidance = {g} needs a denoiser that was trained with its conditioning dropped for a share "
                                 f"of the windows (`train --cond-drop P`, model.cond_drop > 0): this one never saw the null "
                                 f"condition, so it has no unconditional prediction")
        self.guidance = g

    def _guided(self, c: SampleCall) -> bool:
        """this call runs the guided loop.  `observations` may be changed between calls: anything but 'clean' is refused"""
        if self.guidance == 0.0:
            return False
        if c.observed is None or self.observations != "clean":
            raise ValueError(f"guidance = {self.guidance} needs observations (observations='clean'): without them there is "
                             f"no condition to guide by")
        return True

    def _second(self) -> bool:
        """a second-order multistep solver: the loop keeps the fp32 history buffer"""
        return self.solver in ("dpmpp2m", "dpmpp2m_sde")

    def _sde(self) -> bool:
        """the stochastic second-order update runs; 'dpmpp2m_sde' at eta = 0 is the 'dpmpp2m' launches"""
        return self.solver == "dpmpp2m_sde" and self.eta > 0.0

    def _call(self, x_T: torch.Tensor, N: int, W: int, ids=None, observed=None, mask=None, lay=None) -> SampleCall:
        """the record of a call whose window batch is x_T [N * W, T, D]"""
        m = self.model
        B, T, D = x_T.shape
        plan = m._get_plan(next(m.parameters()).device)
        Dp = plan.infer_pitch(D) if (hasattr(plan, "infer_pitch") and m.compute_dtype == torch.bfloat16) else D
        return SampleCall(B, T, D, Dp, N, W, ids, observed, mask, lay)

    def _check_observations(self, mask: torch.Tensor, noun: str):
        """a masked call's check of `observations` (the attribute may be changed between calls) and, in 'clean' mode, of
        its mask, whose last dimension is D: the model was trained with exactly its first cond_cols columns clean and
        nothing else.  The verdict is kept per mask tensor (held, so its address is not reused), its version counter and
        cond_cols: a loop that passes the same mask again compares nothing and, with a device mask, does not wait for the
        device."""
        if self.observations not in OBSERVATIONS:
            raise ValueError(f"observations must be one of {OBSERVATIONS}, got {self.observations!r}")
        if self.observations != "clean":
            return
        C, D = int(getattr(self.model, "cond_cols", 0)), mask.shape[-1]
        key = (mask._version, C)
        if self._mask_ok is not None and self._mask_ok[0] is mask and self._mask_ok[1] == key:
            return
        want = torch.zeros(mask.shape, dtype=torch.bool, device=mask.device)
        want[..., :max(C, 0)] = True
        if not 0 < C < D or not torch.equal(mask, want):
            self._mask_ok = None
            raise ValueError(f"observations='clean': {noun} must mark exactly the first cond_cols columns the denoiser was "
                             f"trained on (`train --cond-cols N`, 0 < N < {D}) as observed and no other element; this "
                             f"model's cond_cols is {C}")
        self._mask_ok = (mask, key)

    @torch.no_grad()
    def sample(self, x_T: torch.Tensor, steps: Optional[int] = None,
               window_ids: Union[None, Sequence[int], torch.Tensor] = None) -> torch.Tensor:
        """x_T [B,T,D] ~ N(0,1) -> x_0.  `steps` (<= num_sample_steps) truncates the loop (benchmarks).  window_ids (default
        0 .. B-1): with eta > 0 the step noise of window b is keyed by (seed, window_ids[b], step), whatever its place in
        the batch; unused at eta = 0."""
        return self._run(self._call(x_T, x_T.shape[0], 1, window_ids), x_T, steps)

    def _run(self, c: SampleCall, x_T: torch.Tensor, steps: Optional[int]) -> torch.Tensor:
        self._resampling(c)                  # a refused call leaves the sampler as it was
        if not x_T.is_cuda and not hip._dry_run:
            x_T = x_T.to(next(self.model.parameters()).device)
        if hip._dry_run:
            return self._sample(c, x_T, steps)
        # hipGraph capture is not allowed on the legacy default stream -> run on a side stream
        if self._stream is None:
            self._stream = hip.new_stream(x_T.device)
        cur = torch.cuda.current_stream()
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            out = self._sample(c, x_T, steps)
        cur.wait_stream(self._stream)
        return out

    @torch.no_grad()
    def sample_noise(self, batch: int, window: int, feat: int, seed: Optional[int] = None, draw: int = 0,
                     steps: Optional[int] = None, window_ids=None) -> torch.Tensor:
        """x_T ~ N(0,1) drawn ON the device (csrc/noise.hip: Philox keyed by (seed, draw); `seed` defaults to torch's) and
        denoised to x_0 -- no host random numbers, no H2D copy of the start state."""
        return self.sample(self.draw_start(batch, window, feat, seed, draw), steps, window_ids)

    def draw_start(self, batch: int, window: int, feat: int, seed: Optional[int] = None, draw: int = 0) -> torch.Tensor:
        """the start state x_T ~ N(0,1) of sample_noise, [batch, window, feat] in the compute dtype on the model's device"""
        m = self.model
        dev = next(m.parameters()).device
        x_T = torch.empty((batch, window, feat), dtype=m.compute_dtype, device=dev)
        seed = int(torch.initial_seed()) if seed is None else int(seed)
        hip.diffusion_draw(seed, step=int(draw), stream_id=0x40000000, eps=x_T)
        return x_T

    def _prepare(self, c: SampleCall, tabs, dev):
        """the signature of the captured step and the device buffers that live as long as it does; a new signature drops
        the graph and makes new buffers.  The captured step bakes in raw pointers: the model's flat parameter buffer and
        bf16 shadow (a HipTrainer built after a first sample() re-packs them), the schedule tables (set_sampler() of another
        sampler re-creates them), the layout's tables -- all of them are part of the signature, so a change re-captures
        instead of replaying stale pointers.  Then, per kind of loop: the observation table's pointer and its kind (a table
        made for the other mode may come back at a freed table's address); solver and grid and the second-order table,
        nothing at the defaults; eta and, for a stochastic loop, the seed and its solver's eta tables."""
        m, lay = self.model, c.lay
        B, T, D, Dp = c.B, c.T, c.D, c.Dp
        second, noisy, sde, cond = self._second(), self.eta > 0.0, self._sde(), c.observed is not None
        ptr = lambda t: t.data_ptr()
        sig = ((B, T, D), m.compute_dtype, ptr(m._flat), ptr(m._shadow) if m._shadow is not None else 0, ptr(tabs.temb),
               ptr(tabs.ddim_coef), ptr(tabs.ddim_t), self.S, Dp)
        if lay is not None:
            sig += ("stitch", c.N, lay["F"], self.hop, self.blend, ptr(lay["start"]), ptr(lay["cover"]), ptr(lay["wn"]))
            if self._one_window_step(c):
                sig += ("one_window_step",)  # another update launch: the step itself changes with the setting here
        if cond:
            sig += (ptr(tabs.obs_coef), tabs.observations)
        if self.solver != "ddim" or self.spacing != "time":
            sig += (self.solver, self.spacing, ptr(tabs.dpmpp_coef) if second else 0)
        if sde:
            sig += (self.eta, self.seed, ptr(tabs.sde_coef), ptr(tabs.sde_obs_noise_coef))
        elif noisy:
            sig += (self.eta, self.seed, ptr(tabs.ddim_coef_eta), ptr(tabs.obs_noise_coef))
        else:
            sig += (0.0,)
        clip = self._clip_call(c, tabs)
        if clip is not None:
            # the launch bakes in the mode, the rank (a function of the call's mask and the bounds) and the tables' addresses
            sig += ("x0_clip", self.x0_clip.mode, clip["k"]) + tuple(ptr(clip[n]) for n in ("coef", "lo", "hi", "m", "h", "ih"))
        if self._prediction() != "eps":
            sig += ("prediction", self._prediction(), ptr(tabs.inv_sqrt_1mab))   # one more launch per step, by kind
        guided = self._guided(c)
        if guided:
            # the seam's launches bake in the strength, the conditioning width and xin's address.  xin belongs to the
            # signature it is part of: while that one is current its pointer is the live buffer's
            sig += ("cfg", self.guidance, int(m.cond_cols))
            if self._sig is not None and sig == self._sig[:-1] and self._sig[-1] == ptr(self._bufs["xin"]):
                return
        if sig == self._sig:
            return
        state = lambda dtype=m.compute_dtype, n=B: torch.zeros((n, T, Dp), dtype=dtype, device=dev)
        # guided: the B windows and their null-condition twins.  The conditioning and pad columns of the second half of xin
        # are zero from here on (no launch writes them); x, the state every other launch sees, is the first half
        xin = state(n=2 * B) if guided else None
        bufs = {"x": xin[:B] if guided else state(), "t": torch.empty(2 * B if guided else B, dtype=torch.int64, device=dev),
                "ctr": torch.zeros(1, dtype=torch.int32, device=dev)}
        if guided:
            bufs.update(xin=xin, eps=state(n=2 * B))             # the noise buffer is pitched even when Dp == D
            sig += (ptr(xin),)
        elif Dp != D:
            bufs["eps"] = state()
        if cond:
            # pitched like the state, pad columns 0 (the mask's pad columns are free, so they stay 0 in x)
            bufs.update(x0=state(), z=state(), mask=torch.zeros((T, Dp), dtype=torch.uint8, device=dev))
        if noisy:
            bufs["win"] = torch.zeros(c.N, dtype=torch.int64, device=dev)       # one id per trial (per window at W = 1)
        if second:
            # the previous step's data prediction, fp32 whatever the state's dtype, pitched like the state.  The first
            # row of the table does not read it, so a new batch needs no reset
            bufs["hist"] = state(torch.float32)
        if sde:
            bufs["one_window"] = tuple(t.to(dev) for t in stitch_layout(T, T, T)[:3])
        self._sig, self._graph, self._bufs = sig, None, bufs

    def _clip_call(self, c: SampleCall, tabs):
        """None without x0_clip; else the clip's tables for this call (DiffusionTables.set_clip, made when the bounds or the
        grid changed) with 'k': the rank of the 'dynamic' quantile among the n free bounded elements of one window, which
        depends on the call's mask and the bounds alone (0 when n == 0: nothing is launched).  The count is kept per mask
        tensor and version, so a loop that passes the same mask again does not wait for the device."""
        q = self.x0_clip
        if q is None:
            return None
        if len(q.lo) != c.D:
            raise ValueError(f"x0_clip: the bounds hold {len(q.lo)} columns, a window row has D = {c.D}")
        if not tabs.clip_serves(self.S, self.spacing, q.lo, q.hi):
            tabs.set_clip(q.lo, q.hi)
        clip = tabs.clip
        key = (None if c.mask is None else c.mask._version, c.T, clip["key"])
        kept = self._clip_n
        if kept is None or kept[0] is not c.mask or kept[1] != key:
            bounded = clip["bounded"]
            if c.mask is None:
                n = c.T * int(bounded.sum())
            else:
                free = (c.mask.to(device="cpu") == 0).sum(dim=0)          # [D] free frames per column
                n = int(free[bounded].sum())
            kept = self._clip_n = (c.mask, key, n)
        n = kept[2]
        return dict(clip, n=n, k=clip_rank(q.quantile, n) if n else 0)

    def _launch_clip(self, c: SampleCall, x, eps, ctr, tabs):
        """the x0 clip's one launch of a step, over the B windows of x / eps as [B, T, ld]; nothing without x0_clip or when no
        element is both free and bounded"""
        clip = self._clip_call(c, tabs)
        if clip is None or clip["n"] == 0:
            return
        mask = self._bufs.get("mask") if c.observed is not None else None
        x3, e3 = x.view(c.B, c.T, -1), eps.view(c.B, c.T, -1)
        if self.x0_clip.mode == "range":
            hip.x0_clip_range(x3, e3, mask, clip["lo"], clip["hi"], clip["coef"], step_dev=ctr, D=c.D)
        else:
            hip.x0_clip_dynamic(x3, e3, mask, clip["lo"], clip["hi"], clip["coef"], clip["m"], clip["h"], clip["ih"], clip["k"],
                                step_dev=ctr, D=c.D)

    def _prediction(self) -> str:
        """what the model's output approximates (prediction.py): 'eps' unless the model says otherwise"""
        return check_kind(getattr(self.model, "prediction", "eps"))

    def _launch_convert(self, c: SampleCall, x, out, t_vec, tabs):
        """an x0 / v model's output becomes the noise prediction every launch after it expects (ib_pred_to_eps), over the B
        windows of x / out as [B, T, ld] at the levels t_vec; nothing for an eps model"""
        kind = self._prediction()
        if kind == "eps":
            return
        hip.pred_to_eps(x.view(c.B, c.T, -1), out.view(c.B, c.T, -1), t_vec, tabs.sqrt_ab, tabs.sqrt_1mab, tabs.inv_sqrt_1mab,
                        kind, D=c.D)

    def _start_masked(self, c: SampleCall, x, tabs):
        """the masked loop's start state, once x holds the start draw: the observation, the mask and the draw z go into
        their buffers and ib_ddim_cond_init pins the observed elements"""
        D = c.D
        x0, z, m = self._bufs["x0"], self._bufs["z"], self._bufs["mask"]
        x0[:, :, :D].copy_(c.observed.to(device=x0.device, dtype=x0.dtype))
        m[:, :D].copy_(c.mask.to(device=m.device, dtype=torch.uint8))
        z.copy_(x)
        hip.ddim_cond_init(x, x0, z, m, tabs.obs_coef, D=D)
        if c.W > 1:
            # the invariant at the start: every copy of a trial element holds its first copy's bits (the start kernel rounds
            # by position in the window batch, which differs between the copies when the row pitch is no multiple of 8)
            x.copy_(_cut(c.lay, _join(c.lay, x, c.N)))

    def _sample(self, c: SampleCall, x_T: torch.Tensor, steps: Optional[int] = None) -> torch.Tensor:
        jumps = self._resampling(c)
        ids = _checked_ids(c.ids, c.N, "window" if c.lay is None else "trial") if self.eta > 0.0 or jumps else None
        m = self.model
        m.ensure_packed()
        m.sync_shadow()
        dev = m._flat.device
        tabs = m.tables(dev)
        obs = self.observations if c.observed is not None else None
        if not tabs.serves(self.S, self.eta, self.solver, self.spacing, obs):
            tabs.set_sampler(self.S, self.eta, self.solver, self.spacing, observations=obs or tabs.observations)
        if jumps and not tabs.serves(self.S, self.eta, self.solver, self.spacing, obs, resample_jump=jumps[0]):
            tabs.set_resample(jumps[0])      # the jump table alone: the step's tables, and so its capture, stay
        plan = m._get_plan(dev)
        self._prepare(c, tabs, dev)
        if jumps:
            # what a jump reads beside the step's buffers.  The eta = 0 step reads neither, so they are no part of the
            # captured step's signature: resampling goes on, off or to other values and the same capture is replayed
            b = self._bufs
            if "win" not in b:
                b["win"] = torch.zeros(c.N, dtype=torch.int64, device=dev)
            if c.lay is None and "one_window" not in b:
                b["one_window"] = tuple(t.to(dev) for t in stitch_layout(c.T, c.T, c.T)[:3])
        if ids is not None:
            self._bufs["win"].copy_(ids)
        x, t_vec, ctr = self._bufs["x"], self._bufs["t"], self._bufs["ctr"]
        x[:, :, :c.D].copy_(x_T.to(device=dev, dtype=m.compute_dtype))
        if c.observed is not None:
            self._start_masked(c, x, tabs)
        ctr.zero_()
        hip.fill_i64(t_vec, int(tabs.ddim_t[0]))
        if "xin" in self._bufs:
            hip.cfg_mirror(self._bufs["xin"], t_vec, int(m.cond_cols), D=c.D)
        P = m.param_source()
        if hasattr(plan, "set_inference"):
            plan.set_inference(True)             # weights are frozen for the whole loop
            plan.prepare_inference(P, c.T, c.D, table=tabs.temb)
        try:
            return self._loop(c, x, t_vec, ctr, tabs, P, steps, jumps)
        finally:
            if hasattr(plan, "set_inference"):
                plan.set_inference(False)

    def _loop(self, c: SampleCall, x, t_vec, ctr, tabs, P, steps, jumps=None):
        """the plain loop, or the walk of a resampled one (schedule.resample_walk): a 'step' is the one step below, eager or
        the captured graph replayed unchanged; a 'jump' is issued on the same stream between the replays, with no host
        synchronisation.  `steps` truncates either after that many denoiser evaluations"""
        if jumps:
            walk = resample_walk(self.S, *jumps)
            total = sum(op[0] == "step" for op in walk)
            n = total if steps is None else min(steps, total)
        else:
            walk = None
            n = self.S if steps is None else min(steps, self.S)
        done = 0
        if self.use_graph and self._graph is None:
            self._step_launches(c, x, t_vec, ctr, tabs, P)       # eager warm-up step allocates plan buffers
            done = 1
            if n > 1:
                g = hip.Graph()
                g.begin()
                self._step_launches(c, x, t_vec, ctr, tabs, P)
                g.end()
                self._graph = g

        def step():
            if self._graph is not None:
                self._graph.launch()
            else:
                self._step_launches(c, x, t_vec, ctr, tabs, P)

        if walk is None:
            for _ in range(done, n):
                step()
        else:
            # the first two operations of any walk are steps (a jump point lies at position >= 2), so the warm-up step
            # above is ('step', 0)
            evals = 0
            for op in walk:
                if evals >= n:
                    break
                if op[0] == "jump":
                    self._jump_launches(c, x, t_vec, ctr, tabs, jumps[0], op[2])
                    continue
                if evals >= done:
                    step()
                evals += 1
        return x[:, :, :c.D].clone()

    def _jump_launches(self, c: SampleCall, x, t_vec, ctr, tabs, jump: int, visit: int):
        """one jump of a resampled loop: the state at the counter's position is diffused back `jump` levels
        (ib_resample_renoise, csrc/resample.hip: fresh noise at the free elements keyed by (seed, id, visit), the observed
        ones pinned to their level), the counter follows, and a guided loop mirrors the re-noised free columns and the new
        timesteps into the null-condition twins"""
        b = self._bufs
        v = lambda t: t.view((c.N, c.W) + tuple(t.shape[1:]))
        start, cover = (c.lay["start"], c.lay["cover"]) if c.lay is not None else b["one_window"][:2]
        hip.resample_renoise(v(x), v(b["x0"]), v(b["z"]), b["mask"], tabs.resample_coef, tabs.obs_coef, tabs.ddim_t, start,
                             cover, b["win"], self.seed, jump, visit, t_vec[:c.B], step_dev=ctr, D=c.D)
        hip.counter_add(ctr, -jump)
        if "xin" in b:
            hip.cfg_mirror(b["xin"], t_vec, int(self.model.cond_cols), D=c.D)

    def _step_launches(self, c: SampleCall, x, t_vec, ctr, tabs, P: ParamSource):
        plan = self.model._get_plan(x.device)
        eps_buf = self._bufs.get("eps")
        xin = self._bufs.get("xin")
        if xin is not None:
            # the guided step (the module docstring): x is the first half of xin, the update writes t_vec[:B]
            B2, T, Dp = xin.shape
            plan.forward(xin.view(B2 * T, Dp)[:, :c.D], t_vec, tabs.temb, P, out=eps_buf.view(B2 * T, Dp)[:, :c.D],
                         BT=(B2, T))
            hip.cfg_combine(eps_buf, self.guidance)
            self._launch_convert(c, x, eps_buf[:c.B], t_vec[:c.B], tabs)
            self._launch_clip(c, x, eps_buf[:c.B], ctr, tabs)
            self._launch_update(c, x, eps_buf[:c.B], ctr, t_vec[:c.B], tabs)
            hip.cfg_mirror(xin, t_vec, int(self.model.cond_cols), D=c.D)
        elif eps_buf is not None:
            # pitched state / noise buffers [B, T, Dp] with zero pad columns (plans.infer_pitch): the plan sees row-padded
            # 2-D views; the DDIM update runs over the whole pitched buffers (0 stays 0 in the pad columns)
            B, T, Dp = x.shape
            plan.forward(x.view(B * T, Dp)[:, :c.D], t_vec, tabs.temb, P, out=eps_buf.view(B * T, Dp)[:, :c.D], BT=(B, T))
            self._launch_convert(c, x, eps_buf, t_vec, tabs)
            self._launch_clip(c, x, eps_buf, ctr, tabs)
            self._launch_update(c, x, eps_buf, ctr, t_vec, tabs)
        else:
            eps = plan.forward(x, t_vec, tabs.temb, P)
            self._launch_convert(c, x, eps, t_vec, tabs)
            self._launch_clip(c, x, eps, ctr, tabs)
            self._launch_update(c, x, eps, ctr, t_vec, tabs)
        hip.counter_add(ctr, 1)

    def _one_window_step(self, c: SampleCall) -> bool:
        """a resampled loop over one-window trials (F == T) updates with the per-window entry: one window has nothing to
        blend, and so the loop IS ConditionalDDIMSampler(resample=...) with window ids = trial ids bit for bit at every row
        pitch -- the stitched entry rounds an observed element by column, the per-window one by flat offset, and the two
        differ where the pitch is no multiple of 8 (include/ib_hip_stitch.h).  The plain stitched loops keep their entry"""
        return c.lay is not None and c.W == 1 and self._resampling(c) is not None

    def _launch_update(self, c: SampleCall, x, eps, ctr, t_vec, tabs):
        """THE choice of the update launch (the module docstring's table): by layout, solver order, eta > 0, observations"""
        b, lay = self._bufs, None if self._one_window_step(c) else c.lay
        second, noisy, sde, cond = self._second(), self.eta > 0.0, self._sde(), c.observed is not None
        # the stitched entries and ib_sde_dpmpp_step see the state as [N, W, T, ld]: a per-window 'dpmpp2m_sde' loop as
        # [B, 1, T, ld], every window a trial of its own (the layout stitch_layout(T, T, T)), the window ids as trial ids
        wide = lay is not None or sde
        v = (lambda t: t.view((c.N, c.W) + tuple(t.shape[1:]))) if wide else (lambda t: t)
        x0, z, m, oc, on = (v(b["x0"]), v(b["z"]), b["mask"], tabs.obs_coef,
                            tabs.sde_obs_noise_coef if sde else tabs.obs_noise_coef) if cond else (None,) * 5
        windows = (lay["start"], lay["cover"], lay["wn"]) if lay is not None else b.get("one_window")
        step = dict(step_dev=ctr, t_out=t_vec)
        if sde:
            hip.sde_dpmpp_step(v(x), v(eps), v(b["hist"]), x0, z, m, tabs.sde_coef, oc, on, tabs.ddim_t, *windows, b["win"],
                               self.seed, D=c.D, **step)
        elif lay is not None and noisy:
            hip.stitch_ddim_step_noise(v(x), v(eps), x0, z, m, tabs.ddim_coef_eta, oc, on, tabs.ddim_t, *windows, b["win"],
                                       self.seed, D=c.D, **step)
        elif lay is not None and second:
            hip.stitch_dpmpp_step(v(x), v(eps), v(b["hist"]), x0, z, m, tabs.dpmpp_coef, oc, tabs.ddim_t, *windows, D=c.D,
                                  **step)
        elif lay is not None:
            hip.stitch_ddim_step(v(x), v(eps), x0, z, m, tabs.ddim_coef, oc, tabs.ddim_t, *windows, D=c.D, **step)
        elif second and cond:
            hip.dpmpp_cond_step(x, eps, b["hist"], x0, z, m, tabs.dpmpp_coef, oc, tabs.ddim_t, D=c.D, **step)
        elif second:
            hip.dpmpp_step(x, eps, b["hist"], tabs.dpmpp_coef, tabs.ddim_t, **step)
        elif noisy and cond:
            hip.ddim_cond_step_noise(x, eps, x0, z, m, tabs.ddim_coef_eta, oc, on, tabs.ddim_t, b["win"], self.seed, D=c.D,
                                     **step)
        elif noisy:
            hip.ddim_step_noise(x, eps, tabs.ddim_coef_eta, tabs.ddim_t, b["win"], self.seed, D=c.D, **step)
        elif cond:
            hip.ddim_cond_step(x, eps, x0, z, m, tabs.ddim_coef, oc, tabs.ddim_t, D=c.D, **step)
        else:
            hip.ddim_step(x, eps, tabs.ddim_coef, tabs.ddim_t, **step)


class ConditionalDDIMSampler(DDIMSampler):
    """DDIM inpainting with an unconditional denoiser (replacement method): the elements a mask marks as observed
    are pinned, at every step, to the observation forward-noised to that step's noise level with the fixed start draw z,
    sqrt(ab) x0 + sqrt(1 - ab) z -- with eta = 0 that is exactly the DDIM trajectory of the observation, so the loop stays
    deterministic and its last step (to alpha_bar = 1) returns the observation itself.  The free elements follow the DDIM
    update.  With eta > 0 an observed element follows the DDIM posterior given the observation: its noise, kept in the z
    buffer, becomes r z + q z' at every step (schedule.observation_noise_coefficients), and the last step still lands on
    the observation.  With solver = 'dpmpp2m' the free elements take the DPM-Solver++(2M) update instead and the observed ones
    the same pinned value (ib_dpmpp_cond_step); with 'dpmpp2m_sde' and eta > 0 the free elements take its stochastic form and the
    stored noise of an observed element becomes r z + q z' by that solver's own table
    (schedule.sde_observation_noise_coefficients).  Same captured single-step graph as DDIMSampler; only the update launch differs (ib_ddim_cond_step, the same
    launch count per step).  The observation, the draw and the mask live in sampler-owned device buffers that the capture
    reads, so a new batch of the same shape is copied in and the captured step replayed.

    observations = 'clean' is the loop of a denoiser trained on clean conditioning columns (`train --cond-cols`,
    model.cond_cols > 0): an observed element IS the observation, in the start state and after every step, so the network
    sees what it saw in training.  Same launches: the observation table's rows are all (1, 0)
    (schedule.clean_observation_coefficients).  The mask must then be the first model.cond_cols columns of every frame.
    The attribute may be changed between calls; the step is captured again."""

    def __init__(self, model, num_sample_steps: int = 100, use_graph: bool = True, eta: float = 0.0,
                 seed: Optional[int] = None, solver: str = "ddim", spacing: str = "time", observations: str = "noised",
                 guidance: float = 0.0, resample=None, x0_clip: Optional[X0Clip] = None):
        check_sampler_settings(eta, solver, spacing, observations)
        super().__init__(model, num_sample_steps, use_graph, eta, seed, solver, spacing, x0_clip=x0_clip)
        self.observations = observations
        self._check_guidance(guidance, observations)
        self.resample = resample
        self._resampling()
        self._mask_ok = None                 # (mask, (version, cond_cols)) of the last mask 'clean' mode accepted

    @torch.no_grad()
    def sample(self, x_T: torch.Tensor, observed: torch.Tensor, mask: torch.Tensor,
               steps: Optional[int] = None, window_ids=None) -> torch.Tensor:
        """x_T [B,T,D] ~ N(0,1) (the draw z), observed [B,T,D], mask [T,D] bool (True = observed) -> x_0, which equals the
        observation (in the compute dtype) wherever mask is True.  `steps` truncates the loop and window_ids key the step
        noise as in DDIMSampler."""
        B, T, D = x_T.shape
        if tuple(observed.shape) != (B, T, D):
            raise ValueError(f"observed must be {(B, T, D)} like x_T, got {tuple(observed.shape)}")
        if tuple(mask.shape) != (T, D) or mask.dtype != torch.bool:
            raise ValueError(f"mask must be a [T, D] = {(T, D)} bool tensor, got {tuple(mask.shape)} {mask.dtype}")
        self._check_observations(mask, "the mask")
        return self._run(self._call(x_T, B, 1, window_ids, observed, mask), x_T, steps)

    @torch.no_grad()
    def sample_noise(self, batch: int, window: int, feat: int, observed: torch.Tensor, mask: torch.Tensor,
                     seed: Optional[int] = None, draw: int = 0, steps: Optional[int] = None,
                     window_ids=None) -> torch.Tensor:
        """as DDIMSampler.sample_noise: z = x_T drawn on the device from (seed, draw)"""
        return self.sample(self.draw_start(batch, window, feat, seed, draw), observed, mask, steps, window_ids)


class StitchedDDIMSampler(DDIMSampler):
    """Samples a whole trial of F >= model.window frames with a denoiser that sees windows of T = model.window frames
    (MultiDiffusion / DiffCollage stitching).  The trial is covered by overlapping windows (schedule.stitch_layout: a window
    every `hop` frames, default T // 2, and a last one that ends on the last frame); after every denoiser evaluation the
    noise predictions of all windows that cover a trial frame are blended ('ramp': a window fades in and out over its
    overlap; 'uniform') and every copy of that frame receives the same updated value, so the windows stay one sequence all
    the way down instead of diverging from the first step.  The state is the window batch [N * W, T, D] the denoiser plan
    consumes: the plans, the captured one-step graph and the launch count per step are DDIMSampler's; only the update launch
    differs (ib_stitch_ddim_step / ib_stitch_dpmpp_step, csrc/stitch.hip).  With F == T it is ConditionalDDIMSampler (or
    DDIMSampler without observations) bit for bit, with hop == T and F a multiple of T the per-window sampler on disjoint
    windows.

    observed / mask_cols make it the masked loop of ConditionalDDIMSampler: mask_cols is a [D] bool, the same columns
    observed in every frame (a per-frame mask would disagree with itself where windows overlap).  Deterministic only:
    eta > 0 is refused, the step noise of the stochastic update is keyed by window and in-window frame and would have to be
    keyed by trial frame.  The constructor takes `eta` only to refuse it: code that builds its samplers from one set of
    arguments gets the reason instead of a TypeError; any value but 0 is a ValueError.

    `layout` (the tables of the last trial sampled) and `to_windows` (a trial tensor cut into that layout's windows) are
    for callers that want the same windows for a per-window sampler.  One layout is kept: a trial of another length
    replaces it, and the step is captured again."""

    def __init__(self, model, num_sample_steps: int = 100, hop: Optional[int] = None, blend: str = "ramp",
                 use_graph: bool = True, solver: str = "ddim", spacing: str = "time", observations: str = "noised",
                 seed: Optional[int] = None, eta: float = 0.0, guidance: float = 0.0, resample=None,
                 x0_clip: Optional[X0Clip] = None):
        if float(eta) != 0.0:
            raise ValueError(f"StitchedDDIMSampler is deterministic: eta must be 0, got {eta} (the step noise of an eta > 0 "
                             f"loop is keyed by window and in-window frame, not by trial frame)")
        check_sampler_settings(0.0, solver, spacing, observations)
        super().__init__(model, num_sample_steps, use_graph, 0.0, seed, solver, spacing, x0_clip=x0_clip)
        self.observations = observations
        self._check_guidance(guidance, observations)
        if getattr(model, "window", None) is None:
            raise ValueError("StitchedDDIMSampler needs a denoiser that states its window (model.window frames)")
        self.T = int(model.window)
        self.hop = self.T // 2 if hop is None else int(hop)
        self.blend = blend
        stitch_layout(3 * self.T, self.T, self.hop, blend)     # refuses a bad hop or blend here, not at the first call
        self._lay = None                     # the layout of the last trial length sampled, the only one kept
        self._mask_ok = None                 # (mask_cols, (version, cond_cols)) of the last mask 'clean' mode accepted
        self.resample = resample             # taken only to be refused with the reason, as eta is: this class has no ids
        self._resampling()

    _takes_ids = False

    @property
    def layout(self) -> Optional[dict]:
        """the layout of the last trial sampled (None before the first call): the kernel's tables 'start', 'cover', 'wn' on
        the device, 'F' and 'W', the gather index 'gather' ([W, T] trial frames) and each frame's first copy 'w0', 't0'"""
        return self._lay

    def _layout(self, F: int, dev):
        """the layout of a trial of F frames on `dev`: the kernel's tables, the gather index trial -> windows ([W, T] trial
        frames) and each frame's first copy (window, in-window frame).  Built when F or the device changes."""
        key = (F, str(dev), self.hop, self.blend)
        if self._lay is None or self._lay["key"] != key:
            start, cover, wn, _ = stitch_layout(F, self.T, self.hop, self.blend)
            gather = start.long()[:, None] + torch.arange(self.T)[None, :]
            w0 = cover[:, 0].long()
            t0 = torch.arange(F) - start.long()[w0]
            self._lay = {"start": start.to(dev), "cover": cover.to(dev), "wn": wn.to(dev), "gather": gather.to(dev),
                         "w0": w0.to(dev), "t0": t0.to(dev), "F": F, "W": start.numel(), "key": key}
        return self._lay

    def to_windows(self, trial: torch.Tensor) -> torch.Tensor:
        """[N, F, D] -> [N * W, T, D]: every window's frames in the layout of the last trial sampled (plumbing: an index, no
        arithmetic)"""
        if self._lay is None or trial.dim() != 3 or trial.shape[1] != self._lay["F"]:
            raise ValueError(f"to_windows: a [N, F, D] trial of the last sampled length is needed, got {tuple(trial.shape)}")
        return _cut(self._lay, trial)

    @torch.no_grad()
    def sample(self, z: torch.Tensor, observed: Optional[torch.Tensor] = None, mask_cols: Optional[torch.Tensor] = None,
               steps: Optional[int] = None) -> torch.Tensor:
        """z [N, F, D] ~ N(0, 1), the trial's start draw -> x_0 [N, F, D].  observed [N, F, D] and mask_cols [D] bool (True:
        the column is observed in every frame) come together; the result equals the observation, in the compute dtype, in
        those columns.  `steps` truncates the loop."""
        return self._sample_trials(z, observed, mask_cols, steps, None)

    def _sample_trials(self, z, observed, mask_cols, steps, trial_ids) -> torch.Tensor:
        if z.dim() != 3:
            raise ValueError(f"z must be [N, F, D], got {tuple(z.shape)}")
        N, F, D = z.shape
        if (observed is None) != (mask_cols is None):
            raise ValueError("observed and mask_cols come together (the masked loop) or not at all")
        if observed is not None:
            if tuple(observed.shape) != (N, F, D):
                raise ValueError(f"observed must be {(N, F, D)} like z, got {tuple(observed.shape)}")
            if not isinstance(mask_cols, torch.Tensor) or tuple(mask_cols.shape) != (D,) or mask_cols.dtype != torch.bool:
                raise ValueError(f"mask_cols must be a [D] = [{D}] bool tensor (the same columns are observed in every "
                                 f"frame), got {tuple(getattr(mask_cols, 'shape', ()))} {getattr(mask_cols, 'dtype', None)}")
            self._check_observations(mask_cols, "mask_cols")
        m = self.model
        dev = z.device if (z.is_cuda or hip._dry_run) else next(m.parameters()).device
        lay = self._lay = self._layout(F, dev)                 # refuses F < model.window
        x_T = _cut(lay, z.to(dev))
        if observed is not None:
            observed = _cut(lay, observed.to(device=dev, dtype=m.compute_dtype))
            mask_cols = mask_cols.to(device=dev, dtype=torch.uint8)[None, :].expand(self.T, D)
        c = self._call(x_T, N, lay["W"], trial_ids, observed, mask_cols, lay)
        return _join(lay, self._run(c, x_T, steps), N)

    @torch.no_grad()
    def sample_noise(self, batch: int, frames: int, feat: int, observed: Optional[torch.Tensor] = None,
                     mask_cols: Optional[torch.Tensor] = None, seed: Optional[int] = None, draw: int = 0,
                     steps: Optional[int] = None) -> torch.Tensor:
        """as DDIMSampler.sample_noise: z [batch, frames, feat] drawn on the device from (seed, draw)"""
        return self.sample(self.draw_start(batch, frames, feat, seed, draw), observed, mask_cols, steps)


class StochasticStitchedSampler(StitchedDDIMSampler):
    """StitchedDDIMSampler with eta in [0, 1]: the stochastic DDIM / DDPM loop over a whole trial.  The step noise is drawn
    inside the update kernel per TRIAL element, keyed by (seed, trial id, step, trial frame, column), so every copy of an
    element in the overlapping windows receives the same normal and the windows stay one sequence; a trial's result depends
    on its id, not on its place in the batch or on the batch's size.  With observations, an observed element's stored noise
    follows the DDIM posterior given the observation (ConditionalDDIMSampler's eta > 0 loop), in every copy.  Layout,
    to_windows, the start state, the captured one-step graph and the launch count per step are the parent's; only the update
    launch differs (ib_stitch_ddim_step_noise, csrc/stitch.hip).  eta = 0 is the parent class bit for bit.  With
    F == T it is ConditionalDDIMSampler(eta, seed) (or DDIMSampler without observations) with window ids = trial ids.  The
    solver is 'ddim' unless the keyword solver = 'dpmpp2m_sde' is given: the stochastic second-order update
    (ib_sde_dpmpp_step, csrc/sde.hip; it belongs with spacing = 'logsnr'), under the same keys.  'dpmpp2m' stays
    deterministic and is StitchedDDIMSampler's.  The trial ids live in a device buffer the captured update reads ('win',
    one id per TRIAL), so a new batch or new ids of the same shape replay the captured step."""

    def __init__(self, model, num_sample_steps: int = 100, eta: float = 1.0, hop: Optional[int] = None, blend: str = "ramp",
                 use_graph: bool = True, spacing: str = "time", observations: str = "noised", seed: Optional[int] = None,
                 guidance: float = 0.0, **keywords):
        """keywords: solver = 'ddim' (the default) or 'dpmpp2m_sde', resample = (jump, times) (eta = 0 and 'ddim' only:
        RePaint resampling, ConditionalDDIMSampler's) and x0_clip = X0Clip(...) (the module docstring), by keyword only.  `solver` is not a named parameter:
        tests/test_stitch_noise_plumbing_cpu.py pins that this signature names no `solver`, from when the class had one
        solver; a misspelt keyword is still a TypeError"""
        solver = keywords.pop("solver", "ddim")
        resample = keywords.pop("resample", None)
        x0_clip = keywords.pop("x0_clip", None)
        if keywords:
            raise TypeError(f"StochasticStitchedSampler: unexpected keyword arguments {sorted(keywords)}")
        if solver == "dpmpp2m":
            raise ValueError("solver 'dpmpp2m' is deterministic: use StitchedDDIMSampler for it; the stochastic loop takes "
                             "'ddim' or 'dpmpp2m_sde'")
        if solver not in ("ddim", "dpmpp2m_sde"):
            raise ValueError(f"solver must be 'ddim' or 'dpmpp2m_sde', got {solver!r}")
        check_sampler_settings(eta, solver, spacing, observations)
        super().__init__(model, num_sample_steps, hop, blend, use_graph, solver, spacing, observations, seed,
                         guidance=guidance, x0_clip=x0_clip)
        self.eta = float(eta)                # the parent's constructor hands DDIMSampler eta = 0
        self.resample = resample
        self._resampling()

    _takes_ids = True

    @torch.no_grad()
    def sample(self, z: torch.Tensor, observed: Optional[torch.Tensor] = None, mask_cols: Optional[torch.Tensor] = None,
               steps: Optional[int] = None, trial_ids: Union[None, Sequence[int], torch.Tensor] = None) -> torch.Tensor:
        """as StitchedDDIMSampler.sample.  trial_ids (default 0 .. N-1): the step noise of trial n is keyed by (seed,
        trial_ids[n], step), whatever its place in the batch; unused at eta = 0."""
        return self._sample_trials(z, observed, mask_cols, steps, trial_ids)

    @torch.no_grad()
    def sample_noise(self, batch: int, frames: int, feat: int, observed: Optional[torch.Tensor] = None,
                     mask_cols: Optional[torch.Tensor] = None, seed: Optional[int] = None, draw: int = 0,
                     steps: Optional[int] = None, trial_ids=None) -> torch.Tensor:
        """as StitchedDDIMSampler.sample_noise, with the trial ids of sample()"""
        return self.sample(self.draw_start(batch, frames, feat, seed, draw), observed, mask_cols, steps, trial_ids)
