"""[BUILD-DEFINED] Ground-contact labels inferred from observed motion with a trained diffusion denoiser.

A window is the denoiser's ``[F, D]`` matrix (``MotionWindowView.matrix``): the frame's model-input channels, then the
30 label channels cop | force | torque | wrench (``LOSS_KEY_ORDER``, widths 6 / 6 / 6 / 12).  The input columns of
every frame are observed, the label columns are free, and the masked DDIM loop (``ConditionalDDIMSampler``) fills them
in.  The result is the reference regression models' outputs dict, so the same ``RegressionLossEvaluator``, CSV rows and
report apply."""
from typing import Dict, Optional

import torch

from ..data.AddBiomechanicsDataset import INPUT_KEY_ORDER, LOSS_KEY_ORDER, LOSS_KEY_WIDTHS, MotionWindowView
from ..diffusion.sampler import ConditionalDDIMSampler

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
    (seed, draw + b), so a window's result does not depend on how windows are batched into calls."""

    def __init__(self, model, num_sample_steps: int = 100, seed: int = 0, output_data_format: str = 'all_frames',
                 use_graph: bool = True):
        if output_data_format != 'all_frames':
            raise ValueError("DiffusionLabelPredictor: the diffusion models need --output-data-format all_frames")
        self.model, self.seed = model, int(seed)
        self.sampler = ConditionalDDIMSampler(model, num_sample_steps, use_graph=use_graph)

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

    @torch.no_grad()
    def __call__(self, inputs: Dict[str, torch.Tensor], labels: Optional[Dict[str, torch.Tensor]] = None,
                 draw: int = 0) -> Dict[str, torch.Tensor]:
        obs = self.window_matrix(inputs)
        B, F, D = obs.shape
        if labels is not None:
            for k in LOSS_KEY_ORDER:
                if labels[k].shape[1] != F:
                    raise ValueError("DiffusionLabelPredictor: labels must be 'all_frames' (one row per input frame)")
        if D != self.model.feat_dim:
            raise ValueError(f"a window row has {D} columns but the denoiser was built for feat_dim = {self.model.feat_dim}")
        if getattr(self.model, 'window', F) != F:
            raise ValueError(f"a window has {F} frames but the denoiser was built for window = {self.model.window}")
        z = torch.cat([self.sampler.draw_start(1, F, D, self.seed, draw + b) for b in range(B)])
        x = self.sampler.sample(z, obs, label_mask(F, D))
        return self.split_labels(x)
