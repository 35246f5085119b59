"""[BUILD-DEFINED] eps-prediction loss of the diffusion wrapper: loss = mean((eps_hat - eps)^2).

One launch pair (per-block partials + fixed-order final sum) that also writes d loss/d eps_hat; the
loss value stays on the device (no host sync per step)."""
from typing import List

import torch

from .. import hip


def _as_f32_scalar(dloss: torch.Tensor) -> torch.Tensor:
    """the upstream gradient of the loss as a one-element fp32 tensor (the loss IS fp32 on the device, so this is a view)"""
    return dloss.detach().reshape(1).to(torch.float32).contiguous()


class _MSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        n = pred.numel()
        result = torch.zeros(1, dtype=torch.float32, device=pred.device)
        ws = torch.empty(hip.mse_loss_workspace_bytes(n), dtype=torch.uint8, device=pred.device)
        dpred = torch.empty_like(pred) if pred.requires_grad else None
        hip.mse_loss(pred, target, result, ws, dpred=dpred)
        ctx.dpred = dpred
        return result[0]

    @staticmethod
    def backward(ctx, dloss):
        if ctx.dpred is None:
            return None, None
        # dpred already holds 2 (pred - target) / n from the forward launch; the upstream gradient of the scalar loss is
        # a device scalar: one in-place HIP launch, no ATen arithmetic on the backward.  In place means consumed: a second
        # backward over the same graph (retain_graph=True) is refused rather than scaled twice.
        if getattr(ctx, "consumed", False):
            raise RuntimeError("eps-MSE loss: backward was already run on this graph; its gradient buffer is scaled in "
                               "place and cannot be reused (call the evaluator again for a second backward)")
        ctx.consumed = True
        return hip.scale_by_device_scalar(ctx.dpred, _as_f32_scalar(dloss)), None


class _CondMSEFn(torch.autograd.Function):
    """_MSEFn over the free columns of a conditional denoiser: the mean runs over [..., cond_cols:], the gradient is 0 on
    the conditioning columns (csrc/loss.hip, mse_partial_cond_kernel)"""

    @staticmethod
    def forward(ctx, pred, target, cond_cols):
        D = pred.shape[-1]
        rows = pred.numel() // D
        result = torch.zeros(1, dtype=torch.float32, device=pred.device)
        ws = torch.empty(hip.mse_loss_workspace_bytes(rows * D), dtype=torch.uint8, device=pred.device)
        dpred = torch.empty_like(pred) if pred.requires_grad else None
        hip.mse_loss_partial_cond(pred.view(rows, D), target, ws, cond_cols,
                                  dpred=None if dpred is None else dpred.view(rows, D))
        hip.mse_loss_finalize_cond(ws, result, rows * D, rows * (D - cond_cols))
        ctx.dpred = dpred
        return result[0]

    @staticmethod
    def backward(ctx, dloss):
        if ctx.dpred is None:
            return None, None, None
        if getattr(ctx, "consumed", False):          # the consume-once rule of _MSEFn
            raise RuntimeError("eps-MSE loss: backward was already run on this graph; its gradient buffer is scaled in "
                               "place and cannot be reused (call the evaluator again for a second backward)")
        ctx.consumed = True
        return hip.scale_by_device_scalar(ctx.dpred, _as_f32_scalar(dloss)), None, None


class DiffusionLossEvaluator:
    def __init__(self, split: str = 'train', cond_cols: int = 0):
        """cond_cols > 0: the loss of a denoiser conditioned on the first cond_cols columns of every frame -- the mean over
        the other columns only"""
        if int(cond_cols) < 0:
            raise ValueError(f"cond_cols must be >= 0, got {cond_cols}")
        self.split, self.cond_cols = split, int(cond_cols)
        self.losses: List[torch.Tensor] = []

    def __call__(self, eps_pred: torch.Tensor, eps: torch.Tensor) -> torch.Tensor:
        eps = eps.to(device=eps_pred.device, dtype=eps_pred.dtype).contiguous()
        if self.cond_cols:
            if not self.cond_cols < eps_pred.shape[-1]:
                raise ValueError(f"cond_cols must lie in [0, {eps_pred.shape[-1]}), got {self.cond_cols}")
            loss = _CondMSEFn.apply(eps_pred.contiguous(), eps, self.cond_cols)
        else:
            loss = _MSEFn.apply(eps_pred.contiguous(), eps)
        self.losses.append(loss.detach())
        return loss

    def print_report(self, reset: bool = True):
        if self.losses:
            m = float(torch.stack(self.losses).mean().cpu())
            print(f'\t[{self.split}] eps-MSE: {m}')
        else:
            m = None
        if reset:
            self.losses = []
        return m
