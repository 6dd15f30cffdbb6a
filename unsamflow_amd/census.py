"""Fused ternary (census) photometric loss: the per-scale, per-direction
``w_ternary * TernaryLoss(flow_warp(im2_s, flow) * vis, im1_s * vis).mean() /
(vis.mean() + 1e-6)`` of losses/flow_loss.py:33-50, 127-148 (TernaryLoss:
loss_blocks.py:12-50) as one autograd op (unsamflow_amd/csrc/census.hip) -- the
reference's stage-1 loss (configs/*_base.json ``train.stage1.loss``). No warped
image, census maps or intermediate gradients in HBM, and the gradient reaches
only the flow (the images and the thresholded occlusion mask carry none, as in
the reference). When the flow needs a gradient the forward pass also writes the
per-pixel gradient basis (the loss is linear in its census sum), so the
backward is one dense pass.
"""
from __future__ import annotations

import torch

from . import _loss_autograd as _ag
from .ops import _CENSUS


def ternary_loss(flow: torch.Tensor, src: torch.Tensor, tgt: torch.Tensor, mask: torch.Tensor,
                 pad: str = "border", w_ternary: float = 1.0) -> torch.Tensor:
    """``loss_photomatric(tgt, flow_warp(src, flow, pad), mask)`` with w_l1 = w_ssim = 0."""
    return _ag.single(_CENSUS, (w_ternary,), flow, src, tgt, mask, pad)


def ternary_loss_pair(flow: torch.Tensor, im1: torch.Tensor, im2: torch.Tensor, mask1: torch.Tensor,
                      mask2: torch.Tensor, pad: str = "border", w_ternary: float = 1.0) -> torch.Tensor:
    """``[loss_photomatric(im1, flow_warp(im2, flow[:, :2]), mask1),
    loss_photomatric(im2, flow_warp(im1, flow[:, 2:]), mask2)]`` (flow_loss.py:130-131)
    of the census term in one launch; ``flow`` is the [B,4,H,W] forward+backward flow."""
    return _ag.pair(_CENSUS, (w_ternary,), flow, im1, im2, mask1, mask2, pad)


def ternary_loss_pyramid(flows, im1s, im2s, masks1, masks2, pad: str = "border",
                         w_ternary: float = 1.0) -> torch.Tensor:
    """``[ternary_loss_pair(flows[k], im1s[k], im2s[k], masks1[k], masks2[k]) for k]``
    as [nscale, 2] from ONE forward launch and one backward launch; the same
    numbers as the per-scale calls."""
    return _ag.pyramid(_CENSUS, (w_ternary,), flows, im1s, im2s, masks1, masks2, pad)
