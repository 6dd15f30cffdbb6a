"""Fused photometric loss: the per-scale, per-direction
``loss_photomatric(im1_s, flow_warp(im2_s, flow), vis_mask)`` of
losses/flow_loss.py:127-148 (L1 + SSIM, loss_blocks.py:53-72) as one autograd
op (unsamflow_amd/csrc/photo.hip): no warped image, SSIM maps or intermediate
gradients in HBM, and the gradient reaches only the flow (the images and the
thresholded occlusion mask carry none, as in the reference). When the flow needs
a gradient, the forward pass also writes the per-pixel gradient basis (the loss
is linear in its L1 and SSIM sums), so the backward is one dense pass.
"""
from __future__ import annotations

import torch

from . import _loss_autograd as _ag
from .ops import _PHOTO


def photometric_loss(flow: torch.Tensor, src: torch.Tensor, tgt: torch.Tensor, mask: torch.Tensor,
                     pad: str = "border", w_l1: float = 0.15, w_ssim: float = 0.85) -> torch.Tensor:
    """``loss_photomatric(tgt, flow_warp(src, flow, pad), mask)`` with w_ternary = 0."""
    return _ag.single(_PHOTO, (w_l1, w_ssim), flow, src, tgt, mask, pad)


def photometric_loss_pair(flow: torch.Tensor, im1: torch.Tensor, im2: torch.Tensor, mask1: torch.Tensor,
                          mask2: torch.Tensor, pad: str = "border", w_l1: float = 0.15,
                          w_ssim: float = 0.85) -> torch.Tensor:
    """``[loss_photomatric(im1, flow_warp(im2, flow[:, :2]), mask1),
    loss_photomatric(im2, flow_warp(im1, flow[:, 2:]), mask2)]`` (flow_loss.py:130-131)
    in one launch; ``flow`` is the [B,4,H,W] forward+backward flow."""
    return _ag.pair(_PHOTO, (w_l1, w_ssim), flow, im1, im2, mask1, mask2, pad)


def photometric_loss_pyramid(flows, im1s, im2s, masks1, masks2, pad: str = "border", w_l1: float = 0.15,
                             w_ssim: float = 0.85) -> torch.Tensor:
    """``[photometric_loss_pair(flows[k], im1s[k], im2s[k], masks1[k], masks2[k]) for k]``
    (flow_loss.py:120-148's scale loop, with_bk) as [nscale, 2] from ONE forward
    launch and one backward launch; the same numbers as the per-scale calls."""
    return _ag.pyramid(_PHOTO, (w_l1, w_ssim), flows, im1s, im2s, masks1, masks2, pad)
