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
from torch.autograd import Function

from . import ops

_FLOW_ONLY = "the fused census loss differentiates w.r.t. the flow only"


class TernaryLossFunction(Function):
    @staticmethod
    def forward(ctx, flow, src, tgt, mask, pad, w_ternary):
        need = ctx.needs_input_grad[0]
        out, basis = ops.census_loss_forward(src, tgt, mask, flow, pad, w_ternary, need_grad=need)
        if need:
            ctx.save_for_backward(basis, out)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_loss):
        gflow = None
        if ctx.needs_input_grad[0]:
            basis, out = ctx.saved_tensors
            gflow = ops.census_loss_backward(basis, out, grad_loss)
        return gflow, None, None, None, None, None


def ternary_loss(flow: torch.Tensor, src: torch.Tensor, tgt: torch.Tensor, mask: torch.Tensor,
                 pad: str = "border", w_ternary: float = 1.0) -> torch.Tensor:
    """``loss_photomatric(tgt, flow_warp(src, flow, pad), mask)`` with w_l1 = w_ssim = 0."""
    if src.requires_grad or tgt.requires_grad:
        raise NotImplementedError(_FLOW_ONLY)
    return TernaryLossFunction.apply(flow, src, tgt, mask.detach(), pad, float(w_ternary))


class TernaryPairFunction(Function):
    """Both directions of a with_bk scale in one launch: returns [2] losses
    (direction 0: im1 vs warp(im2, flow[:, :2]) under mask1; direction 1: im2
    vs warp(im1, flow[:, 2:]) under mask2); the gradient is [B,4,H,W]."""

    @staticmethod
    def forward(ctx, flow, im1, im2, mask1, mask2, pad, w_ternary):
        need = ctx.needs_input_grad[0]
        out, basis = ops.census_loss_pair_forward(flow, im1, im2, mask1, mask2, pad, w_ternary, need_grad=need)
        if need:
            ctx.save_for_backward(basis, out)
        return out.view(2, 2)[:, 0].clone()

    @staticmethod
    def backward(ctx, grad_losses):
        gflow = None
        if ctx.needs_input_grad[0]:
            basis, out = ctx.saved_tensors
            gflow = ops.census_loss_backward(basis, out, grad_losses)
        return gflow, None, None, None, None, None, None


def ternary_loss_pair(flow: torch.Tensor, im1: torch.Tensor, im2: torch.Tensor, mask1: torch.Tensor,
                      mask2: torch.Tensor, pad: str = "border", w_ternary: float = 1.0) -> torch.Tensor:
    """``[loss_photomatric(im1, flow_warp(im2, flow[:, :2]), mask1),
    loss_photomatric(im2, flow_warp(im1, flow[:, 2:]), mask2)]`` (flow_loss.py:130-131)
    of the census term in one launch; ``flow`` is the [B,4,H,W] forward+backward flow."""
    if im1.requires_grad or im2.requires_grad:
        raise NotImplementedError(_FLOW_ONLY)
    return TernaryPairFunction.apply(flow, im1, im2, mask1.detach(), mask2.detach(), pad, float(w_ternary))


class TernaryPyramidFunction(Function):
    """The with_bk pairs of up to 4 loss scales in one launch (the largest
    first): returns [nscale, 2] losses; the gradient w.r.t. each scale's
    [B,4,H,W] flow comes from one backward launch for all scales."""

    @staticmethod
    def forward(ctx, pad, w_ternary, n, *tensors):
        flows, im1s, im2s, m1s, m2s = (list(tensors[i * n:(i + 1) * n]) for i in range(5))
        need = any(ctx.needs_input_grad[3:3 + n])
        out, bases = ops.census_loss_pyramid_forward(flows, im1s, im2s, m1s, m2s, pad, w_ternary, need_grad=need)
        ctx.n = n
        if need:
            ctx.save_for_backward(out, *bases)
        return out[:, 0::2].clone()

    @staticmethod
    def backward(ctx, grad_losses):
        n = ctx.n
        grads = [None] * (3 + 5 * n)
        if any(ctx.needs_input_grad[3:3 + n]):
            out, *bases = ctx.saved_tensors
            gflows = ops.census_loss_pyramid_backward(bases, out, grad_losses)
            for k in range(n):
                if ctx.needs_input_grad[3 + k]:
                    grads[3 + k] = gflows[k]
        return tuple(grads)


def ternary_loss_pyramid(flows, im1s, im2s, masks1, masks2, pad: str = "border",
                         w_ternary: float = 1.0) -> torch.Tensor:
    """``[ternary_loss_pair(flows[k], im1s[k], im2s[k], masks1[k], masks2[k]) for k]``
    as [nscale, 2] from ONE forward launch and one backward launch; the same
    numbers as the per-scale calls."""
    if any(t.requires_grad for t in list(im1s) + list(im2s)):
        raise NotImplementedError(_FLOW_ONLY)
    n = len(flows)
    return TernaryPyramidFunction.apply(pad, float(w_ternary), n, *flows, *im1s, *im2s,
                                        *[m.detach() for m in masks1], *[m.detach() for m in masks2])
