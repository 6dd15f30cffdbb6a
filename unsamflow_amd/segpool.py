"""The mask-feature branch's per-segment max pool and spread (the reference's
``models/pwclite.py:317-357``, enabled by ``add_mask_corr``).

Every feature channel is max-pooled over each SAM segment and the pooled value
is written back to the segment's pixels::

    onehot = F.one_hot(seg)                                    # [B,1,h,w,K]
    pooled = torch.amax(onehot * proj[..., None], dim=(2, 3))  # [B,C,K]
    spread = (onehot * pooled[:, :, None, None, :]).sum(-1)    # [B,C,h,w]

:func:`segment_max_spread_torch` is that composition (any device; the A/B
partner of the kernels). :func:`segment_max_spread` runs it as the HIP kernels
of ``csrc/segpool.hip`` on a ROCm device: one read of ``proj`` and ``seg`` and
one write of ``spread``, with per-(sample, channel, segment) tables as the only
K-sized memory instead of two ``[B,C,h,w,K]`` products.

Because the one-hot product is 0 outside a segment, a segment that does not
cover its sample pools to ``max(m, 0)``; ``amax`` shares its gradient evenly
among all positions equal to the maximum, those zeros included.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.autograd import Function

from . import ops
from ._lib import SEGPOOL_MAX_K  # noqa: F401  (the kernels' K limit, USF_SEGPOOL_MAX_K)


def segment_max_spread_torch(proj, seg, num_segments=None):
    """The reference's three lines. ``proj`` [B,C,h,w]; ``seg`` [B,1,h,w] holding
    integer ids (any dtype) in [0, num_segments); ``num_segments=None`` takes
    ``seg.max() + 1`` (a device-to-host sync on a GPU)."""
    onehot = F.one_hot(seg.long()) if num_segments is None else F.one_hot(seg.long(), int(num_segments))
    pooled = torch.amax(onehot * proj[..., None], dim=(2, 3))  # [B,C,K]: per-segment max
    return (onehot * pooled[:, :, None, None, :]).sum(dim=-1)  # back to pixels


class SegmentMaxSpreadFunction(Function):
    @staticmethod
    def forward(ctx, proj, seg, num_segments):
        spread, state = ops.segpool_forward(proj, seg, num_segments)
        ctx.save_for_backward(proj, seg, state)
        ctx.num_segments = num_segments
        return spread

    @staticmethod
    def backward(ctx, grad_spread):
        gproj = None
        if ctx.needs_input_grad[0]:
            proj, seg, state = ctx.saved_tensors
            gproj = ops.segpool_backward(proj, seg, state, grad_spread, ctx.num_segments)
        return gproj, None, None


def _use_hip(t: torch.Tensor, fused) -> bool:
    """fp32 tensors on a ROCm device take the HIP path (a missing library is an
    error there, never a fall-back); ``fused=False`` selects the composition."""
    if fused is None:
        return t.is_cuda and t.dtype == torch.float32
    return bool(fused)


def segment_max_spread(proj, seg, num_segments=None, fused=None):
    """``spread[b,c,p] = max(proj[b,c,.] over the pixels with p's id)`` with the
    one-hot product's zero for partial segments (module docstring). ``proj``
    [B,C,h,w] in any memory layout; ``seg`` [B,1,h,w] integer ids in
    [0, num_segments) as fp32 (what the nearest resize returns) or an integer
    type. The gradient reaches ``proj`` only.

    With ``num_segments`` given the fused call does no host sync and can be
    captured into a HIP graph; ``None`` reads ``seg.max()`` back first. On the
    fused path a pixel whose id is outside [0, num_segments) or not an integer
    gets ``spread = 0`` and no gradient, and raises USF_DEVERR_SEGPOOL_BAD_ID
    (``ops.device_errors``)."""
    if not _use_hip(proj, fused):
        return segment_max_spread_torch(proj, seg, num_segments)
    if seg.requires_grad:
        raise NotImplementedError("segment ids carry no gradient")
    if num_segments is None:
        num_segments = int(seg.max()) + 1
    if seg.dtype != torch.float32:
        seg = seg.to(torch.float32)
    # the kernels read dense NCHW (TrainStep(channels_last=True) hands over NHWC strides)
    return SegmentMaxSpreadFunction.apply(proj.contiguous(), seg.contiguous(), int(num_segments))
