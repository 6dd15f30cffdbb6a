"""A convolution's bias add and LeakyReLU as one in-place HIP pass
(``csrc/convepi.hip``), and their backward with the bias gradient summed on
the way.

``conv_block`` (pwclite.py) is ``Conv2d(bias=True)[, LeakyReLU(0.1, inplace)]``.
As torch runs it every convolution is followed by a broadcast add, an in-place
activation, the activation's backward and an ``at::sum`` over (N, H, W) for the
bias gradient: four passes over the conv's output that the result does not
need as passes of their own. :func:`bias_act_` takes the output of the same
convolution run WITHOUT its bias and does the rest in place, bit-identical in
the forward and in the input gradient; the bias gradient differs from
``at::sum`` by the summation order only (deterministic here).
"""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops


class ConvEpilogueFunction(Function):
    @staticmethod
    def forward(ctx, raw, bias, slope):
        ops.conv_epilogue_forward(raw, bias, slope)
        ctx.mark_dirty(raw)
        ctx.slope = float(slope)
        if ctx.slope != 1.0:
            ctx.save_for_backward(raw)  # the sign of y is the sign of the pre-activation (slope > 0)
        return raw

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        y = ctx.saved_tensors[0] if ctx.slope != 1.0 else None
        need_in, need_bias = ctx.needs_input_grad[:2]
        if not need_in and not need_bias:
            return None, None, None
        gin, gbias = ops.conv_epilogue_backward(grad_out, y, ctx.slope, need_bias=need_bias)
        return (gin if need_in else None), gbias, None


def bias_act_(raw: torch.Tensor, bias: torch.Tensor, slope: float = 1.0) -> torch.Tensor:
    """``raw = leaky_relu(raw + bias[None, :, None, None], slope)`` in place and
    differentiable; ``slope == 1`` is the bias add alone. ``raw``: a dense fp32
    NCHW tensor on a ROCm device that nothing else needs unmodified (a bias-free
    convolution's output); ``slope > 0``."""
    return ConvEpilogueFunction.apply(raw, bias, slope)
