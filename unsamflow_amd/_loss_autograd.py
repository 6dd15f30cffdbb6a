"""The autograd layer of the fused photometric losses (photometric.py: L1 +
SSIM, census.py: ternary): one direction, the with_bk pair of a scale, and the
pairs of up to 4 scales, each as one Function over a loss kind of ops.py and
its tuple of weights. The gradient reaches only the flow; when the flow needs
one, the forward also writes the gradient basis and the backward is one dense
pass over it.
"""
from __future__ import annotations

from torch.autograd import Function

from . import ops


def _flow_only(kind, images):
    if any(t.requires_grad for t in images):
        raise NotImplementedError(f"the fused {kind.title} loss differentiates w.r.t. the flow only")


class _Single(Function):
    @staticmethod
    def forward(ctx, flow, src, tgt, mask, kind, pad, weights):
        need = ctx.needs_input_grad[0]
        out, basis = ops._loss_forward(kind, 1, flow, src, tgt, mask, None, pad, weights, need)
        ctx.kind = kind
        if need:
            ctx.save_for_backward(basis, out)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_loss):
        gflow = None
        if ctx.needs_input_grad[0]:
            basis, out = ctx.saved_tensors
            gflow = ops._loss_backward(ctx.kind, basis, out, grad_loss)
        return (gflow,) + (None,) * 6


class _Pair(Function):
    """Both directions of a with_bk scale in one launch: returns [2] losses
    (direction 0: im1 vs warp(im2, flow[:, :2]) under mask1; direction 1: im2
    vs warp(im1, flow[:, 2:]) under mask2); the gradient is [B,4,H,W]."""

    @staticmethod
    def forward(ctx, flow, im1, im2, mask1, mask2, kind, pad, weights):
        need = ctx.needs_input_grad[0]
        out, basis = ops._loss_forward(kind, 2, flow, im1, im2, mask1, mask2, pad, weights, need)
        ctx.kind = kind
        if need:
            ctx.save_for_backward(basis, out)
        return out.view(2, kind.nout)[:, 0].clone()

    @staticmethod
    def backward(ctx, grad_losses):
        gflow = None
        if ctx.needs_input_grad[0]:
            basis, out = ctx.saved_tensors
            gflow = ops._loss_backward(ctx.kind, basis, out, grad_losses)
        return (gflow,) + (None,) * 7


class _Pyramid(Function):
    """The with_bk pairs of up to 4 loss scales in one launch (the largest
    first): returns [nscale, 2] losses; the gradient w.r.t. each scale's
    [B,4,H,W] flow comes from one backward launch for all scales."""

    @staticmethod
    def forward(ctx, kind, pad, weights, n, *tensors):
        flows, im1s, im2s, m1s, m2s = (list(tensors[i * n:(i + 1) * n]) for i in range(5))
        need = any(ctx.needs_input_grad[4:4 + n])
        out, bases = ops._loss_pyramid_forward(kind, flows, im1s, im2s, m1s, m2s, pad, weights, need)
        ctx.kind, ctx.n = kind, n
        if need:
            ctx.save_for_backward(out, *bases)
        return out[:, 0::kind.nout].clone()

    @staticmethod
    def backward(ctx, grad_losses):
        n = ctx.n
        grads = [None] * (4 + 5 * n)
        if any(ctx.needs_input_grad[4:4 + n]):
            out, *bases = ctx.saved_tensors
            gflows = ops._loss_pyramid_backward(ctx.kind, bases, out, grad_losses)
            for k in range(n):
                if ctx.needs_input_grad[4 + k]:
                    grads[4 + k] = gflows[k]
        return tuple(grads)


def single(kind, weights, flow, src, tgt, mask, pad):
    _flow_only(kind, (src, tgt))
    return _Single.apply(flow, src, tgt, mask.detach(), kind, pad, tuple(float(w) for w in weights))


def pair(kind, weights, flow, im1, im2, mask1, mask2, pad):
    _flow_only(kind, (im1, im2))
    return _Pair.apply(flow, im1, im2, mask1.detach(), mask2.detach(), kind, pad, tuple(float(w) for w in weights))


def pyramid(kind, weights, flows, im1s, im2s, masks1, masks2, pad):
    _flow_only(kind, list(im1s) + list(im2s))
    return _Pyramid.apply(kind, pad, tuple(float(w) for w in weights), len(flows), *flows, *im1s, *im2s,
                          *[m.detach() for m in masks1], *[m.detach() for m in masks2])
