"""The stage-1 "augmentation as regularisation" branch (ARFlow) of the
reference's trainers (trainer/kitti_trainer_ar.py:137-249): the random affine
transform of both frames, the first pass's flow and its visibility mask
(transforms/ar_transforms/sp_transforms.py ``RandomAffineFlow`` with
interpolation.py ``Interp2``), the AR loss of the second and third pass, and the
third pass's random crop (oc_transforms.random_crop).

On a ROCm device the transform is one HIP launch and the loss one forward and
one backward pass (unsamflow_amd/csrc/ar.hip). The torch composition of the same
formulas (``spatial_transform_torch``, ``ar_loss_torch``) runs in fp32 and fp64
on any device: it serves CPU tensors and is the tests' standard.

The thetas are sampled on the host (``sample_thetas``): the reference's
rejection loop ``while invalid.sum() > 0`` is a device sync per round; here the
caller copies 48 B per sample to the device instead.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd import Function

from . import ops

_XBOUNDS = (-1.0, -1.0, 1.0, 1.0)
_YBOUNDS = (-1.0, 1.0, -1.0, 1.0)


# ------------------------------------------------------------------ thetas --
def _compose(theta0: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """apply_transform_to_params (sp_transforms.py:23-46)."""
    a1, a2, a3, a4, a5, a6 = theta0.unbind(1)
    b1, b2, b3, b4, b5, b6 = t.unbind(1)
    return torch.stack([a1 * b1 + a4 * b2, a2 * b1 + a5 * b2, b3 + a3 * b1 + a6 * b2,
                        a1 * b4 + a4 * b5, a2 * b4 + a5 * b5, b6 + a3 * b4 + a6 * b5], dim=1)


def find_invalid(thetas: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """[N,1] bool: a corner of the output samples outside the source
    (RandomAffineFlow.find_invalid, sp_transforms.py:175-202)."""
    x = thetas.new_tensor(_XBOUNDS)
    y = thetas.new_tensor(_YBOUNDS)
    a1, a2, a3, a4, a5, a6 = (thetas[:, k:k + 1] for k in range(6))
    z = a1 * a5 - a2 * a4
    b1, b2, b4, b5 = a5 / z, -a2 / z, -a4 / z, a1 / z
    xhat, yhat = x - a3, y - a6
    xq = 0.5 * (W - 1.0) * ((b1 * xhat + b2 * yhat) + 1.0)
    yq = 0.5 * (H - 1.0) * ((b4 * xhat + b5 * yhat) + 1.0)
    return ((xq < 0) | (yq < 0) | (xq >= W) | (yq >= H)).sum(dim=1, keepdim=True) > 0


def _random_params(theta0, max_translate, zoom, squeeze, rotate, H, W, generator):
    """apply_random_transforms_to_params (sp_transforms.py:204-258): the same
    draws in the same order (zoom, squeeze, tx, ty, phi per round, [B,1] each)."""
    max_translate = max_translate * 0.5
    B = theta0.size(0)
    thetas = torch.zeros_like(theta0)
    draw = [torch.zeros(B, 1) for _ in range(5)]
    invalid = torch.ones(B, 1, dtype=torch.bool)
    ranges = [zoom, squeeze, (-max_translate, max_translate), (-max_translate, max_translate), rotate]
    while bool(invalid.any()):
        for t, (lo, hi) in zip(draw, ranges):
            t.uniform_(lo, hi, generator=generator)
        zm, sq, tx, ty, phi = draw
        sx, sy = zm * sq, zm / sq
        sin_phi, cos_phi = torch.sin(phi), torch.cos(phi)
        t = torch.cat([cos_phi * sx, sin_phi * sy, tx, -sin_phi * sx, cos_phi * sy, ty], dim=1)
        f = invalid.float()
        thetas = f * _compose(theta0, t) + (1 - f) * thetas
        invalid = find_invalid(thetas, H, W)
    return thetas


def sample_thetas(st_cfg, B: int, H: int, W: int, n_frames: int = 2, generator=None) -> torch.Tensor:
    """[n_frames, B, 6] float32 on the CPU: the global transform, then each
    frame's transform relative to the previous one, each resampled until no
    output corner leaves the source, then the random mirror
    (RandomAffineFlow.forward, sp_transforms.py:299-336). The draws come from
    torch's CPU generator (``generator`` or the default one) in the
    reference's order, so under one seed these are the reference's thetas."""
    theta0 = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]).repeat(B, 1)
    lst = [_random_params(theta0, st_cfg.trans[0], st_cfg.zoom[0:2], st_cfg.squeeze[0:2], st_cfg.rotate[0:2],
                          H, W, generator)]
    for _ in range(n_frames - 1):
        lst.append(_random_params(lst[-1], st_cfg.trans[1], st_cfg.zoom[2:4], st_cfg.squeeze[2:4],
                                  st_cfg.rotate[2:4], H, W, generator))
    # RandomMirror(cfg.vflip) if cfg.hflip else RandomMirror(p=1): the latter still draws (and never flips)
    p, vertical = (0.5, bool(st_cfg.vflip)) if st_cfg.hflip else (1.0, True)
    probs = torch.full((B, 1), p)
    one = torch.ones(B, 1)
    sign = torch.sign(2.0 * torch.bernoulli(probs, generator=generator) - 1.0)
    mirror = torch.cat([sign, sign, sign, one, one, one], dim=1)
    lst = [t * mirror for t in lst]
    if vertical:
        sign = torch.sign(2.0 * torch.bernoulli(probs, generator=generator) - 1.0)
        mirror = torch.cat([one, one, one, sign, sign, sign], dim=1)
        lst = [t * mirror for t in lst]
    return torch.stack(lst)


# --------------------------------------------------------------- transform --
def _grid(H: int, W: int, like: torch.Tensor):
    ys = torch.arange(H, device=like.device, dtype=like.dtype).view(1, H, 1).expand(1, H, W)
    xs = torch.arange(W, device=like.device, dtype=like.dtype).view(1, 1, W).expand(1, H, W)
    return xs, ys


def _coef(theta: torch.Tensor):
    return (theta[:, k].reshape(-1, 1, 1) for k in range(6))


def transform_coords(theta: torch.Tensor, H: int, W: int):
    """Source coordinates (xq, yq) [B,H,W] of every output pixel
    (RandomAffineFlow.transform_coords, sp_transforms.py:147-173)."""
    xs, ys = _grid(H, W, theta)
    xx = (2.0 / (W - 1.0)) * xs - 1.0
    yy = (2.0 / (H - 1.0)) * ys - 1.0
    a1, a2, a3, a4, a5, a6 = _coef(theta)
    z = a1 * a5 - a2 * a4
    b1, b2, b4, b5 = a5 / z, -a2 / z, -a4 / z, a1 / z
    xhat, yhat = xx - a3, yy - a6
    xq = 0.5 * (W - 1.0) * ((b1 * xhat + b2 * yhat) + 1.0)
    yq = 0.5 * (H - 1.0) * ((b4 * xhat + b5 * yhat) + 1.0)
    return xq, yq


def forward_coords(theta: torch.Tensor, xs: torch.Tensor, ys: torch.Tensor, H: int, W: int):
    """Tk of pixel positions (xs, ys) (inverse_transform_coords, sp_transforms.py:121-145)."""
    xx = (2.0 / (W - 1.0)) * xs - 1.0
    yy = (2.0 / (H - 1.0)) * ys - 1.0
    a1, a2, a3, a4, a5, a6 = _coef(theta)
    xq = 0.5 * (W - 1.0) * ((a1 * xx + a2 * yy + a3) + 1.0)
    yq = 0.5 * (H - 1.0) * ((a4 * xx + a5 * yy + a6) + 1.0)
    return xq, yq


def interp2(v: torch.Tensor, xq: torch.Tensor, yq: torch.Tensor) -> torch.Tensor:
    """Interp2(clamp=False) (interpolation.py:80-149): taps clamped into the
    image, fractions from the clamped tap, 0 where (xq, yq) lies outside."""
    B, C, H, W = v.shape
    x0 = torch.floor(xq).long().clamp(0, W - 1)
    y0 = torch.floor(yq).long().clamp(0, H - 1)
    x1 = (x0 + 1).clamp(0, W - 1)
    y1 = (y0 + 1).clamp(0, H - 1)
    flat = v.reshape(B, C, H * W)

    def tap(yi, xi):
        idx = (yi * W + xi).view(B, 1, H * W).expand(B, C, H * W)
        return flat.gather(2, idx).view(B, C, H, W)

    fx = (xq - x0.to(v.dtype)).unsqueeze(1)
    fy = (yq - y0.to(v.dtype)).unsqueeze(1)
    values = (tap(y0, x0) * ((1.0 - fy) * (1.0 - fx)) + tap(y0, x1) * ((1.0 - fy) * fx)
              + tap(y1, x0) * (fy * (1.0 - fx)) + tap(y1, x1) * (fy * fx))
    invalid = ((xq < 0) | (xq >= W) | (yq < 0) | (yq >= H)).unsqueeze(1)
    return torch.where(invalid, torch.zeros_like(values), values)


def transform_image(img: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
    H, W = img.shape[-2:]
    return interp2(img, *transform_coords(theta.to(img.dtype), H, W))


def transform_flow(flow: torch.Tensor, theta1: torch.Tensor, theta2: torch.Tensor) -> torch.Tensor:
    """transform_flow (sp_transforms.py:266-290): the flow re-expressed between
    the two transformed frames, sampled at theta1's coordinates."""
    H, W = flow.shape[-2:]
    theta1, theta2 = theta1.to(flow.dtype), theta2.to(flow.dtype)
    xs, ys = _grid(H, W, flow)
    x0, y0 = forward_coords(theta1, xs, ys, H, W)
    x1, y1 = forward_coords(theta2, xs + flow[:, 0], ys + flow[:, 1], H, W)
    new_flow = torch.stack([x1 - x0, y1 - y0], dim=1)
    return interp2(new_flow, *transform_coords(theta1, H, W))


def spatial_transform_torch(img1, img2, flow, mask, thetas, noise1=None, noise2=None):
    """The torch composition of :func:`spatial_transform` (any device, fp32 or fp64)."""
    thetas = thetas.to(img1.device)
    out1, out2 = transform_image(img1, thetas[0]), transform_image(img2, thetas[1])
    if noise1 is not None:
        out1 = (out1 + noise1).clamp(0.0, 1.0)
    if noise2 is not None:
        out2 = (out2 + noise2).clamp(0.0, 1.0)
    return out1, out2, transform_flow(flow, thetas[0], thetas[1]), transform_image(mask, thetas[0])


def _use_hip(t: torch.Tensor, fused) -> bool:
    """fp32 tensors on a ROCm device take the HIP path (a missing library is an
    error there, never a fall-back); ``fused=False`` selects the composition."""
    if fused is None:
        return t.is_cuda and t.dtype == torch.float32
    return bool(fused)


def spatial_transform(img1, img2, flow, mask, thetas, noise1=None, noise2=None, fused=None):
    """(img1_t, img2_t, flow_t, mask_t): both frames [B,3,H,W], the flow
    [B,2,H,W] between them and a mask [B,1,H,W] under the per-sample affine maps
    ``thetas`` [2,B,6] (frame 1, frame 2); ``noise*`` (already scaled) is added
    to the transformed frames, which are then clamped to [0, 1]. No gradient."""
    with torch.no_grad():
        if _use_hip(img1, fused):
            th = thetas.to(device=img1.device, dtype=torch.float32, non_blocking=True)
            return ops.ar_transform(img1, img2, flow, mask, th, noise1, noise2)
        return spatial_transform_torch(img1, img2, flow, mask, thetas, noise1, noise2)


class RandomAffineFlow(nn.Module):
    """The reference's module (sp_transforms.py:101-370) with its dict
    interface: ``data["imgs"]``, ``["flows_f"]``, ``["masks_f"]`` and optionally
    ``["full_segs"]`` are lists of tensors, replaced by their transformed
    versions. Two frames with one flow, one mask and no segment maps take the
    fused path; anything else the torch composition. The thetas and the noise's
    standard deviation (U[0, 0.04)) come from ``generator`` (a CPU generator;
    None: torch's default); the noise itself is drawn on the frames' device."""

    def __init__(self, st_cfg, addnoise: bool = True, generator=None, fused=None):
        super().__init__()
        self.cfg = st_cfg
        self._addnoise = addnoise
        self.generator = generator
        self.fused = fused
        self._noise_gen = {}

    def _noise(self, like: torch.Tensor, std: float) -> torch.Tensor:
        g = self._noise_gen.get(like.device)
        if g is None:  # seeded from the host generator, so a seed fixes the whole step
            seed = int(torch.randint(0, 2 ** 31 - 1, (), generator=self.generator))
            g = self._noise_gen[like.device] = torch.Generator(device=like.device).manual_seed(seed)
        return torch.randn(like.shape, device=like.device, dtype=like.dtype, generator=g) * std

    def forward(self, data: dict) -> dict:
        imgs, flows, masks = list(data["imgs"]), list(data["flows_f"]), list(data["masks_f"])
        segs = list(data.get("full_segs") or [])
        B, _, H, W = imgs[0].shape
        thetas = sample_thetas(self.cfg, B, H, W, n_frames=len(imgs), generator=self.generator)
        std = float(torch.rand((), generator=self.generator)) * 0.04 if self._addnoise else 0.0
        with torch.no_grad():
            noise = [self._noise(im, std) for im in imgs] if self._addnoise else [None] * len(imgs)
            if len(imgs) == 2 and len(flows) == 1 and len(masks) == 1 and not segs:
                im1, im2, fl, mk = spatial_transform(imgs[0], imgs[1], flows[0], masks[0], thetas, noise[0],
                                                     noise[1], fused=self.fused)
                imgs, flows, masks = [im1, im2], [fl], [mk]
            else:
                th = list(thetas.to(imgs[0].device))
                imgs = [transform_image(im, t) for im, t in zip(imgs, th)]
                segs = [transform_image(s, t) for s, t in zip(segs, th)]
                if len(imgs) > 2:
                    th = th[1:-1]
                flows = [transform_flow(f, t1, t2) for f, t1, t2 in zip(flows, th[:-1], th[1:])]
                masks = [transform_image(m, t) for m, t in zip(masks, th)]
                if self._addnoise:
                    imgs = [(im + n).clamp(0.0, 1.0) for im, n in zip(imgs, noise)]
        data["imgs"], data["flows_f"], data["masks_f"] = imgs, flows, masks
        if "full_segs" in data:
            data["full_segs"] = segs
        return data


# ----------------------------------------------------------------- AR loss --
def ar_loss_torch(pred, target, noc, eps: float = 0.0, q: float = 1.0, denom=None):
    """``(((pred - target).abs() + eps) ** q * noc).mean() / (D + 1e-7)``, D =
    ``noc.mean()`` or ``denom`` (kitti_trainer_ar.py:169-172; the Sintel
    trainer's l_ot divides by the transformed mask's mean)."""
    l = ((pred - target).abs() + eps) ** q
    d = noc.mean() if denom is None else denom
    return (l * noc).mean() / (d + 1e-7)


class ARLossFunction(Function):
    @staticmethod
    def forward(ctx, pred, target, noc, eps, q, denom):
        out = ops.ar_loss_forward(pred, target, noc, eps, q, denom)
        ctx.save_for_backward(pred, target, noc, out)
        ctx.eps, ctx.q = eps, q
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_loss):
        gpred = None
        if ctx.needs_input_grad[0]:
            pred, target, noc, out = ctx.saved_tensors
            gpred = ops.ar_loss_backward(pred, target, noc, out, grad_loss, ctx.eps, ctx.q)
        return gpred, None, None, None, None, None


def ar_loss(pred, target, noc, eps: float = 0.0, q: float = 1.0, denom=None, fused=None):
    """The AR loss of a pass: ``pred`` [B,2,H,W] against the transformed (or
    cropped) first-pass flow ``target`` under the mask ``noc`` [B,1,H,W]. The
    gradient reaches ``pred`` only. ``target`` and ``noc`` may be crop views
    (unit column stride): the fused path reads them in place."""
    if target.requires_grad or noc.requires_grad or (isinstance(denom, torch.Tensor) and denom.requires_grad):
        raise NotImplementedError("the AR loss differentiates w.r.t. the prediction only")
    if not _use_hip(pred, fused):
        return ar_loss_torch(pred, target, noc, eps, q, denom)
    if target.stride(-1) != 1:
        target = target.contiguous()
    if noc.stride(-1) != 1:
        noc = noc.contiguous()
    if denom is not None and not isinstance(denom, torch.Tensor):
        denom = torch.full((1,), float(denom), device=pred.device, dtype=torch.float32)
    return ARLossFunction.apply(pred, target, noc, float(eps), float(q), denom)


def crop_offsets(h: int, w: int, crop_sz, generator=None) -> tuple[int, int]:
    """(y1, x1) of oc_transforms.random_crop's window: x is drawn first, then y,
    each from ``randint(0, size - crop)``; a dimension equal to the crop draws
    nothing and gives 0."""
    c_h, c_w = crop_sz
    if c_h > h or c_w > w:
        raise ValueError(f"crop {(c_h, c_w)} larger than the image {(h, w)}")
    x1 = int(torch.randint(0, w - c_w, (), generator=generator)) if w > c_w else 0
    y1 = int(torch.randint(0, h - c_h, (), generator=generator)) if h > c_h else 0
    return y1, x1


def random_crop(imgs, flow, noc, crop_sz, generator=None):
    """oc_transforms.random_crop as the trainers call it (three tensors): one
    random window of ``crop_sz`` = (h, w) as views of all three. The offsets (x
    first, then y, as the reference draws them) come from ``generator``; a
    dimension equal to the crop gives offset 0."""
    h, w = imgs.shape[-2:]
    c_h, c_w = crop_sz
    y1, x1 = crop_offsets(h, w, crop_sz, generator)
    if c_h == h and c_w == w:
        return imgs, flow, noc
    win = (slice(None), slice(None), slice(y1, y1 + c_h), slice(x1, x1 + c_w))
    return imgs[win], flow[win], noc[win]
