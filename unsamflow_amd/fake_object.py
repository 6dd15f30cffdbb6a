"""Key-object augmentation of the third pass (the reference's ``key_obj_aug``,
trainer/kitti_trainer_ar.py:192-262): objects cut out of earlier samples are
pasted into both frames, the first pass's flow and its visibility mask before
the random crop, and the step's own key objects go into a cache for later steps.

* ``add_fake_object`` is the reference's function
  (transforms/ar_transforms/oc_transforms.py:124-156) with its dict interface
  and 7-tuple, as a torch composition on any device in fp32 or fp64: it serves
  CPU tensors and is the tests' standard.
* ``ObjectCache`` is trainer/object_cache.py with the buffers on the device.
  ``count`` and the slot bookkeeping stay on the host; ``pop`` hands out slot
  indices and per-object parameters instead of gathered copies, and ``push``
  takes the loader's ``valid`` flags from the host, so neither touches the
  device's data from the host (the reference gathers 3 B objects on the host,
  copies them to the device every step and computes the mean flow from a
  device-to-host copy of the flow).
* ``paste_and_crop`` runs the K rounds and the crop: on a ROCm device one HIP
  launch over the crop window that reads the objects in place from the cache
  (unsamflow_amd/csrc/fakeobj.hip); elsewhere the composition, then the slice.

No gradient flows anywhere here: the inputs are the detached first-pass flow,
its mask and the frames.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ops
from .ar import _use_hip


def flow_warp_torch(x: torch.Tensor, flow12: torch.Tensor, pad: str = "border") -> torch.Tensor:
    """utils/warp_utils.py:97-106 with torch's own sampler (any device, fp32 or fp64)."""
    B, _, H, W = x.shape
    xs = torch.arange(W, device=x.device).view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H, device=x.device).view(1, H, 1).expand(B, H, W)
    v = torch.stack([xs, ys], 1) + flow12
    grid = torch.stack([2.0 * v[:, 0] / (W - 1) - 1.0, 2.0 * v[:, 1] / (H - 1) - 1.0], dim=-1)
    return F.grid_sample(x, grid, mode="bilinear", padding_mode=pad, align_corners=True)


def add_fake_object(input_dict: dict):
    """oc_transforms.add_fake_object: one round for a batch. Keys ``img1_tgt``,
    ``img2_tgt`` [B,3,H,W], ``flow_tgt`` [B,2,H,W], ``noc_tgt`` [B,1,H,W],
    ``img_src`` [B,3,H,W], ``obj_mask`` [B,1,H,W], ``motion`` [B,2] and
    optionally ``full_seg1_st`` / ``full_seg2_st`` [B,1,H,W] -> (img1, img2,
    full_seg1, full_seg2, flow, noc, new_obj_mask); the segment maps are None
    when their keys are absent (the trainers dropped them)."""
    img1_ot, img2_ot = input_dict["img1_tgt"], input_dict["img2_tgt"]
    full_seg1_ot, full_seg2_ot = input_dict.get("full_seg1_st"), input_dict.get("full_seg2_st")
    flow_ot, noc_ot = input_dict["flow_tgt"], input_dict["noc_tgt"]
    img, obj_mask = input_dict["img_src"], input_dict["obj_mask"]
    motion = input_dict["motion"][:, :, None, None]
    _, _, h, w = img1_ot.shape

    img1_ot = obj_mask * img + (1 - obj_mask) * img1_ot
    if full_seg1_ot is not None:
        full_seg1_ot = obj_mask * (full_seg1_ot.max() + 1) + (1 - obj_mask) * full_seg1_ot

    back = -motion.repeat(1, 1, h, w)
    new_obj_mask = flow_warp_torch(obj_mask, back, pad="zeros")
    new_img = flow_warp_torch(img, back, pad="border")
    img2_ot = new_obj_mask * new_img + (1 - new_obj_mask) * img2_ot
    if full_seg2_ot is not None:
        full_seg2_ot = new_obj_mask * (full_seg2_ot.max() + 1) + (1 - new_obj_mask) * full_seg2_ot

    flow_ot = obj_mask * motion + (1 - obj_mask) * flow_ot
    noc_ot = torch.max(noc_ot, obj_mask)
    return img1_ot, img2_ot, full_seg1_ot, full_seg2_ot, flow_ot, noc_ot, new_obj_mask


def pop_arithmetic(scale: torch.Tensor, sign: torch.Tensor, flip: torch.Tensor) -> torch.Tensor:
    """``params`` [n,4] = (sx, sy, flip, 0) of ObjectCache.pop(with_aug=True)
    from its three uniform draws (object_cache.py:35-47): the motion is scaled
    by ``(0.8 + 0.7 scale) * (-1)^(sign > 0.5)`` and, for ``flip > 0.5``, the
    object is mirrored in x and mx negated after the scaling. The factors are
    applied to the cached motion where it lives, on the device."""
    s = (scale * 0.7 + 0.8) * (-1) ** (sign > 0.5).float()
    f = flip > 0.5
    return torch.stack([torch.where(f, -s, s), s, f.float(), torch.zeros_like(s)], dim=1)


class ObjectCache:
    """trainer/object_cache.py on the device. ``cache_size`` slots of (mask
    [1,H,W], frame [3,H,W], motion [2]) live on ``device`` (None: the device of
    the first push), allocated at the first push. ``count`` and the choice of
    slots stay on the host and follow object_cache.py:51-88: fill in order while
    there is room; a partial fill plus random distinct overwrites among the
    slots filled before; random distinct overwrites once full.

    Every random draw comes from ``generator`` (a CPU generator; None: torch's
    default), for a pop in this order: ``randperm(cache_size)[:n]``, then
    ``rand(n)`` for the scale, the sign and the flip. The reference takes its
    indices from numpy's global stream (``np.random.choice``); that stream is
    not reproduced here, only the distribution (distinct uniform slots)."""

    def __init__(self, cache_size: int = 100, device=None, generator=None):
        self.cache_size = int(cache_size)
        self.device = None if device is None else torch.device(device)
        self.generator = generator
        self.count = 0
        self.obj_mask = self.img = self.motion = None

    def _init_cache(self, H: int, W: int, device) -> None:
        if self.device is None:
            self.device = torch.device(device)
        n = self.cache_size
        self.obj_mask = torch.zeros(n, 1, H, W, dtype=torch.float32, device=self.device)
        self.img = torch.zeros(n, 3, H, W, dtype=torch.float32, device=self.device)
        self.motion = torch.zeros(n, 2, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ pop --
    def pop(self, n: int, with_aug: bool = True):
        """(slots [n] int32, params [n,4] float32), both on the host, or None
        while the cache is not full. Nothing is removed and no cache byte
        changes: the mirror and the rescaling are parameters of the read."""
        if self.count < self.cache_size:
            return None
        if n > self.cache_size:
            raise ValueError(f"cannot pop {n} distinct objects from a cache of {self.cache_size}")
        slots = torch.randperm(self.cache_size, generator=self.generator)[:n].to(torch.int32)
        if with_aug:
            scale, sign, flip = (torch.rand(n, generator=self.generator) for _ in range(3))
            params = pop_arithmetic(scale, sign, flip)
        else:
            params = torch.tensor([1.0, 1.0, 0.0, 0.0]).repeat(n, 1)
        return slots, params

    def gather(self, slots: torch.Tensor, params: torch.Tensor):
        """(obj_mask [n,1,H,W], img [n,3,H,W], motion [n,2]) of a pop as the
        reference returns them: gathered copies, mirrored and rescaled."""
        idx = slots.to(device=self.device, dtype=torch.long)
        p = params.to(self.device)
        flip = (p[:, 2] != 0).view(-1, 1, 1, 1)
        mask, img = self.obj_mask[idx], self.img[idx]
        mask = torch.where(flip, mask.flip(dims=[3]), mask)
        img = torch.where(flip, img.flip(dims=[3]), img)
        return mask, img, self.motion[idx] * p[:, :2]

    def pop_tensors(self, n: int, with_aug: bool = True):
        """The reference's ``pop``: (obj_mask, img, motion) or None."""
        out = self.pop(n, with_aug)
        return None if out is None else self.gather(*out)

    # ----------------------------------------------------------------- push --
    def _choose_slots(self, B: int) -> list[int]:
        """Slots of the next B objects (object_cache.py:63-88); advances ``count``."""
        n, c = self.cache_size, self.count
        if c <= n - B:
            slots = list(range(c, c + B))
            self.count += B
        elif c < n:
            space = n - c
            over = torch.randperm(c, generator=self.generator)[:B - space]
            slots = list(range(c, n)) + [int(v) for v in over]
            self.count = n
        else:
            slots = [int(v) for v in torch.randperm(n, generator=self.generator)[:B]]
        return slots

    def push(self, obj_mask: torch.Tensor, img: torch.Tensor, flow: torch.Tensor, valid=None, fused=None) -> None:
        """Store the valid samples' (obj_mask [B,1,H,W], img [B,3,H,W]) with the
        masked mean of ``flow`` [B,2,H,W] as their motion. ``valid`` is a host
        bool tensor [B]: what the loader knows and the reference encodes as a
        NaN placeholder mask. Without it a CPU mask is tested for that marker;
        a device mask is refused (reading it would be a sync)."""
        B = obj_mask.shape[0]
        if valid is None:
            if obj_mask.device.type != "cpu":
                raise ValueError("ObjectCache.push: pass `valid` (a host bool tensor) with a device mask; deriving it "
                                 "from the mask would synchronise the device")
            valid = ~torch.isnan(obj_mask[:, 0, 0, 0])
        valid = torch.as_tensor(valid)
        if valid.device.type != "cpu" or valid.dtype != torch.bool or tuple(valid.shape) != (B,):
            raise ValueError(f"valid must be a host bool tensor of shape {(B,)}")
        keep = [b for b in range(B) if bool(valid[b])]
        if len(keep) > self.cache_size:
            raise ValueError(f"{len(keep)} objects pushed into a cache of {self.cache_size}")
        if not keep:
            return
        if self.obj_mask is None:
            self._init_cache(*img.shape[-2:], img.device)
        slots = torch.full((B,), -1, dtype=torch.int32)
        slots[keep] = torch.tensor(self._choose_slots(len(keep)), dtype=torch.int32)
        with torch.no_grad():
            if _use_hip(img, fused):
                ops.fakeobj_push(obj_mask, img, flow, slots.to(self.device, non_blocking=True), self.obj_mask,
                                 self.img, self.motion)
                return
            idx = slots[keep].to(device=self.device, dtype=torch.long)
            k = torch.tensor(keep, device=obj_mask.device)
            m = obj_mask[k].to(self.device)
            self.obj_mask[idx] = m
            self.img[idx] = img[k].to(self.device)
            f = flow[k].to(self.device)
            self.motion[idx] = (f * m).sum(dim=[2, 3]) / m.sum(dim=[2, 3])


def paste_and_crop_torch(img1, img2, flow, noc, obj_mask, img_src, motion, crop_sz, offsets):
    """K = n / B rounds of :func:`add_fake_object` on gathered objects (object
    k B + b goes to sample b in round k), then the crop window -> (imgs_ot
    [B,6,ch,cw], flow_ot, noc_ot, new_obj_mask of the last round, uncropped)."""
    B = img1.shape[0]
    new_mask = None
    for k in range(obj_mask.shape[0] // B):
        r = slice(k * B, (k + 1) * B)
        img1, img2, _, _, flow, noc, new_mask = add_fake_object({
            "img1_tgt": img1, "img2_tgt": img2, "flow_tgt": flow, "noc_tgt": noc, "img_src": img_src[r],
            "obj_mask": obj_mask[r], "motion": motion[r]})
    (ch, cw), (y0, x0) = crop_sz, offsets
    win = (slice(None), slice(None), slice(y0, y0 + ch), slice(x0, x0 + cw))
    return torch.cat([img1, img2], 1)[win], flow[win], noc[win], new_mask


def paste_and_crop(img1, img2, flow, noc, cache: ObjectCache, slots, params, crop_sz, offsets, fused=None):
    """The third pass's inputs with ``len(slots) / B`` rounds of cached objects
    pasted in: (imgs_ot [B,6,ch,cw], flow_ot [B,2,ch,cw], noc_ot [B,1,ch,cw]),
    the window ``crop_sz`` = (ch, cw) at ``offsets`` = (y0, x0) of the pasted
    full-size tensors. ``slots`` / ``params`` are a pop's host tables. fp32
    tensors on a ROCm device take the fused kernel (a missing library is an
    error there, never a fall-back); ``fused=False`` selects the composition."""
    with torch.no_grad():
        if _use_hip(img1, fused):
            dev = img1.device
            return ops.fakeobj_paste_crop(img1, img2, flow, noc, cache.obj_mask, cache.img, cache.motion,
                                          slots.to(dev, non_blocking=True), params.to(dev, non_blocking=True),
                                          crop_sz, offsets)
        mask, src, motion = cache.gather(slots, params)
        dt = img1.dtype
        return paste_and_crop_torch(img1, img2, flow, noc, mask.to(dt), src.to(dt), motion.to(dt), crop_sz,
                                    offsets)[:3]
