"""Training-step harness around the hot path (the benchmark's "step").

Reproduces the shape of the reference's training step
(trainer/kitti_trainer_ar.py:108-317 with trainer/base_trainer.py:141-169):

    res = model(img1, img2, with_bk=True)
    flows = [cat(f12, f21)]                       # :113-117
    loss = unFlowLoss(flows, img1, img2).mean()   # :127-133
    optimizer.zero_grad(set_to_none=True); loss.backward()          # :309-310
    clip_grad_norm_(params, max_grad_norm); optimizer.step(); scheduler.step()  # :313-317

with Adam(betas=(momentum, beta), eps=1e-7) over the bias / weight parameter
groups (base_trainer.py:141-169) and OneCycleLR. Data is synthetic (U[0,1)
frames, as ``/255`` images of datasets/flow_datasets.py:59-63). With
``ddp=True`` the model is wrapped in DistributedDataParallel (train.py:116-120):
one process per GPU, gradient all-reduce over RCCL ("nccl" backend) / gloo.

With ``cfg.train.run_atst`` / ``run_ot`` (config.*_stage1_ar(), the reference's
epochs 50-200) the step adds the ARFlow branch of kitti_trainer_ar.py:137-249:
the detached first-pass flow and its visibility mask are transformed by random
affine maps together with the frames (unsamflow_amd.ar), a second pass
(with_bk=False) on the transformed frames is held to the transformed flow by
the AR loss, and a third pass does the same on a random crop. With
``cfg.train.key_obj_aug`` (config.*_aug(), *_aug_hg(), the reference's epochs
150-200) the third pass's inputs first get ``key_obj_count`` rounds of objects
from a device-resident cache pasted in, and the step's own key objects are
pushed into that cache (unsamflow_amd.fake_object, kitti_trainer_ar.py:192-262).

The per-step host syncs of the reference's logging (``loss.item()``,
kitti_trainer_ar.py:284-293) are not part of the step.
"""
from __future__ import annotations

from typing import Callable

import torch

from .flow_loss import unFlowLoss
from .pwclite import PWCLite


def param_groups(model: torch.nn.Module, train_cfg) -> list[dict]:
    """Bias / weight / other groups as utils/torch_utils.py:27-40 (empty groups dropped)."""
    named = list(model.named_parameters())
    groups = [
        {"params": [p for n, p in named if ".bias" in n], "weight_decay": train_cfg.bias_decay},
        {"params": [p for n, p in named if ".weight" in n], "weight_decay": train_cfg.weight_decay},
        {"params": [p for n, p in named if ".bias" not in n and ".weight" not in n], "weight_decay": 0},
    ]
    return [g for g in groups if g["params"]]


def synthetic_pair(B: int, H: int, W: int, device, seed: int = 42, with_seg: bool = False, n_seg: int = 32):
    """U[0,1) frame pair [B,3,H,W] (+ piecewise-constant segment maps [B,1,H,W] as float)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    img1 = torch.rand(B, 3, H, W, generator=g).to(device)
    img2 = torch.rand(B, 3, H, W, generator=g).to(device)
    if not with_seg:
        return img1, img2, None, None
    blk = 32
    segs = []
    for _ in range(2):
        ids = torch.randint(0, n_seg, (B, 1, (H + blk - 1) // blk, (W + blk - 1) // blk), generator=g).float()
        seg = ids.repeat_interleave(blk, 2).repeat_interleave(blk, 3)[:, :, :H, :W]
        segs.append(seg.contiguous().to(device))
    return img1, img2, segs[0], segs[1]


def synthetic_key_objects(B: int, H: int, W: int, device, seed: int = 42, p_invalid: float = 0.25):
    """Key-object masks as the loader hands them over: (mask [B,1,H,W] float,
    valid [B] host bool). A valid sample holds one binary ellipse or rectangle
    lying inside the image, of half-sizes H/8..H/4 by W/10..W/5 (an ellipse of
    the smallest covers 3.9 % of the image, above the loader's 0.5 % floor); an
    invalid one holds the reference's NaN placeholder."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    valid = torch.rand(B, generator=g) >= p_invalid
    ys = torch.arange(H, dtype=torch.float32).view(H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, W)
    mask = torch.full((B, 1, H, W), float("nan"))
    for b in range(B):
        u = torch.rand(5, generator=g)
        ry = max(1.0, float(H / 8 + u[0] * H / 8))
        rx = max(1.0, float(W / 10 + u[1] * W / 10))
        cy = ry + float(u[2]) * max(0.0, H - 1 - 2 * ry)
        cx = rx + float(u[3]) * max(0.0, W - 1 - 2 * rx)
        dy, dx = (ys - cy).abs() / ry, (xs - cx).abs() / rx
        inside = (dy * dy + dx * dx <= 1.0) if float(u[4]) < 0.5 else ((dy <= 1.0) & (dx <= 1.0))
        if bool(valid[b]):
            mask[b, 0] = inside.float()
    return mask.to(device), valid


class TrainStep:
    """One PWCLite fwd(with_bk) + unFlowLoss + bwd + clip + Adam + OneCycleLR step."""

    def __init__(self, cfg, device, ddp: bool = False, corr_module=None, warp_fn: Callable | None = None,
                 loss_kwargs: dict | None = None, fused_adam: bool | None = None, seed: int = 42,
                 channels_last: bool = False, occ_backward_fn: Callable | None = None,
                 capturable: bool = False, fused_ar: bool = True, fused_fake_object: bool = True,
                 obj_cache_size: int = 100):
        torch.manual_seed(seed)
        self.cfg = cfg
        self.device = torch.device(device)
        model = PWCLite(cfg.model, corr_module=corr_module, warp_fn=warp_fn).to(self.device)
        if channels_last:  # NHWC weights/activations for MIOpen's NHWC convolutions
            model = model.to(memory_format=torch.channels_last)
        self.module = model
        if ddp:
            ids = [self.device.index] if self.device.type == "cuda" else None
            model = torch.nn.parallel.DistributedDataParallel(model, device_ids=ids)
        self.model = model
        self.loss_fn = unFlowLoss(cfg.loss, warp_fn=warp_fn, occ_backward_fn=occ_backward_fn,
                                  **(loss_kwargs or {}))
        t = cfg.train
        if fused_adam is None:
            fused_adam = self.device.type == "cuda"
        # capturable: the step counters and the learning rate live on the device
        # (the scheduler fills the lr tensor in place), so the step can be
        # captured into a HIP graph (GraphedTrainStep)
        lr = torch.tensor(float(t.lr), device=self.device) if capturable else t.lr
        self.optimizer = torch.optim.Adam(param_groups(self.module, t), lr, betas=(t.momentum, t.beta), eps=1e-7,
                                          fused=fused_adam or None, capturable=capturable)
        sched = t.get("lr_scheduler")
        if sched and sched.module == "OneCycleLR":
            p = dict(sched.params)
            p.update(epochs=t.epoch_num, steps_per_epoch=t.epoch_size)
            self.scheduler = torch.optim.lr_scheduler.OneCycleLR(self.optimizer, **p)
        else:
            self.scheduler = torch.optim.lr_scheduler.ExponentialLR(self.optimizer, gamma=1)
        self.max_grad_norm = t.max_grad_norm
        # None, or a list that every call appends one (start, after backward, end)
        # triple of device events to: the optimizer step (clip + Adam + scheduler)
        # timed apart from fwd + loss + bwd (bench.py)
        self.phase_events: list | None = None
        # the stage-1 augmentation branch (kitti_trainer_ar.py:137-249): off for every config without the keys
        self.run_atst = bool(t.get("run_atst", False))
        self.run_ot = bool(t.get("run_ot", False))
        self.has_ar = self.run_atst or self.run_ot
        self.l_atst = self.l_ot = None  # the last step's terms (detached)
        if self.has_ar:
            from .ar import RandomAffineFlow

            # fused_ar: the HIP transform and loss on a ROCm device (the torch composition elsewhere);
            # False: the torch composition everywhere
            self.fused_ar = None if fused_ar else False
            # thetas, crop offsets and the noise's std: one seeded host generator owned by the step
            self.ar_generator = torch.Generator(device="cpu").manual_seed(seed)
            self.sp_transform = RandomAffineFlow(t.st_cfg, addnoise=t.st_cfg.add_noise,
                                                 generator=self.ar_generator, fused=self.fused_ar)
        # the key-object augmentation of the third pass (kitti_trainer_ar.py:192-262): the cache lives on the
        # device, its slot choices and the pop's draws come from the step's host generator
        self.key_obj_aug = self.run_ot and bool(t.get("key_obj_aug", False))
        self.obj_cache = None
        if self.key_obj_aug:
            from .fake_object import ObjectCache

            # fused_fake_object: the HIP paste + crop and push on a ROCm device; False: the torch composition
            self.fused_fake_object = None if fused_fake_object else False
            self.obj_cache = ObjectCache(obj_cache_size, self.device, generator=self.ar_generator)

    def forward_loss(self, img1, img2, full_seg1=None, full_seg2=None, img1_ph=None, img2_ph=None,
                     key_obj_mask=None, key_obj_valid=None):
        res = self.model(img1, img2, full_seg1, full_seg2, with_bk=True)
        flows = [torch.cat([a, b], 1) for a, b in zip(res["flows_12"], res["flows_21"])]
        kw = {}
        if full_seg1 is not None:
            kw = dict(full_seg1=full_seg1, full_seg2=full_seg2)
        loss, l_ph, l_sm, fmean, vis1, _ = self.loss_fn(flows, img1, img2, **kw)
        loss = loss.mean()
        if self.has_ar:
            loss = loss + self._ar_branch(res["flows_12"][0].detach(), vis1.detach(),
                                          img1 if img1_ph is None else img1_ph, img2 if img2_ph is None else img2_ph,
                                          key_obj_mask, key_obj_valid)
        return loss, flows

    def _ar_branch(self, flow_ori, noc_ori, img1, img2, key_obj_mask=None, key_obj_valid=None):
        """w_ar * (l_atst + l_ot): the second pass on the spatially transformed
        frames and the third on a random crop, each held to the first pass's
        (transformed / cropped) flow where it was visible. With key_obj_aug and
        a full object cache the third pass's inputs get key_obj_count rounds of
        cached objects pasted in before the crop; afterwards the step's own key
        objects (``key_obj_mask`` [B,1,H,W] on the device, ``key_obj_valid`` [B]
        host bool) are pushed. Host draws in order: the pop, the crop offsets (x
        before y), the push's slots. Nothing here reads the device from the host."""
        from .ar import ar_loss, crop_offsets, random_crop

        t = self.cfg.train
        total = 0.0
        self.l_atst = self.l_ot = None
        if self.run_atst:
            s = {"imgs": [img1, img2], "flows_f": [flow_ori], "masks_f": [noc_ori]}
            if t.run_st:
                s = self.sp_transform(s)
            flow_t, noc_t = s["flows_f"][0], s["masks_f"][0]
            pred = self.model(s["imgs"][0], s["imgs"][1], with_bk=False)["flows_12"][0]
            if not t.mask_st:
                noc_t = torch.ones_like(noc_t)
            l_atst = ar_loss(pred, flow_t, noc_t, t.ar_eps, t.ar_q, fused=self.fused_ar)
            total = total + t.w_ar * l_atst
            self.l_atst = l_atst.detach()
        if self.run_ot:
            popped = None
            if self.key_obj_aug:  # None (and no draw) until the cache is full
                popped = self.obj_cache.pop(img1.shape[0] * int(t.key_obj_count), with_aug=True)
            if popped is None:
                imgs, flow_ot, noc_ot = random_crop(torch.cat([img1, img2], 1), flow_ori, noc_ori, t.ot_size,
                                                    self.ar_generator)
            else:
                from .fake_object import paste_and_crop

                offsets = crop_offsets(*img1.shape[-2:], t.ot_size, self.ar_generator)
                imgs, flow_ot, noc_ot = paste_and_crop(img1, img2, flow_ori, noc_ori, self.obj_cache, *popped,
                                                       tuple(t.ot_size), offsets, fused=self.fused_fake_object)
            pred = self.model(imgs[:, :3], imgs[:, 3:6], with_bk=False)["flows_12"][0]
            l_ot = ar_loss(pred, flow_ot, noc_ot, t.ar_eps, t.ar_q, fused=self.fused_ar)
            total = total + t.w_ar * l_ot
            self.l_ot = l_ot.detach()
            if self.key_obj_aug and key_obj_mask is not None:
                self.obj_cache.push(key_obj_mask, img1, flow_ori, key_obj_valid, fused=self.fused_fake_object)
        return total

    def __call__(self, img1, img2, full_seg1=None, full_seg2=None, img1_ph=None, img2_ph=None, key_obj_mask=None,
                 key_obj_valid=None):
        ev = None
        if self.phase_events is not None:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
        loss, _ = self.forward_loss(img1, img2, full_seg1, full_seg2, img1_ph, img2_ph, key_obj_mask, key_obj_valid)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if ev is not None:
            ev[1].record()
        torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_grad_norm)
        self.optimizer.step()
        self.scheduler.step()
        if ev is not None:
            ev[2].record()
            self.phase_events.append(ev)
        return loss.detach()


class FlatGrads:
    """Every parameter's .grad as a view of one flat fp32 buffer: static
    addresses for graph capture, and ONE all-reduce bucket per step for data
    parallelism (10 MB for PWCLite: one RCCL ring all-reduce over xGMI instead
    of DDP's per-bucket hooks). Backward accumulates into the views, so the
    buffer is zeroed at the start of every step."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.flat = torch.zeros(n, device=dev, dtype=torch.float32)
        off = 0
        for p in self.params:
            p.grad = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()

    def zero_(self):
        self.flat.zero_()

    def all_reduce_mean(self, group=None):
        import torch.distributed as dist

        world = dist.get_world_size(group)
        if world > 1:
            dist.all_reduce(self.flat, group=group)
            self.flat.div_(world)


def broadcast_params(module: torch.nn.Module, src: int = 0, group=None) -> None:
    """Replicas start from rank ``src``'s weights (what DDP's constructor does)."""
    import torch.distributed as dist

    with torch.no_grad():
        for t in list(module.parameters()) + list(module.buffers()):
            dist.broadcast(t, src, group=group)


class GraphedTrainStep:
    """The TrainStep replayed from HIP graphs (torch.cuda.CUDAGraph): the ~4k
    kernel launches of a PWCLite step (MIOpen convolutions, torch elementwise
    work and this library's kernels) are captured once and re-issued by one
    graph launch, so the step no longer pays per-launch host cost.

    Single process: one graph = zero grads + fwd(with_bk) + unFlowLoss + bwd +
    clip_grad_norm_ + Adam(capturable). Data parallel (world > 1): graph A =
    zero + fwd + loss + bwd into the flat gradient buffer, then one eager
    all-reduce of that buffer over RCCL, then graph B = clip + Adam. OneCycleLR
    runs eagerly between replays (it fills the device lr tensor in place).
    Inputs are static buffers: ``load()`` copies new frames in before a replay.
    """

    def __init__(self, step: TrainStep, img1, img2, full_seg1=None, full_seg2=None, warmup: int = 3,
                 group=None):
        import torch.distributed as dist

        from . import ops

        if getattr(step, "has_ar", False):
            raise NotImplementedError("GraphedTrainStep: the stage-1 augmentation branch (run_atst / run_ot) is not "
                                      "capturable (the crop offsets move pointers, the thetas are sampled on the host)")
        self.step = step
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.inputs = [None if t is None else t.clone() for t in (img1, img2, full_seg1, full_seg2)]
        self.grads = FlatGrads(step.module.parameters())
        dev = step.device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # allocator pools, solver selection, optimizer state
            for _ in range(warmup):  # real training steps, as TrainStep.__call__
                self._fwd_bwd()
                self._reduce()
                self._update()
                self.step.scheduler.step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        # the graphs record the raw addresses of the persistent workspaces the
        # warm-up created (warp backward, occlusion maps): this hold keeps those
        # tensors allocated for as long as the graphs can be replayed
        self.workspaces = ops.WorkspaceHold()
        if self.world == 1:
            self.graph_a = torch.cuda.CUDAGraph()
            with self.workspaces, torch.cuda.graph(self.graph_a):
                self.loss = self._fwd_bwd()
                self._update()
            self.graph_b = None
        else:
            self.graph_a = torch.cuda.CUDAGraph()
            with self.workspaces, torch.cuda.graph(self.graph_a):
                self.loss = self._fwd_bwd()
            self.graph_b = torch.cuda.CUDAGraph()
            with self.workspaces, torch.cuda.graph(self.graph_b, pool=self.graph_a.pool()):
                self._update()

    def release(self):
        """Delete the graphs and release the persistent workspaces they
        recorded. Call it on the stream the step was replayed on; the step
        cannot be called afterwards. An object that is merely dropped frees
        them too, with its hold: do that only once its replays have finished."""
        self.graph_a = self.graph_b = None
        self.workspaces.release()

    def _fwd_bwd(self):
        self.grads.zero_()
        loss, _ = self.step.forward_loss(*self.inputs)
        loss.backward()
        return loss.detach()

    def _reduce(self):
        if self.world > 1:
            self.grads.all_reduce_mean(self.group)

    def _update(self):
        torch.nn.utils.clip_grad_norm_(self.grads.params, self.step.max_grad_norm)
        self.step.optimizer.step()

    def load(self, img1, img2, full_seg1=None, full_seg2=None):
        for dst, src in zip(self.inputs, (img1, img2, full_seg1, full_seg2)):
            if dst is not None:
                dst.copy_(src)

    def __call__(self):
        if self.graph_a is None:
            raise RuntimeError("GraphedTrainStep: called after release()")
        self.graph_a.replay()
        if self.graph_b is not None:
            self._reduce()
            self.graph_b.replay()
        self.step.scheduler.step()
        return self.loss



def synthetic_flow_gt(B: int, sizes, device, seed: int = 42):
    """Ragged validation ground truth as KITTI's loader yields it, padded into
    one batch: ``sizes`` a list of B (H_b, W_b) -> (gt [B,4,Hmax,Wmax] float32
    planar (u, v, valid, noc), zero outside each sample's window, Wmax rounded up
    to a multiple of 4 as evaluate.pad_ground_truth does; size table [B,2]
    int32), both on ``device``. u, v ~ 8 N(0,1) px; about 60 % of the
    pixels are valid (KITTI's ground truth is sparse) and 75 % of those are
    non-occluded."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    if len(sizes) != B:
        raise ValueError(f"{len(sizes)} sizes for a batch of {B}")
    Hmax, Wmax = max(h for h, _ in sizes), (max(w for _, w in sizes) + 3) // 4 * 4
    g = torch.Generator(device="cpu").manual_seed(seed)
    gt = torch.zeros(B, 4, Hmax, Wmax)
    for b, (h, w) in enumerate(sizes):
        gt[b, :2, :h, :w] = torch.randn(2, h, w, generator=g) * 8.0
        valid = (torch.rand(h, w, generator=g) < 0.6).float()
        gt[b, 2, :h, :w] = valid
        gt[b, 3, :h, :w] = valid * (torch.rand(h, w, generator=g) < 0.75).float()
    return gt.to(device), torch.tensor(sizes, dtype=torch.int32).to(device)


class Validator:
    """The reference's ``_validate_with_gt`` (trainer/kitti_trainer_ar.py:360-402,
    trainer/sintel_trainer_ar.py:343-378) without its per-batch device-to-host
    copy and numpy loop: every batch runs ``model(img1, img2, with_bk=False)``
    under ``torch.no_grad()`` in ``eval()`` mode and feeds ``flows_12[0]`` to
    :class:`unsamflow_amd.evaluate.FlowMetrics`; the model's mode is restored
    afterwards. ``step_or_model``: a :class:`TrainStep` (its unwrapped module is
    used: no DDP traffic in validation) or a module.

    ``metrics="kitti"``: ``gt`` is [B,4,Hmax,Wmax] (u, v, valid, noc) with an
    optional size table, five numbers (seven with a move mask, "kitti_move").
    ``metrics="sintel"``: ``gt`` is the flow [B,2,H,W] and ``occ`` the occlusion
    mask [B,1,H,W]; valid = 1 and noc = 1 - occ as sintel_trainer_ar.py:367-369
    builds them, and the first three numbers are reported."""

    def __init__(self, step_or_model, metrics: str = "kitti", fused=None):
        from .evaluate import FlowMetrics

        if metrics not in ("kitti", "kitti_move", "sintel"):
            raise ValueError(f"metrics must be 'kitti', 'kitti_move' or 'sintel', got {metrics!r}")
        self.model = getattr(step_or_model, "module", step_or_model)
        self.kind = metrics
        self.metrics = FlowMetrics(metrics, fused=fused)

    def reset(self) -> None:
        self.metrics.reset()

    def update(self, img1, img2, gt, sizes=None, move=None, occ=None, full_seg1=None, full_seg2=None):
        """One validation batch; returns the prediction ``flows_12[0]``. Nothing
        here reads the device from the host."""
        model = self.model
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                pred = model(img1, img2, full_seg1, full_seg2, with_bk=False)["flows_12"][0]
                if self.kind == "sintel":
                    if occ is None:
                        raise ValueError("Validator(metrics='sintel') needs the occlusion mask `occ`")
                    gt = torch.cat([gt[:, :2], torch.ones_like(occ), 1 - occ], dim=1)
                self.metrics.update(pred, gt, sizes, move)
        finally:
            model.train(was_training)
        return pred

    def all_reduce(self, group=None) -> None:
        self.metrics.all_reduce(group)

    def compute(self) -> dict:
        """{name: mean over the validated samples} (the single sync)."""
        return self.metrics.compute()
