"""Validation: the reference's ``resize_flow`` and ``evaluate_flow``
(utils/flow_utils.py:62-71, 117-201) as they are used by ``_validate_with_gt``
(trainer/kitti_trainer_ar.py:360-402, trainer/sintel_trainer_ar.py:343-378) and
by the inference script (test.py:95-187).

The reference copies every predicted batch to the host and loops over its
samples in numpy: a bilinear resize to the ground truth's resolution and about
fifteen full-resolution passes per sample. Here a batch of ragged ground truths
is padded into one planar tensor with an int32 size table, and on a ROCm device
the resize, the error map, the masked sums and the outlier counts are one HIP
launch plus a small finalisation (unsamflow_amd/csrc/eval.hip); nothing reads
the device from the host until the caller asks for the numbers.

* ``resize_flow(flow, new_shape)`` is the reference's function; with ``sizes``
  every sample gets a size of its own inside a padded output.
* ``flow_errors(pred, gt, sizes, move)`` -> (metrics [B,7], sums [B,12]) per
  sample, on ``pred``'s device. The torch composition of the same formulas
  (``fused=False``, and every CPU tensor) is the reference's algorithm in fp32
  and serves as the tests' standard.
* ``evaluate_flow(gt_flows, pred_flows, moving_masks)`` is the drop-in for the
  reference's numpy interface.
* ``FlowMetrics`` accumulates the per-sample metrics on the device over a
  validation run and makes one sync at the end.

Empty masks. The reference divides by the mask's sum without a guard (only
EPE_occ is guarded by ``max(sum, 1)``): a sample whose valid (or noc, move,
static) mask is empty yields NaN (0/0) in that metric, here as there. Without a
move mask EPE_move and EPE_static are NaN. A sample whose size lies outside
[2, Hmax] x [2, Wmax] is skipped: its sums are 0, all its metrics NaN, and the
kernels raise DEVERR_EVAL_BAD_SIZE (``ops.device_errors``).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, ops
from .ar import _use_hip

# the order evaluate_flow returns and `metrics` keeps (unsamflow_hip_eval.h)
METRIC_NAMES = ("EPE_all", "EPE_noc", "EPE_occ", "Fl_all", "Fl_noc", "EPE_move", "EPE_static")
# flow_error_names of the two trainers (kitti_trainer_ar.py:368, sintel_trainer_ar.py:350)
FLOW_ERROR_NAMES = {"kitti": METRIC_NAMES[:5], "sintel": METRIC_NAMES[:3], "kitti_move": METRIC_NAMES}
NACC = _lib.EVAL_NACC
NMETRIC = _lib.EVAL_NMETRIC


def _fused_path(t: torch.Tensor, fused) -> bool:
    """A CPU tensor always takes the composition; on a device ``ar._use_hip`` decides."""
    return t.is_cuda and _use_hip(t, fused)


# ------------------------------------------------------------------ resize --
def resize_flow_torch(flow: torch.Tensor, new_shape) -> torch.Tensor:
    """flow_utils.resize_flow on any device, fp32 or fp64: bilinear
    align_corners interpolation, then u / (w / new_w) and v / (h / new_h), as
    true divisions by the quotient rounded to the tensor's type."""
    _, _, h, w = flow.shape
    new_h, new_w = int(new_shape[0]), int(new_shape[1])
    out = F.interpolate(flow, (new_h, new_w), mode="bilinear", align_corners=True)
    scale = out.new_tensor([w / float(new_w), h / float(new_h)]).view(1, 2, 1, 1)
    return out / scale


def _size_list(sizes, B: int, Hmax: int, Wmax: int):
    """The size table as a host list (a device table is copied: a sync)."""
    if sizes is None:
        return [(Hmax, Wmax)] * B
    return [(int(a), int(b)) for a, b in torch.as_tensor(sizes).tolist()]


def _size_ok(H: int, W: int, Hmax: int, Wmax: int) -> bool:
    return 2 <= H <= Hmax and 2 <= W <= Wmax


def resize_flow(flow: torch.Tensor, new_shape, sizes=None, fused=None) -> torch.Tensor:
    """Drop-in for flow_utils.resize_flow: ``flow`` [B,2,h,w] -> [B,2,H,W] for
    ``new_shape`` = (H, W). With ``sizes`` ([B,2] int32 of (H_b, W_b), on the
    flow's device for the fused path) sample b is resized to its own size into
    the window [0,H_b) x [0,W_b) of the [B,2,H,W] result, zero elsewhere; a size
    outside [2,H] x [2,W] leaves its sample zero. fp32 tensors on a ROCm device
    take the HIP kernel (a missing library is an error there, never a
    fall-back); ``fused=False`` selects the torch composition."""
    H, W = int(new_shape[0]), int(new_shape[1])
    with torch.no_grad():
        if _fused_path(flow, fused):
            if sizes is not None:
                sizes = torch.as_tensor(sizes, dtype=torch.int32).to(flow.device, non_blocking=True).contiguous()
            return ops.flow_resize(flow, sizes, H, W)
        if sizes is None:
            return resize_flow_torch(flow, (H, W))
        out = flow.new_zeros((flow.shape[0], 2, H, W))
        for b, (Hb, Wb) in enumerate(_size_list(sizes, flow.shape[0], H, W)):
            if _size_ok(Hb, Wb, H, W):
                out[b, :, :Hb, :Wb] = resize_flow_torch(flow[b:b + 1], (Hb, Wb))[0]
        return out


# ----------------------------------------------------------------- metrics --
def _bad(e: torch.Tensor, thr: torch.Tensor) -> torch.Tensor:
    """calculate_error_rate's outlier test (flow_utils.py:119-124) on e = epe * mask."""
    return ((e > 3) & (e > thr)).sum()


def flow_errors_torch(pred, gt, sizes=None, move=None):
    """evaluate_flow's per-sample arithmetic as a torch composition, in the
    tensors' type on their device: (metrics [B,7], sums [B,12]) with the columns
    of unsamflow_hip_eval.h. The sums are torch's; the ratios are formed in fp64
    and stored in ``pred``'s type, as the kernel's finalisation does."""
    B, Cg, Hmax, Wmax = gt.shape
    if Cg not in (2, 4):
        raise ValueError(f"gt must have 2 or 4 channels (u, v, valid, noc), got {Cg}")
    sums = torch.zeros((B, NACC), dtype=torch.float64, device=pred.device)
    ok = torch.zeros(B, dtype=torch.bool)
    for b, (H, W) in enumerate(_size_list(sizes, B, Hmax, Wmax)):
        if not _size_ok(H, W, Hmax, Wmax):
            continue
        ok[b] = True
        g = gt[b, :, :H, :W]
        flo = resize_flow_torch(pred[b:b + 1], (H, W))[0]
        epe = torch.sqrt(torch.sum(torch.square(flo - g[:2]), dim=0))
        valid = g[2] if Cg == 4 else torch.ones_like(epe)
        noc = g[3] if Cg == 4 else torch.ones_like(epe)
        thr = 0.05 * torch.sqrt(torch.sum(torch.square(g[:2]), dim=0))
        occ = valid - noc
        s = [torch.sum(epe * valid), torch.sum(valid), torch.sum(epe * noc), torch.sum(noc),
             torch.sum(epe * occ), torch.sum(occ)]
        if move is not None:
            mv = move[b, 0, :H, :W]
            s += [torch.sum(epe * valid * mv), torch.sum(valid * mv),
                  torch.sum(epe * valid * (1.0 - mv)), torch.sum(valid * (1.0 - mv))]
        else:
            s += [epe.new_zeros(())] * 4
        s += [_bad(epe * valid, thr), _bad(epe * noc, thr)]
        sums[b] = torch.stack([v.double() for v in s])
    s = sums.unbind(1)
    nan = torch.full_like(s[0], float("nan"))
    has_move = move is not None
    cols = [s[0] / s[1], s[2] / s[3], s[4] / s[5].clamp(min=1.0), s[10] / s[1] * 100.0, s[11] / s[3] * 100.0,
            s[6] / s[7] if has_move else nan, s[8] / s[9] if has_move else nan]
    metrics = torch.stack(cols, dim=1)
    metrics[~ok.to(metrics.device)] = float("nan")
    return metrics.to(pred.dtype), sums.to(pred.dtype)


def flow_errors(pred, gt, sizes=None, move=None, fused=None):
    """Per-sample validation numbers of a batch: ``pred`` [B,2,h,w] (a channel
    slice of a [B,4,h,w] tensor is used in place), ``gt`` [B,Cg,Hmax,Wmax] planar
    with Cg = 2 (u, v) or 4 (u, v, valid, noc), ``sizes`` [B,2] int32 (H_b, W_b)
    or None (every sample fills the planes), ``move`` [B,1,Hmax,Wmax] or None
    -> (metrics [B,7] in the order of ``METRIC_NAMES``, sums [B,12]) on ``pred``'s
    device. The prediction is resized to each sample's size as ``resize_flow``
    does; the padding outside a sample's window is never read.

    fp32 tensors on a ROCm device take the fused kernels (no host sync, two runs
    agree bit for bit; a missing library is an error there, never a fall-back);
    ``fused=False``, and every CPU tensor, runs the torch composition."""
    with torch.no_grad():
        if _fused_path(pred, fused):
            if sizes is not None:
                sizes = torch.as_tensor(sizes, dtype=torch.int32).to(pred.device, non_blocking=True).contiguous()
            return ops.flow_eval(pred, gt, sizes, move)
        return flow_errors_torch(pred, gt, sizes, move)


def pad_ground_truth(gt_flows, moving_masks=None):
    """Lists of HWC numpy ground truths (and HW or HW1 move masks) of differing
    sizes -> (gt [B,C,Hmax,Wmax], sizes [B,2] int32, move [B,1,Hmax,Wmax] or
    None): float32 CPU tensors, planar, zero outside each sample's window. Wmax
    is rounded up to a multiple of 4, so every plane starts on a 16-byte
    boundary and the kernels take their 16-byte loads (KITTI's 375 x 1242 alone
    would not)."""
    B = len(gt_flows)
    shapes = [g.shape for g in gt_flows]
    C = shapes[0][-1]
    if any(len(s) != 3 or s[-1] != C for s in shapes) or C not in (2, 4):
        raise ValueError(f"ground truths must be HxWx2 or HxWx4 arrays of one channel count, got {shapes}")
    Hmax, Wmax = max(s[0] for s in shapes), (max(s[1] for s in shapes) + 3) // 4 * 4
    gt = torch.zeros((B, C, Hmax, Wmax), dtype=torch.float32)
    move = None if moving_masks is None else torch.zeros((B, 1, Hmax, Wmax), dtype=torch.float32)
    for b, g in enumerate(gt_flows):
        H, W = g.shape[:2]
        gt[b, :, :H, :W] = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).permute(2, 0, 1)
        if move is not None:
            m = np.asarray(moving_masks[b], dtype=np.float32).reshape(H, W)
            move[b, 0, :H, :W] = torch.from_numpy(m)
    sizes = torch.tensor([s[:2] for s in shapes], dtype=torch.int32)
    return gt, sizes, move


def evaluate_flow(gt_flows, pred_flows, moving_masks=None, device=None, fused=None):
    """Drop-in for flow_utils.evaluate_flow: ``gt_flows`` a list of HxWx2 or
    HxWx4 numpy ground truths (sizes may differ), ``pred_flows`` an NHWC numpy
    prediction [B,h,w,2], ``moving_masks`` an optional list of HxW masks ->
    a list of Python floats, the means over the samples: [EPE] for 2-channel
    ground truth, else [EPE_all, EPE_noc, EPE_occ, Fl_all, Fl_noc] and, with
    moving masks, EPE_move and EPE_static. The work runs on ``device`` (default:
    the ROCm device when one is present, else the CPU)."""
    if device is None:
        device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    device = torch.device(device)
    gt, sizes, move = pad_ground_truth(gt_flows, moving_masks)
    pred = torch.from_numpy(np.ascontiguousarray(pred_flows, dtype=np.float32)).permute(0, 3, 1, 2).contiguous()
    if device.type != "cpu":
        pred, gt, sizes = pred.to(device), gt.to(device), sizes.to(device)
        move = None if move is None else move.to(device)
    metrics, _ = flow_errors(pred, gt, sizes, move, fused=fused)
    mean = metrics.double().mean(dim=0).tolist()  # the one sync
    if gt.shape[1] == 2:
        return mean[:1]
    return mean[:5] + (mean[5:7] if moving_masks is not None else [])


class FlowMetrics:
    """Running validation metrics: the per-metric sums over the samples seen and
    their count, both as device tensors (fp64). ``update`` only queues device
    work; ``compute`` makes the single sync. The result is the mean over the
    samples, which is what the reference's batch-weighted ``AverageMeter`` of
    per-batch means yields. ``names``: "kitti" (5 numbers), "sintel" (3),
    "kitti_move" (7), or a tuple of leading ``METRIC_NAMES``."""

    def __init__(self, names="kitti", device=None, fused=None):
        self.names = tuple(FLOW_ERROR_NAMES[names] if isinstance(names, str) else names)
        if self.names != METRIC_NAMES[:len(self.names)]:
            raise ValueError(f"names must be leading entries of {METRIC_NAMES}, got {self.names}")
        self.fused = fused
        self.device = None if device is None else torch.device(device)
        self.total = self.count = None

    def reset(self) -> None:
        self.total = self.count = None

    def _init(self, device) -> None:
        if self.device is None:
            self.device = torch.device(device)
        self.total = torch.zeros(NMETRIC, dtype=torch.float64, device=self.device)
        self.count = torch.zeros((), dtype=torch.float64, device=self.device)

    def update(self, pred, gt, sizes=None, move=None):
        """Add a batch (the arguments of :func:`flow_errors`); returns its
        per-sample metrics [B,7]. Never reads the device from the host."""
        metrics, _ = flow_errors(pred, gt, sizes, move, fused=self.fused)
        if self.total is None:
            self._init(metrics.device)
        self.total += metrics.double().sum(dim=0)
        self.count += metrics.shape[0]
        return metrics

    def all_reduce(self, group=None) -> None:
        """Sum the running totals and counts over the ranks of ``group``."""
        import torch.distributed as dist

        if self.total is None:
            raise RuntimeError("FlowMetrics.all_reduce before the first update (the device is not known yet)")
        dist.all_reduce(self.total, group=group)
        dist.all_reduce(self.count, group=group)

    def compute(self) -> dict:
        """{name: mean over the samples} as Python floats (one sync)."""
        if self.total is None:
            return {n: float("nan") for n in self.names}
        mean = (self.total / self.count).tolist()
        return {n: mean[i] for i, n in enumerate(self.names)}
