"""The homography smoothness loss of stage 2 (the reference's
``losses/loss_blocks.py:125-200``, ``smooth_type: "homography"``).

Per sample the six segments with the most occluded pixels (id 0 aside) are
refined: a homography is fitted by RANSAC to the segment's non-occluded
("reliable") pixel pairs ``p -> p + flow``, and the loss is the L1 distance of
``p + flow`` to ``dehom(H p)`` over the whole segment, / (h * w), / B. H passes
through numpy in the reference, so it is a constant of the loss::

    dloss/dflow = -sign(diff) / (h * w * B)   on the refined segments

The reference fits with ``cv2.findHomography`` on the host, one round trip per
segment. Here the fit is this project's own RANSAC, specified in
``include/unsamflow_hip_hg.h`` (a counter-hash draw of 4-point samples, all
reliable pairs scored, a Hartley-normalised least-squares refit; cv2's LM polish
is out of scope):

* :func:`fit_homographies` -> ``records``, int32 ``[B, 6, 16]``: per (sample,
  slot) ``id, status, n_seg, n_rel, n_inl, H[9] (float bits), best_j, offset``.
  On a ROCm device it is the kernels of ``csrc/hg.hip``, with no host sync.
* :func:`homography_loss` -> the loss of given records, an autograd op with a
  gradient to ``flow`` only.
* :func:`smooth_homography` is fit plus loss.
* :func:`smooth_homography_torch` is the reference's host loop restated in
  torch, with a pluggable estimator whose default,
  :func:`ransac_homography_np`, restates the kernels' RANSAC in numpy (the same
  hash stream, the same point order, fp64). It serves CPU tensors and
  ``fused=False`` and is the A/B partner of the kernels.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd import Function

from . import ops
from ._lib import HG_DEFAULT_HYP, HG_MAX_K, HG_RECORD_WORDS, HG_SLOTS, HG_STATUS  # noqa: F401

ACCEPTED, FEW_RELIABLE, LOW_RELIABLE, LOW_INLIER, DEGENERATE, EMPTY = range(6)

_G = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


# ------------------------------------------------------------- the records --
def records_status(records):
    """[B, 6] status codes (``HG_STATUS`` names them)."""
    return records[..., 1]


def records_H(records):
    """[B, 6, 3, 3] float32 homographies (zeros where no fit was made)."""
    return records[..., 5:14].contiguous().view(torch.float32).reshape(*records.shape[:-1], 3, 3)


# ------------------------------------------ the RANSAC of the header, numpy --
def _mix(z):
    with np.errstate(over="ignore"):
        z = z + _G
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def hypothesis_positions(n_rel, sample, slot, n_hyp=HG_DEFAULT_HYP, seed=0):
    """[n_hyp, 4] list positions of every hypothesis of (sample, slot): the counter hash of the header."""
    j = np.arange(n_hyp, dtype=np.uint64)[:, None]
    t = np.arange(4, dtype=np.uint64)[None, :]
    c = (np.uint64((sample * 8 + slot) << 34) | (j << np.uint64(2))) | t
    base = _mix(np.array([seed & (2 ** 64 - 1)], dtype=np.uint64))
    with np.errstate(over="ignore"):
        z = _mix(base + c)
    return (((z >> np.uint64(32)) * np.uint64(n_rel)) >> np.uint64(32)).astype(np.int64)


def _solve8(A, tol):
    """Batched ``A[:, :, :8] h = A[:, :, 8]`` by Gaussian elimination with partial pivoting (the first
    largest |pivot| from the top), as ``solve8`` of csrc/hg.hip -> (h [n, 8], ok [n])."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    idx = np.arange(n)
    ok = np.ones(n, dtype=bool)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), (n,))
    with np.errstate(all="ignore"):
        for k in range(8):
            col = np.abs(A[:, k:, k])
            p = np.argmax(col, axis=1) + k
            ok &= col[idx, p - k] > tol
            rows = A[idx, p].copy()
            A[idx, p] = A[:, k]
            A[:, k] = rows
            inv = 1.0 / np.where(ok, A[:, k, k], 1.0)
            f = A[:, k + 1:, k] * inv[:, None]
            A[:, k + 1:, k + 1:] -= f[:, :, None] * A[:, None, k, k + 1:]
        h = np.zeros((n, 8))
        for k in range(7, -1, -1):
            s = A[:, k, 8].copy()
            for c in range(k + 1, 8):
                s -= A[:, k, c] * h[:, c]
            h[:, k] = s / np.where(ok, A[:, k, k], 1.0)
    return h, ok


def _dlt_rows(x, y, u, v):
    """The two rows per pair of the h33 = 1 system and their right-hand sides."""
    z, o = np.zeros_like(x), np.ones_like(x)
    r1 = np.stack([x, y, o, z, z, z, -x * u, -y * u], axis=-1)
    r2 = np.stack([z, z, z, x, y, o, -x * v, -y * v], axis=-1)
    return r1, r2


def inliers_np(H, pts1, pts2, thr):
    """The transfer-error test of the header in fp64: |H p1 - p2 w|^2 <= thr^2 w^2 and w != 0."""
    H = np.asarray(H, dtype=np.float64).reshape(3, 3)
    p1, p2 = np.asarray(pts1, dtype=np.float64), np.asarray(pts2, dtype=np.float64)
    X = H[0, 0] * p1[:, 0] + H[0, 1] * p1[:, 1] + H[0, 2]
    Y = H[1, 0] * p1[:, 0] + H[1, 1] * p1[:, 1] + H[1, 2]
    Wd = H[2, 0] * p1[:, 0] + H[2, 1] * p1[:, 1] + H[2, 2]
    dx, dy = X - p2[:, 0] * Wd, Y - p2[:, 1] * Wd
    thr2 = float(np.float32(thr)) ** 2
    return (Wd != 0) & (dx * dx + dy * dy <= thr2 * Wd * Wd)


def refit_homography_np(pts1, pts2):
    """The header's refit on the given pairs: Hartley normalisation, the 8x8 normal equations of the
    h33 = 1 system in fp64, denormalised and divided by its last entry -> fp64 [3, 3], or None."""
    p1, p2 = np.asarray(pts1, dtype=np.float64), np.asarray(pts2, dtype=np.float64)
    if len(p1) < 4:
        return None
    c1, c2 = p1.mean(0), p2.mean(0)
    d1 = np.sqrt(((p1 - c1) ** 2).sum(1)).mean()
    d2 = np.sqrt(((p2 - c2) ** 2).sum(1)).mean()
    if not (d1 > 0 and d2 > 0):
        return None
    s1, s2 = np.sqrt(2.0) / d1, np.sqrt(2.0) / d2
    a, b = s1 * (p1 - c1), s2 * (p2 - c2)
    r1, r2 = _dlt_rows(a[:, 0], a[:, 1], b[:, 0], b[:, 1])
    AtA = r1.T @ r1 + r2.T @ r2
    Atb = r1.T @ b[:, 0] + r2.T @ b[:, 1]
    h, ok = _solve8(np.concatenate([AtA, Atb[:, None]], axis=1)[None], 1e-11 * np.abs(np.diag(AtA)).max())
    if not ok[0]:
        return None
    Hn = np.append(h[0], 1.0).reshape(3, 3)
    T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1]])
    T2i = np.array([[1 / s2, 0, c2[0]], [0, 1 / s2, c2[1]], [0, 0, 1]])
    with np.errstate(all="ignore"):
        H = T2i @ Hn @ T1
        H = H / H[2, 2]
    return H if np.isfinite(H).all() else None


def hypotheses_np(pts1, pts2, sample=0, slot=0, n_hyp=HG_DEFAULT_HYP, seed=0):
    """Every hypothesis of (sample, slot) on the reliable pairs: (H [n_hyp, 9] rounded to fp32, valid [n_hyp])."""
    p1, p2 = np.asarray(pts1, dtype=np.float32), np.asarray(pts2, dtype=np.float32)
    q = hypothesis_positions(len(p1), sample, slot, n_hyp, seed)
    valid = np.array([len(set(r)) == 4 for r in q.tolist()])
    a, b = p1[q].astype(np.float64), p2[q].astype(np.float64)  # [n_hyp, 4, 2]
    r1, r2 = _dlt_rows(a[..., 0], a[..., 1], b[..., 0], b[..., 1])
    A = np.zeros((n_hyp, 8, 9))
    A[:, 0::2, :8], A[:, 1::2, :8] = r1, r2
    A[:, 0::2, 8], A[:, 1::2, 8] = b[..., 0], b[..., 1]
    h, ok = _solve8(A, 1e-10)
    valid &= ok & np.isfinite(h).all(1)
    return np.concatenate([h, np.ones((n_hyp, 1))], axis=1).astype(np.float32), valid


def ransac_homography_np(pts1, pts2, thr, sample=0, slot=0, n_hyp=HG_DEFAULT_HYP, seed=0, chunk=16, info=None):
    """The RANSAC of ``include/unsamflow_hip_hg.h`` on the reliable pairs of one slot, in numpy fp64:
    ``(H float32 [3, 3], mask bool [n])`` like ``cv2.findHomography``, or ``(None, None)`` where the
    kernels report a degenerate slot. ``info`` (a dict) receives ``best_j`` and the scores."""
    p1, p2 = np.asarray(pts1, dtype=np.float32), np.asarray(pts2, dtype=np.float32)
    Hs, valid = hypotheses_np(p1, p2, sample, slot, n_hyp, seed)
    Hs = Hs.astype(np.float64)
    counts = np.zeros(n_hyp, dtype=np.int64)
    x, y, u, v = (c.astype(np.float64) for c in (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]))
    thr2 = float(np.float32(thr)) ** 2
    for j0 in range(0, n_hyp, chunk):
        Hc = Hs[j0:j0 + chunk, :, None]
        Wd = Hc[:, 6] * x + Hc[:, 7] * y + Hc[:, 8]
        dx = Hc[:, 0] * x + Hc[:, 1] * y + Hc[:, 2] - u * Wd
        dy = Hc[:, 3] * x + Hc[:, 4] * y + Hc[:, 5] - v * Wd
        counts[j0:j0 + chunk] = ((Wd != 0) & (dx * dx + dy * dy <= thr2 * Wd * Wd)).sum(1)
    counts[~valid] = 0
    best = int(np.argmax(counts))  # the first largest: the lowest j on ties
    if info is not None:
        info.update(best_j=best if counts[best] > 0 else -1, scores=counts)
    if counts[best] < 4:
        return None, None
    inl = inliers_np(Hs[best], p1, p2, thr)
    H = refit_homography_np(p1[inl], p2[inl])
    if H is None:
        return None, None
    H = H.astype(np.float32)
    return H, inliers_np(H, p1, p2, thr)


# ------------------------------------------- the reference's loop in torch --
def _num_segments(full_seg, num_segments):
    return int(full_seg.max()) + 1 if num_segments is None else int(num_segments)


def fit_homographies_torch(flow, full_seg, occ_mask, ransac_threshold=3, num_segments=None, find_homography=None,
                           n_hyp=HG_DEFAULT_HYP, seed=0):
    """The selection, the drop rules and the fit of the reference's loop (loss_blocks.py:131-178) ->
    records on ``flow``'s device. ``find_homography(pts1, pts2, thr, sample, slot) -> (H, mask)`` (H None:
    a skipped segment) defaults to :func:`ransac_homography_np`. Every id must be an integer in
    [0, num_segments). One host round trip per segment, as in the reference."""
    if find_homography is None:
        def find_homography(p1, p2, thr, sample, slot):
            return ransac_homography_np(p1, p2, thr, sample, slot, n_hyp, seed)
    B, _, h, w = flow.shape
    K = _num_segments(full_seg, num_segments)
    dev = flow.device
    rec = np.zeros((B, HG_SLOTS, HG_RECORD_WORDS), dtype=np.int32)
    rec[:, :, 0], rec[:, :, 1], rec[:, :, 14] = -1, EMPTY, -1
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    coords1 = torch.stack((xs, ys), dim=2).float().to(dev)
    for i in range(B):
        seg_i, occ_i = full_seg[i, 0], occ_mask[i, 0]
        occ_ids = seg_i[occ_i.to(bool)].long()
        counts = torch.bincount(occ_ids, minlength=K)[:K].cpu().numpy()
        # (occluded count descending, id ascending), id 0 dropped, the first six
        order = sorted(range(1, K), key=lambda k: (-int(counts[k]), k))[:HG_SLOTS]
        coords2 = coords1 + flow[i].detach().permute(1, 2, 0).float()
        for slot, k in enumerate(order):
            m = seg_i == k
            reliable = (1 - occ_i[m]).bool().cpu().numpy()
            r = rec[i, slot]
            r[0], r[2], r[3] = k, reliable.size, int(reliable.sum())
            if reliable.sum() < 4:
                r[1] = FEW_RELIABLE
                continue
            if reliable.mean() < 0.2:
                r[1] = LOW_RELIABLE
                continue
            rel = torch.from_numpy(reliable).to(dev)
            H, mask = find_homography(coords1[m][rel].cpu().numpy(), coords2[m][rel].cpu().numpy(),
                                      ransac_threshold, i, slot)
            if H is None:
                r[1] = DEGENERATE
                continue
            mask = np.asarray(mask).astype(bool).reshape(-1)
            r[4] = int(mask.sum())
            r[5:14] = np.asarray(H, dtype=np.float32).reshape(9).view(np.int32)
            r[1] = LOW_INLIER if mask.mean() < 0.5 else ACCEPTED
    return torch.from_numpy(rec).to(dev)


def homography_loss_torch(flow, full_seg, records):
    """The loss of given records as the reference composes it (loss_blocks.py:179-200), in ``flow``'s
    dtype, differentiable w.r.t. ``flow``; H is a constant."""
    B, _, h, w = flow.shape
    dev = flow.device
    rec = records.cpu()
    Hs = records_H(rec)
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    coords1 = torch.stack((xs, ys), dim=2).to(flow.dtype).to(dev)
    loss = flow[:0].sum()  # a zero that is a function of flow: no accepted slot still has a (zero) gradient
    for i in range(B):
        coords2 = coords1 + flow[i].permute(1, 2, 0)
        for slot in range(HG_SLOTS):
            if int(rec[i, slot, 1]) != ACCEPTED:
                continue
            m = full_seg[i, 0] == int(rec[i, slot, 0])
            pts1, pts2 = coords1[m], coords2[m]
            H = Hs[i, slot].to(flow.dtype).to(dev)
            pts1_homo = torch.cat((pts1, torch.ones((pts1.shape[0], 1), dtype=flow.dtype, device=dev)), dim=1)
            new_homo = torch.matmul(H, pts1_homo.T).T
            diff = new_homo[:, :2] / new_homo[:, 2:3] - pts2
            loss = loss + diff.abs().sum() / (h * w)
    return loss / B


def smooth_homography_torch(flow, full_seg, occ_mask, ransac_threshold=3, num_segments=None, find_homography=None,
                            n_hyp=HG_DEFAULT_HYP, seed=0):
    """The reference's ``smooth_homography``: the host loop of :func:`fit_homographies_torch` and the
    loss of its records."""
    rec = fit_homographies_torch(flow, full_seg, occ_mask, ransac_threshold, num_segments, find_homography, n_hyp,
                                 seed)
    return homography_loss_torch(flow, full_seg, rec)


# ----------------------------------------------------------- the HIP path --
def _use_hip(t: torch.Tensor, fused) -> bool:
    """fp32 tensors on a ROCm device take the HIP path (a missing library is an
    error there, never a fall-back); ``fused=False`` selects the composition."""
    if fused is None:
        return t.is_cuda and t.dtype == torch.float32
    return bool(fused)


def _f32(t):
    return t if t.dtype == torch.float32 else t.to(torch.float32)


def fit_homographies(flow, full_seg, occ_mask, ransac_threshold=3, num_segments=None, n_hyp=HG_DEFAULT_HYP, seed=0,
                     fused=None):
    """Select the six segments per sample and fit their homographies -> records (module docstring).
    ``flow`` [B,2,h,w] (a channel slice of a [B,4,h,w] tensor is read in place); ``full_seg``
    [B,1,h,w] integer ids in [0, num_segments); ``occ_mask`` [B,1,h,w], 1 where occluded.

    With ``num_segments`` given the fused call does no host sync and can be captured into a HIP
    graph; ``None`` reads ``full_seg.max()`` back first -- the only sync of the path. On the fused
    path a pixel whose id is outside [0, num_segments) or not an integer belongs to no segment
    and raises USF_DEVERR_HG_BAD_ID (``ops.device_errors``). The fit is not differentiated."""
    if not _use_hip(flow, fused):
        return fit_homographies_torch(flow, full_seg, occ_mask, ransac_threshold, num_segments, None, n_hyp, seed)
    K = _num_segments(full_seg, num_segments)
    return ops.hg_fit(flow.detach(), _f32(full_seg), _f32(occ_mask.detach()), K, ransac_threshold, n_hyp, seed)


class HomographyLossFunction(Function):
    @staticmethod
    def forward(ctx, flow, full_seg, records):
        ctx.save_for_backward(flow, full_seg, records)
        return ops.hg_loss_forward(flow, full_seg, records)

    @staticmethod
    def backward(ctx, grad_loss):
        gflow = None
        if ctx.needs_input_grad[0]:
            flow, full_seg, records = ctx.saved_tensors
            gflow = ops.hg_loss_backward(flow, full_seg, records, grad_loss.reshape(1))
        return gflow, None, None


def homography_loss(flow, full_seg, records, fused=None):
    """The loss of given records: sum over the accepted slots' segments of
    ``|dehom(H p) - (p + flow)|`` / (h * w * B). Nothing is saved for the backward but the inputs
    and the records; the gradient reaches ``flow`` only."""
    if not _use_hip(flow, fused):
        return homography_loss_torch(flow, full_seg, records)
    if full_seg.requires_grad:
        raise NotImplementedError("segment ids carry no gradient")
    return HomographyLossFunction.apply(flow, _f32(full_seg).contiguous(), records)


def smooth_homography(flow, full_seg, occ_mask, ransac_threshold=3, num_segments=None, fused=None,
                      n_hyp=HG_DEFAULT_HYP, seed=0):
    """The reference's ``smooth_homography(flo, full_seg, occ_mask, ransac_threshold)``: fit plus loss.
    fp32 tensors on a ROCm device run the kernels (``fused=False``: the host loop of
    :func:`smooth_homography_torch`)."""
    if not _use_hip(flow, fused):
        return smooth_homography_torch(flow, full_seg, occ_mask, ransac_threshold, num_segments, None, n_hyp, seed)
    rec = fit_homographies(flow, full_seg, occ_mask, ransac_threshold, num_segments, n_hyp, seed, fused=True)
    return homography_loss(flow, full_seg, rec, fused=True)
