"""Shared by the flow-evaluation tests and tests/golden/make_golden_eval.py:
the four cases, their inputs (regenerated from oracle/hashrng.py, never
stored) and an fp64 numpy restatement of the reference's resize_flow +
evaluate_flow (utils/flow_utils.py:62-71, 117-201).

The restatement states the same real-valued function as the reference: the
source positions are the fp32 numbers ATen's align_corners bilinear forms
(scale (in - 1) / (out - 1) in fp32, position scale * index in fp32) and the
channel divisors are w / W and h / H rounded to fp32, as the reference's
in-place division sees them; everything after that is fp64.

Outlier counts. fp32 rounding can flip "epe > 3" or "epe > 0.05 |gt|" only at
pixels whose fp64 EPE lies within rounding distance of a threshold. The
generator invalidates every valid pixel whose fp64 EPE lies within 1e-3 of 3,
or within 1e-3 of 0.05 |gt| while its EPE exceeds 2.9 (both tests must hold for
a pixel to count, so the second threshold matters only near or above the first),
far more than the 1e-5 the fp32 paths may deviate; the counts of what remains
are exact in every implementation. It asserts that this removes at most 0.2 %
of the valid pixels (a condition, not a measurement).
"""
import numpy as np

from oracle import hashrng

# name -> (B, (h, w) of the prediction, per-sample (H_b, W_b), seed)
CASES = {
    "ragged_small": (2, (8, 16), ((11, 23), (9, 19)), 9500),   # odd sizes, per-sample window, padding ignored
    "identity": (1, (6, 10), ((6, 10),), 9510),                 # scale 1, upper tap clamp
    "multi_block": (2, (16, 40), ((70, 150), (64, 131)), 9520),  # many workgroups, empty tail workgroups
    "kitti_like": (2, (64, 208), ((375, 1242), (370, 1226)), 9530),  # real ragged sizes, long sums
}
SMALL = ("ragged_small", "identity")  # the golden stores the resized flow itself for these
MARGIN = 1e-3
MAX_INVALIDATED = 0.002
EPE_COLS, FL_COLS = [0, 1, 2, 5, 6], [3, 4]  # columns of the metrics
TOL = dict(atol=1e-5, rtol=1e-5)  # EPE numbers and the resized flow against the capture
NAMES = ("EPE_all", "EPE_noc", "EPE_occ", "Fl_all", "Fl_noc", "EPE_move", "EPE_static")


def _taps(out: int, inp: int):
    scale = np.float32(inp - 1) / np.float32(out - 1)
    src = (scale * np.arange(out, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), inp - 1)
    i1 = i0 + (i0 < inp - 1)
    l1 = src.astype(np.float64) - i0
    return i0, i1, 1.0 - l1, l1


def resize_f64(pred: np.ndarray, H: int, W: int) -> np.ndarray:
    """resize_flow of one sample: pred [2,h,w] -> [2,H,W] float64."""
    _, h, w = pred.shape
    y0, y1, ly0, ly1 = _taps(H, h)
    x0, x1, lx0, lx1 = _taps(W, w)
    p = pred.astype(np.float64)
    top = p[:, y0][:, :, x0] * lx0 + p[:, y0][:, :, x1] * lx1
    bot = p[:, y1][:, :, x0] * lx0 + p[:, y1][:, :, x1] * lx1
    out = ly0[None, :, None] * top + ly1[None, :, None] * bot
    out[0] /= float(np.float32(w / float(W)))
    out[1] /= float(np.float32(h / float(H)))
    return out


def epe_f64(pred: np.ndarray, gt: np.ndarray) -> np.ndarray:
    """EPE map [H,W] of one sample: pred [2,h,w], gt [H,W,C]."""
    H, W = gt.shape[:2]
    flo = resize_f64(pred, H, W)
    g = gt.astype(np.float64)
    return np.sqrt((flo[0] - g[..., 0]) ** 2 + (flo[1] - g[..., 1]) ** 2)


def evaluate_f64(pred: np.ndarray, gts, moves=None):
    """Per-sample (metrics [B,7], bad counts [B,2] int64) in fp64 from pred
    [B,2,h,w] and lists of HWC ground truths / HW move masks; NaN where the
    reference has no number (2-channel gt: masks of ones; no move: columns 5, 6)."""
    B = len(gts)
    metrics = np.full((B, 7), np.nan)
    bad = np.zeros((B, 2), dtype=np.int64)
    for b, gt in enumerate(gts):
        g = gt.astype(np.float64)
        epe = epe_f64(pred[b], gt)
        ones = np.ones_like(epe)
        valid, noc = (g[..., 2], g[..., 3]) if gt.shape[-1] == 4 else (ones, ones)
        thr = 0.05 * np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2)
        for k, m in enumerate((valid, noc)):
            bad[b, k] = int(np.sum((epe * m > 3) & (epe * m > thr)))
        occ = valid - noc
        with np.errstate(invalid="ignore", divide="ignore"):
            metrics[b, :5] = [np.sum(epe * valid) / np.sum(valid), np.sum(epe * noc) / np.sum(noc),
                              np.sum(epe * occ) / max(np.sum(occ), 1.0), bad[b, 0] / np.sum(valid) * 100.0,
                              bad[b, 1] / np.sum(noc) * 100.0]
            if moves is not None:
                mv = moves[b].astype(np.float64)
                metrics[b, 5] = np.sum(epe * valid * mv) / np.sum(valid * mv)
                metrics[b, 6] = np.sum(epe * valid * (1.0 - mv)) / np.sum(valid * (1.0 - mv))
    return metrics, bad


_CACHE = {}


def case(name: str):
    """The inputs of a case, built once and shared (treat as read-only):
    ``pred`` [B,2,h,w]; ``gts`` a list of HxWx4 (u, v, valid, noc) and ``moves`` a
    list of HxW float32 arrays; ``sizes`` [B,2] int32; ``invalidated`` and
    ``valid_before``, the counts behind the 0.2 % cap."""
    if name in _CACHE:
        return _CACHE[name]
    B, (h, w), sizes, seed = CASES[name]
    pred = hashrng.symmetric((B, 2, h, w), seed, 6)
    gts, moves, removed, before = [], [], 0, 0
    for b, (H, W) in enumerate(sizes):
        s = seed + 10 * (b + 1)
        flow = (resize_f64(pred[b], H, W).astype(np.float32) + hashrng.symmetric((2, H, W), s, 5)).astype(np.float32)
        valid = hashrng.uniform((H, W), s + 1) < 0.6
        noc = valid & (hashrng.uniform((H, W), s + 2) < 0.75)
        move = (hashrng.uniform((H, W), s + 3) < 0.3).astype(np.float32)
        gt = np.concatenate([flow.transpose(1, 2, 0), valid[..., None], noc[..., None]], axis=2).astype(np.float32)
        epe = epe_f64(pred[b], gt)
        mag = 0.05 * np.sqrt(gt[..., 0].astype(np.float64) ** 2 + gt[..., 1].astype(np.float64) ** 2)
        near = (np.abs(epe - 3.0) < MARGIN) | ((np.abs(epe - mag) < MARGIN) & (epe > 2.9))
        before += int(valid.sum())
        removed += int((valid & near).sum())
        gt[near, 2:] = 0.0
        gts.append(gt)
        moves.append(move)
    assert removed <= MAX_INVALIDATED * before, (name, removed, before)
    out = {"name": name, "B": B, "hw": (h, w), "pred": pred, "gts": gts, "moves": moves,
           "sizes": np.array(sizes, dtype=np.int32), "invalidated": removed, "valid_before": before}
    _CACHE[name] = out
    return out


def planar_batch(c, channels: int = 4, fill: float = float("nan"), pad_to=None):
    """(gt [B,channels,Hmax,Wmax], move [B,1,Hmax,Wmax]) float32 of a case, the
    padding outside each sample's window holding ``fill`` (NaN: whatever reads
    the padding shows up in the result)."""
    Hmax, Wmax = pad_to or (int(c["sizes"][:, 0].max()), int(c["sizes"][:, 1].max()))
    gt = np.full((c["B"], channels, Hmax, Wmax), fill, dtype=np.float32)
    move = np.full((c["B"], 1, Hmax, Wmax), fill, dtype=np.float32)
    for b, (g, m) in enumerate(zip(c["gts"], c["moves"])):
        H, W = g.shape[:2]
        gt[b, :, :H, :W] = g[..., :channels].transpose(2, 0, 1)
        move[b, 0, :H, :W] = m
    return gt, move


# ---------------------------------------------- checks against the capture --
def check_metrics(got, golden, name, move=True, channels=4):
    """Per-sample metrics [B,7] (numpy) against the capture of ``name``."""
    got = np.asarray(got, dtype=np.float64)
    if channels == 2:
        np.testing.assert_allclose(got[:, 0], golden[f"{name}_sample1"], **TOL)
        return
    want = golden[f"{name}_sample7"]
    cols = EPE_COLS if move else EPE_COLS[:3]
    print(f"[eval] {name}: max rel EPE deviation {np.max(np.abs(got[:, cols] - want[:, cols]) / want[:, cols]):.2e}")
    np.testing.assert_allclose(got[:, cols], want[:, cols], **TOL)
    np.testing.assert_allclose(got[:, FL_COLS], want[:, FL_COLS], rtol=1e-5, atol=0)
    if not move:
        assert np.isnan(got[:, 5:]).all()


def check_counts(sums, golden, name):
    assert np.array_equal(np.asarray(sums)[:, 10:12].astype(np.int64), golden[f"{name}_bad"])
