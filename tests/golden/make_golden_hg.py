"""Generate tests/golden/hg_smooth.npz by running the REFERENCE's
smooth_homography (losses/loss_blocks.py:125-200) with a stub estimator.

Run where a checkout of the reference is at hand (it is imported, never copied):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hg.py /path/to/reference

OpenCV is not needed: a ``cv2`` stub is installed whose ``findHomography`` is
the plain fp64 least-squares fit of tests/hg_util.py over the points it is
given, with ``mask = residual <= thr``. So the golden pins everything AROUND the
estimator -- the selection of the six segments, the drop rules, the order and
the point sets of the estimator calls, the inlier-share test, the loss and its
gradient -- as the reference's own code computes it (torch CPU fp32).

Per case of hg_util.GOLDEN_CASES (b2_24x40: nine ids, eight candidates for six
slots; b1_5x7: three candidates, all dropped) it stores the inputs (flow, seg,
occ, thr), every estimator call in order (sample, number of points, H), the
loss and dloss/dflo. Data only, a few tens of KB.
"""
from __future__ import annotations

import sys
import types
import warnings
from pathlib import Path

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hg_util  # noqa: E402


def install_cv2_stub(state):
    """``cv2.findHomography(pts1, pts2, cv2.RANSAC, thr)`` -> hg_util's least-squares stub; every call is
    appended to state["calls"] as (sample, n_points, H). The sample is the one whose flow the pairs carry."""
    cv2 = types.ModuleType("cv2")
    cv2.RANSAC = 8

    def findHomography(pts1, pts2, method, thr):  # noqa: N802 (cv2's name)
        assert method == cv2.RANSAC
        calls = []
        H, mask = hg_util.stub_estimator(calls)(pts1, pts2, thr)
        x, y = pts1[:, 0].astype(int), pts1[:, 1].astype(int)
        flow = state["flow"].numpy()
        match = [i for i in range(flow.shape[0])
                 if np.array_equal(pts1 + np.stack([flow[i, 0, y, x], flow[i, 1, y, x]], 1), pts2)]
        assert len(match) == 1, match
        state["calls"].append((match[0], len(pts1), H))
        return H, mask.astype(np.uint8)[:, None]

    cv2.findHomography = findHomography
    sys.modules["cv2"] = cv2


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = Path(sys.argv[1]).resolve()
    warnings.filterwarnings("ignore", category=UserWarning)  # the reference's meshgrid call without indexing=
    state = {"calls": [], "flow": None}
    install_cv2_stub(state)
    sys.path.insert(0, str(ref))
    from losses.loss_blocks import smooth_homography

    out = {"thr": np.float64(hg_util.GOLDEN_THR)}
    for name in hg_util.GOLDEN_CASES:
        flow, seg, occ = hg_util.golden_inputs(name)
        state["calls"], state["flow"] = [], flow
        flo = flow.clone().requires_grad_(True)
        loss = smooth_homography(flo, seg, occ, hg_util.GOLDEN_THR)
        grad = torch.zeros_like(flow)
        if loss.requires_grad:
            (grad,) = torch.autograd.grad(loss, flo)
        calls = state["calls"]
        shares = [float((hg_util.transfer_error(H, *_pairs(flow, seg, occ, s, n)) <= hg_util.GOLDEN_THR).mean())
                  for s, n, H in calls]
        assert any(s < 0.5 for s in shares), (name, shares)  # a segment whose stub inlier share is below 0.5
        out[f"{name}_flow"] = flow.numpy()
        out[f"{name}_seg"] = seg.numpy()
        out[f"{name}_occ"] = occ.numpy()
        out[f"{name}_call_sample"] = np.array([c[0] for c in calls], dtype=np.int64)
        out[f"{name}_call_npts"] = np.array([c[1] for c in calls], dtype=np.int64)
        out[f"{name}_call_H"] = np.array([c[2] for c in calls], dtype=np.float64).reshape(-1, 3, 3)
        out[f"{name}_loss"] = np.float32(loss.detach().numpy())
        out[f"{name}_grad"] = grad.numpy().astype(np.float32)
        print(name, "calls", [(c[0], c[1]) for c in calls], "shares", [round(s, 3) for s in shares],
              "loss", float(loss.detach()))
    path = HERE / "hg_smooth.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")
    assert path.stat().st_size < 128 * 1024


def _pairs(flow, seg, occ, sample, n):
    """The reliable pairs of the segment of ``sample`` with ``n`` reliable pixels (the counts are distinct)."""
    for k in range(1, int(seg.max()) + 1):
        p1, p2 = hg_util.slot_pairs(flow.numpy(), seg.numpy(), occ.numpy(), sample, k)
        if len(p1) == n:
            return p1, p2
    raise AssertionError((sample, n))


if __name__ == "__main__":
    main()
