"""Same-process A/B of the homography smoothness loss (unsamflow_amd.homography,
csrc/hg.hip) against the reference's structure: a host loop over samples and
segments with device-to-host copies and a host estimator
(homography.smooth_homography_torch).

(a) op, both directions, forward + backward, at B = 8, 256x832: segments are the
    block maps of 32 ids of harness.synthetic_pair, the flows piecewise
    homographies (one per sample and id) plus +-0.05 px noise with 10 % of the
    pixels occluded and 15 % of the rest displaced, so that segments are
    accepted. The composition is host-bound, so both paths are timed by wall
    clock around a device sync; the fused path by HIP events as well. OpenCV is
    not available, so the composition's estimator is the numpy restatement of
    the kernels' RANSAC: this is NOT cv2.findHomography's time.
(b) the whole TrainStep at B = 8, 256x832: kitti_stage2_hg() with the fused path
    and with fused_homography=False against kitti_stage1_ar(), i.e. what the
    loss adds to the step.
(c) warm graph-replay device times of the fit, the loss forward and the loss
    backward of one direction (kernel_timer.device_time_us) with algorithmic
    bytes for the dense passes.

The paths alternate in one process after a warm-up; mean (min-max) of 7. A gap is
resolved when it exceeds the larger of the two max - min spreads (the rule of
tools/segpool_ab.py), otherwise it is reported as not resolved.

``--trace-loop N`` only runs fit + loss forward + backward N times: the program
to put behind ``rocprofv3 --kernel-trace --stats`` for the per-kernel table.

Usage (GPU box, repo root): python tools/hg_ab.py [--out profiles/hg_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from unsamflow_amd import homography, ops  # noqa: E402
from unsamflow_amd.config import kitti_stage1_ar, kitti_stage2_hg  # noqa: E402
from unsamflow_amd.harness import TrainStep, synthetic_pair  # noqa: E402
from unsamflow_amd.kernel_timer import device_time_us  # noqa: E402

HBM_BYTES_PER_S = 8e12
B, H, W, K, THR = 8, 256, 832, 32, 0.5


def stats(v):
    return {"mean_ms": round(statistics.fmean(v), 4), "min_ms": round(min(v), 4),
            "median_ms": round(statistics.median(v), 4), "max_ms": round(max(v), 4),
            "runs_ms": [round(x, 4) for x in v]}


def alternate(fns, repeats, warmup):
    """{key: ([wall ms], [HIP-event ms])}: the paths of ``fns`` alternating, each run bracketed by a
    device sync (wall clock) and by HIP events."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    wall, dev = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            dev[k].append(s.elapsed_time(e))
    return wall, dev


def verdict(ms, new, old):
    a, b = stats(ms[new]), stats(ms[old])
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    gap = b["mean_ms"] - a["mean_ms"]
    return {new: a, old: b, "gap_ms": round(gap, 4), "larger_spread_ms": round(spread, 4),
            "resolved": bool(abs(gap) > spread)}


def piecewise_flow(seg, gen, noise=0.05):
    """[B,2,H,W] flow following one near-identity homography per (sample, id), occ [B,1,H,W]."""
    Bn, _, h, w = seg.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    flow = torch.zeros((Bn, 2, h, w), dtype=torch.float64)
    for b in range(Bn):
        for k in range(K):
            m = seg[b, 0] == k
            if not bool(m.any()):
                continue
            r = (torch.rand(8, generator=gen, dtype=torch.float64) * 2 - 1)
            cx, cy = xs[m].mean(), ys[m].mean()
            a, bb, c, d = 1 + 0.02 * r[0], 0.02 * r[1], 0.02 * r[2], 1 + 0.02 * r[3]
            x, y = xs[m] - cx, ys[m] - cy
            den = 1 + 1e-5 * (r[4] * x + r[5] * y)
            flow[b, 0][m] = (a * x + bb * y + 4 * r[6]) / den - x
            flow[b, 1][m] = (c * x + d * y + 4 * r[7]) / den - y
    flow += noise * (torch.rand(flow.shape, generator=gen, dtype=torch.float64) * 2 - 1)
    u = torch.rand((Bn, 1, h, w), generator=gen)
    occ = (u < 0.10).float()
    moved = ((u >= 0.10) & (u < 0.235)).expand(-1, 2, -1, -1)  # 15 % of the reliable pixels
    flow[moved] += 6.0
    return flow.float(), occ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/hg_ab.json")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true", help="skip (b), the whole training step")
    ap.add_argument("--trace-loop", type=int, default=0, help="only run fit + loss fwd + bwd this many times")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from unsamflow_amd import _lib

    gen = torch.Generator().manual_seed(11)
    img1, img2, s1, s2 = synthetic_pair(B, H, W, dev, with_seg=True, n_seg=K)
    f12, o1 = piecewise_flow(s1.cpu(), gen)
    f21, o2 = piecewise_flow(s2.cpu(), gen)
    flow4 = torch.cat([f12, f21], 1).to(dev)
    occ = [o1.to(dev), o2.to(dev)]
    segs = [s1, s2]
    one = torch.ones(1, device=dev)

    def kernels_once():
        rec = ops.hg_fit(flow4[:, :2], s1, occ[0], K, THR)
        return rec, ops.hg_loss_forward(flow4[:, :2], s1, rec), ops.hg_loss_backward(flow4[:, :2], s1, rec, one)

    if a.trace_loop:
        for _ in range(a.trace_loop):
            kernels_once()
        torch.cuda.synchronize()
        return
    if a.repeats < 5:
        sys.exit("--repeats must be at least 5")

    res = {
        "what": "homography smoothness loss: fused HIP path vs the reference's host loop with the numpy estimator "
                "(not cv2's time); wall clock around a device sync, the paths alternating in one process "
                "(tools/hg_ab.py)",
        "device": torch.cuda.get_device_name(dev),
        "build_id": _lib.build_id(),
        "repeats": a.repeats,
        "warmup": a.warmup,
        "shape": [B, 4, H, W],
        "segments": K,
        "thr": THR,
    }

    def run(fused):
        f = flow4.detach().requires_grad_(True)
        ls = [homography.smooth_homography(f[:, 2 * i:2 * i + 2], segs[i], occ[i], THR, K, fused=fused)
              for i in range(2)]
        loss = (ls[0] + ls[1]) / 2.0
        loss.backward()
        return loss.detach(), f.grad

    wall, devms = alternate({"fused": lambda: run(True), "host_loop": lambda: run(False)}, a.repeats, a.warmup)
    lf, gf = run(True)
    lh, gh = run(False)
    statuses = [homography.fit_homographies(flow4[:, 2 * i:2 * i + 2], segs[i], occ[i], THR, K)[..., 1].cpu()
                for i in range(2)]
    res["op_both_directions_fwd_bwd"] = {
        **verdict(wall, "fused", "host_loop"),
        "fused_hip_events": stats(devms["fused"]),
        "loss_fused": float(lf), "loss_host_loop": float(lh),
        "grad_max_abs_diff": float((gf - gh).abs().max()),
        "accepted_slots": int(sum(int((s == 0).sum()) for s in statuses)), "slots": 2 * B * 6,
    }
    print(json.dumps({k: v for k, v in res["op_both_directions_fwd_bwd"].items() if not isinstance(v, dict)},
                     default=str), flush=True)

    # (c) warm graph replay of the three entries, one direction
    rec = ops.hg_fit(flow4[:, :2], s1, occ[0], K, THR)
    px = B * H * W
    rows = []
    for name, fn, bpp in (("hg_fit", lambda: ops.hg_fit(flow4[:, :2], s1, occ[0], K, THR), None),
                          ("hg_loss_fwd", lambda: ops.hg_loss_forward(flow4[:, :2], s1, rec), 12),
                          ("hg_loss_bwd", lambda: ops.hg_loss_backward(flow4[:, :2], s1, rec, one), 20)):
        us = device_time_us(fn, reps=20, iters=5)
        row = {"op": name, "shape": [B, 2, H, W], "us": round(us, 2)}
        if bpp:
            row.update(bytes_per_pixel=bpp, MB=round(bpp * px / 1e6, 3),
                       hbm_fraction=round(bpp * px / (us * 1e-6) / HBM_BYTES_PER_S, 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
    res["kernels_one_direction"] = rows

    # (b) the whole step
    if not a.no_step:
        steps = {"stage1_ar": TrainStep(kitti_stage1_ar(), dev),
                 "stage2_hg_fused": TrainStep(kitti_stage2_hg(), dev),
                 "stage2_hg_host_loop": TrainStep(kitti_stage2_hg(), dev, loss_kwargs=dict(fused_homography=False))}
        wall, _ = alternate({k: (lambda k=k: steps[k](img1, img2, s1, s2)) for k in steps}, a.repeats, a.warmup)
        res["train_step_kitti_b8"] = {
            "shape": [B, 3, H, W],
            "fused_vs_stage1_ar": verdict(wall, "stage1_ar", "stage2_hg_fused"),
            "host_loop_vs_stage1_ar": verdict(wall, "stage1_ar", "stage2_hg_host_loop"),
            "fused_vs_host_loop": verdict(wall, "stage2_hg_fused", "stage2_hg_host_loop"),
        }
        for k, v in res["train_step_kitti_b8"].items():
            if isinstance(v, dict):
                print(json.dumps({k: {n: x for n, x in v.items() if not isinstance(x, dict)},
                                  **{m: v[m]["mean_ms"] for m in steps if m in v}}), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    np.set_printoptions(linewidth=200)
    print("statuses", [s.flatten().bincount(minlength=6).tolist() for s in statuses])


if __name__ == "__main__":
    main()
