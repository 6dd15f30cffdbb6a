"""Same-process A/B of the stage-1 augmentation branch at B=8, 832x256
(unsamflow_amd.ar, csrc/ar.hip) against the torch composition of the same
formulas on the GPU (ar.spatial_transform_torch / ar.ar_loss_torch) -- the
reference's Interp2 gathers and elementwise loss, never the code under test.

(i)   transform + AR loss forward + backward, fused vs torch composition: after
      a warm-up the two paths alternate, each repeat bracketed by HIP events;
      min / median / max per path.
(ii)  per-kernel device times (kernel_timer.device_time_us, graph replay) with
      algorithmic bytes and the fraction of 8 TB/s.
(iii) the whole TrainStep(kitti_stage1_ar()) both ways (fused_ar=True / False),
      alternating, from the same seed.

accepted = the fused median is below the torch composition's median by more
than the larger of the two max - min spreads (the rule of tools/census_ab.py).

Usage (GPU box, repo root): python tools/ar_ab.py [--out profiles/ar_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from oracle import hashrng  # noqa: E402
from unsamflow_amd import ar, ops  # noqa: E402
from unsamflow_amd.config import kitti_stage1_ar  # noqa: E402
from unsamflow_amd.kernel_timer import device_time_us  # noqa: E402

HBM_BYTES_PER_S = 8e12


def stats(v):
    return {"min_ms": round(min(v), 4), "median_ms": round(statistics.median(v), 4), "max_ms": round(max(v), 4),
            "runs_ms": [round(x, 4) for x in v]}


def alternate(fns, repeats, warmup):
    """{key: [ms]}: the paths of ``fns`` alternating, each run bracketed by HIP events."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e))
    return ms


def verdict(ms):
    fused, torch_path = stats(ms["fused"]), stats(ms["torch"])
    spread = max(fused["max_ms"] - fused["min_ms"], torch_path["max_ms"] - torch_path["min_ms"])
    gap = torch_path["median_ms"] - fused["median_ms"]
    return {"fused": fused, "torch_composition": torch_path, "gap_ms": round(gap, 4),
            "larger_spread_ms": round(spread, 4),
            "ratio_torch_over_fused": round(torch_path["median_ms"] / fused["median_ms"], 3),
            "accepted": bool(gap > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ar_ab.json")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip (iii), the whole training step")
    a = ap.parse_args()
    if a.repeats < 5:
        sys.exit("--repeats must be at least 5")
    dev = torch.device("cuda:0")
    B, H, W = 8, 256, 832
    cfg = kitti_stage1_ar()
    img1 = torch.from_numpy(hashrng.uniform((B, 3, H, W), 11)).to(dev)
    img2 = torch.from_numpy(hashrng.uniform((B, 3, H, W), 12)).to(dev)
    flow = (torch.from_numpy(hashrng.normal((B, 2, H, W), 13)) * 5.0).to(dev)
    mask = (torch.from_numpy(hashrng.uniform((B, 1, H, W), 14)) > 0.3).float().to(dev)
    pred = (torch.from_numpy(hashrng.normal((B, 2, H, W), 15)) * 5.0).to(dev)
    noise1 = (torch.from_numpy(hashrng.normal((B, 3, H, W), 16)) * 0.02).to(dev)
    noise2 = (torch.from_numpy(hashrng.normal((B, 3, H, W), 17)) * 0.02).to(dev)
    thetas = ar.sample_thetas(cfg.train.st_cfg, B, H, W, generator=torch.Generator().manual_seed(1))
    th_dev = thetas.to(dev)
    value = {}

    def branch(fused):
        _, _, fl, mk = ar.spatial_transform(img1, img2, flow, mask, th_dev, noise1, noise2, fused=fused)
        p = pred.clone().requires_grad_(True)
        loss = ar.ar_loss(p, fl, mk, cfg.train.ar_eps, cfg.train.ar_q, fused=fused)
        loss.backward()
        value[fused] = loss.detach()
        return p.grad

    res = {
        "what": "stage-1 augmentation branch at B=8 832x256 (kitti_stage1_ar: KITTI st_cfg thetas, ar_q 1, ar_eps 0, "
                "noise on): fused HIP path vs the torch composition on the GPU; HIP events, the two paths "
                "alternating in one process (tools/ar_ab.py)",
        "device": torch.cuda.get_device_name(dev),
        "repeats": a.repeats,
        "warmup": a.warmup,
    }
    from unsamflow_amd import _lib

    res["build_id"] = _lib.build_id()
    ab = verdict(alternate({"fused": lambda: branch(True), "torch": lambda: branch(False)}, a.repeats, a.warmup))
    ab["loss"] = {"fused": float(value[True]), "torch_composition": float(value[False])}
    res["transform_plus_loss"] = ab
    print(json.dumps({"transform_plus_loss": {k: v for k, v in ab.items() if k not in ("fused", "torch_composition")},
                      "fused_median_ms": ab["fused"]["median_ms"],
                      "torch_median_ms": ab["torch_composition"]["median_ms"]}), flush=True)

    # (ii) per-kernel device times
    fl, mk = ops.ar_transform(img1, img2, flow, mask, th_dev)[2:]
    out = ops.ar_loss_forward(pred, fl, mk, 0.0, 1.0)
    gl = torch.ones(1, device=dev)
    px = B * H * W
    sites = [
        ("ar_transform", lambda: ops.ar_transform(img1, img2, flow, mask, th_dev), 4 * 18),
        ("ar_transform+noise", lambda: ops.ar_transform(img1, img2, flow, mask, th_dev, noise1, noise2), 4 * 24),
        ("ar_loss_fwd q=1", lambda: ops.ar_loss_forward(pred, fl, mk, 0.0, 1.0), 4 * 5),
        ("ar_loss_bwd q=1", lambda: ops.ar_loss_backward(pred, fl, mk, out, gl, 0.0, 1.0), 4 * 7),
        ("ar_loss_fwd q=0.4", lambda: ops.ar_loss_forward(pred, fl, mk, 0.01, 0.4), 4 * 5),
        ("ar_loss_bwd q=0.4", lambda: ops.ar_loss_backward(pred, fl, mk, out, gl, 0.01, 0.4), 4 * 7),
        ("copy 18 planes (torch clone: the ceiling)", lambda: (img1.clone(), img2.clone(), flow.clone(),
                                                                mask.clone()), 4 * 18),
    ]
    kernels = []
    for name, fn, bpp in sites:
        us = device_time_us(fn, reps=20, iters=10)
        kernels.append({"op": name, "shape": [B, H, W], "us": round(us, 2), "bytes_per_pixel": bpp,
                        "MB": round(bpp * px / 1e6, 2),
                        "hbm_fraction": round(bpp * px / (us * 1e-6) / HBM_BYTES_PER_S, 4)})
        print(json.dumps(kernels[-1]), flush=True)
    res["kernels"] = kernels

    # (iii) the whole step
    if not a.no_step:
        from unsamflow_amd.harness import TrainStep, synthetic_pair

        s1, s2, _, _ = synthetic_pair(B, H, W, dev)
        steps = {"fused": TrainStep(cfg, dev, fused_ar=True), "torch": TrainStep(cfg, dev, fused_ar=False)}
        sv = verdict(alternate({k: (lambda st=st: st(s1, s2)) for k, st in steps.items()}, a.repeats, a.warmup))
        res["train_step"] = sv
        print(json.dumps({"train_step": {k: v for k, v in sv.items() if k not in ("fused", "torch_composition")},
                          "fused_median_ms": sv["fused"]["median_ms"],
                          "torch_median_ms": sv["torch_composition"]["median_ms"]}), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
