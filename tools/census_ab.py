"""Same-process A/B of the stage-1 loss: unFlowLoss(kitti_stage1().loss) forward
+ backward at B=8, 832x256 with the fused census op (unsamflow_amd.census,
csrc/census.hip) against fused_photometric=False -- the library warp under
torch's census composition, the path before the fused op existed.

The flows are the five synthetic pyramid flows of
tests/test_gpu_photometric.py::test_photometric_loss_in_unflowloss_matches_torch_path.
After a warm-up the two paths alternate, each repeat bracketed by HIP events;
min / median / max per path go to --out, with the per-scale device times of the
new pair kernels (kernel_timer.device_time_us, graph replay), their algorithmic
bytes per pixel and fraction of 8 TB/s.

accepted = the fused median is below the torch-path median by more than the
larger of the two max - min spreads.

Usage (GPU box, repo root): python tools/census_ab.py [--out profiles/census_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from oracle import hashrng  # noqa: E402
from unsamflow_amd.config import kitti_stage1  # noqa: E402
from unsamflow_amd.flow_loss import unFlowLoss  # noqa: E402
from unsamflow_amd.kernel_timer import device_time_us, site_launcher  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/census_ab.json")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if a.repeats < 5:
        sys.exit("--repeats must be at least 5")
    dev = torch.device("cuda:0")
    B, H, W = 8, 256, 832
    img1 = torch.from_numpy(hashrng.uniform((B, 3, H, W), 11)).to(dev)
    img2 = torch.from_numpy(hashrng.uniform((B, 3, H, W), 12)).to(dev)
    flows = [torch.from_numpy(hashrng.symmetric((B, 4, H >> i, W >> i), 20 + i, 3.0 / (1 << i))).to(dev)
             for i in range(5)]
    cfg = kitti_stage1().loss
    losses = {True: unFlowLoss(cfg, fused_photometric=True), False: unFlowLoss(cfg, fused_photometric=False)}

    def step(fused):
        fl = [f.clone().requires_grad_(True) for f in flows]
        loss = losses[fused](fl, img1, img2)[0].sum()
        loss.backward()
        return loss

    value = {}
    for _ in range(a.warmup):
        for fused in (True, False):
            value[fused] = float(step(fused))
    torch.cuda.synchronize()
    ms = {True: [], False: []}
    for _ in range(a.repeats):
        for fused in (True, False):  # the two paths alternate
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            step(fused)
            e.record()
            e.synchronize()
            ms[fused].append(s.elapsed_time(e))

    def stats(v):
        return {"min_ms": round(min(v), 4), "median_ms": round(statistics.median(v), 4), "max_ms": round(max(v), 4),
                "runs_ms": [round(x, 4) for x in v]}

    fused, torch_path = stats(ms[True]), stats(ms[False])
    spread = max(fused["max_ms"] - fused["min_ms"], torch_path["max_ms"] - torch_path["min_ms"])
    gap = torch_path["median_ms"] - fused["median_ms"]

    kernels = []
    for op, ndir_planes in (("census_pair_grad", 4), ("census_pair", 0)):
        for i in range(4):
            key = (B, 3, H >> i, W >> i, "border")
            if op == "census_pair" and i:
                continue
            us = device_time_us(site_launcher(op, key, dev), reps=20, iters=10)
            bpp = 4 * (2 * 3 + 4 + 2 + ndir_planes)  # both images, the 4-channel flow, two masks, the basis
            nbytes = bpp * B * key[2] * key[3]
            kernels.append({"op": op, "shape": list(key), "us": round(us, 2), "bytes_per_pixel": bpp,
                            "hbm_fraction": round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 4)})
            print(json.dumps(kernels[-1]), flush=True)
    for i in range(4):
        key = (B, 2, H >> i, W >> i)
        us = device_time_us(site_launcher("census_bwd", key, dev), reps=20, iters=10)
        nbytes = 4 * 8 * B * key[2] * key[3]
        kernels.append({"op": "census_bwd", "shape": list(key), "us": round(us, 2), "bytes_per_pixel": 32,
                        "hbm_fraction": round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 4)})
        print(json.dumps(kernels[-1]), flush=True)
    hw4 = tuple(v for i in range(4) for v in (H >> i, W >> i))
    for op, key in (("census_pyr_grad", (B, 3) + hw4 + ("border",)), ("census_pyr_bwd", (B, 2) + hw4)):
        us = device_time_us(site_launcher(op, key, dev), reps=20, iters=10)
        kernels.append({"op": op, "shape": list(key), "us": round(us, 2)})
        print(json.dumps(kernels[-1]), flush=True)

    from unsamflow_amd import _lib

    res = {
        "what": "unFlowLoss(kitti_stage1().loss) forward + backward, B=8 832x256, five synthetic pyramid flows: "
                "fused census op vs fused_photometric=False (library warp + torch census composition); "
                "HIP events, the two paths alternating in one process (tools/census_ab.py)",
        "build_id": _lib.build_id(),
        "device": torch.cuda.get_device_name(dev),
        "repeats": a.repeats,
        "warmup": a.warmup,
        "loss": {"fused": value[True], "torch_path": value[False]},
        "fused": fused,
        "torch_path": torch_path,
        "gap_ms": round(gap, 4),
        "larger_spread_ms": round(spread, 4),
        "ratio_torch_over_fused": round(torch_path["median_ms"] / fused["median_ms"], 3),
        "accepted": bool(gap > spread),
        "kernels": kernels,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("fused", "torch_path", "gap_ms", "larger_spread_ms",
                                          "ratio_torch_over_fused", "accepted")}))


if __name__ == "__main__":
    main()
