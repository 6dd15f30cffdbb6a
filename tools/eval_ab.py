"""What one validation batch costs on the reference's route and on the device:
KITTI-like, B=8, prediction 256x832, ragged ground truth near 375x1242 with the
valid / noc masks (unsamflow_amd.evaluate, csrc/eval.hip).

(i)   host path vs device path, alternating in one process, each repeat
      bracketed by HIP events that end in a synchronise:
      host   = the reference's route (kitti_trainer_ar.py:396-401): the
               prediction copied to the host, then the per-sample bilinear
               resize and masked means there (flow_errors(fused=False) on the
               .cpu() tensors: the torch composition of evaluate_flow's numpy
               passes; the ground truth already lives on the host, as the
               loader leaves it);
      device = flow_errors on the device tensors (two launches, no copy). One
               call is tens of microseconds, so a repeat times --inner calls
               back to back and reports the time per call.
      min / median / max per path. No pass or fail rests on them.
(ii)  device time of the two kernels (kernel_timer.device_time_us, graph
      replay) with algorithmic bytes -- every ground-truth plane and the
      prediction read once; for the resize the prediction read and the output
      written once -- and the fraction of 8 TB/s.

Usage (GPU box, repo root): python tools/eval_ab.py [--out profiles/eval_ab.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from oracle import hashrng  # noqa: E402
from tools.ar_ab import HBM_BYTES_PER_S, stats  # noqa: E402
from unsamflow_amd import _lib, ops  # noqa: E402
from unsamflow_amd.evaluate import flow_errors  # noqa: E402
from unsamflow_amd.harness import synthetic_flow_gt  # noqa: E402
from unsamflow_amd.kernel_timer import device_time_us  # noqa: E402

KITTI_SIZES = [(375, 1242), (370, 1226), (374, 1238), (376, 1241)]


def timed_ms(fn, calls=1):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / calls, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/eval_ab.json")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=200, help="device-path calls per timed repeat")
    a = ap.parse_args()
    if a.repeats < 5:
        sys.exit("--repeats must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("tools/eval_ab.py measures on a ROCm device; none is visible")
    dev = torch.device("cuda:0")
    B, h, w = 8, 256, 832
    sizes_list = [KITTI_SIZES[b % len(KITTI_SIZES)] for b in range(B)]
    pred = (torch.from_numpy(hashrng.normal((B, 2, h, w), 21)) * 5.0).to(dev)
    gt, sizes = synthetic_flow_gt(B, sizes_list, dev, seed=22)
    gt_host, sizes_host = gt.cpu(), sizes.cpu()
    Hmax, Wmax = gt.shape[-2:]
    torch.cuda.synchronize()

    paths = {
        "host": (lambda: flow_errors(pred.cpu(), gt_host, sizes_host, fused=False), 1),
        "device": (lambda: flow_errors(pred, gt, sizes), a.inner),
    }
    for _ in range(a.warmup):
        for fn, _n in paths.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in paths}
    outs = {}
    for _ in range(a.repeats):
        for k, (fn, n) in paths.items():
            t, outs[k] = timed_ms(fn, n)
            ms[k].append(t)
    host, device = stats(ms["host"]), stats(ms["device"])
    m_host, m_dev = outs["host"][0].double(), outs["device"][0].double().cpu()
    res = {
        "what": f"one validation batch, B={B}, prediction {h}x{w}, ragged ground truth {sizes_list[:4]}... padded to "
                f"{Hmax}x{Wmax}: the reference's route (D2H copy + per-sample resize and masked means on the host) vs "
                "the fused HIP kernels; HIP events, the paths alternating in one process (tools/eval_ab.py)",
        "device": torch.cuda.get_device_name(dev),
        "host_threads": torch.get_num_threads(),
        "repeats": a.repeats,
        "warmup": a.warmup,
        "inner_device_calls": a.inner,
        "build_id": _lib.build_id(),
        "host_path": host,
        "device_path": device,
        "ratio_host_over_device": round(host["median_ms"] / device["median_ms"], 1),
        "max_rel_diff_first_five_metrics": float(((m_dev - m_host).abs() / m_host.abs())[:, :5].max()),
    }

    # (ii) per-kernel device times
    nb_eval = 4 * B * (4 * Hmax * Wmax + 2 * h * w)
    nb_resize = 4 * B * 2 * (h * w + Hmax * Wmax)
    kernels = []
    for name, fn, nbytes in (("flow_eval", lambda: ops.flow_eval(pred, gt, sizes), nb_eval),
                             ("flow_resize", lambda: ops.flow_resize(pred, sizes, Hmax, Wmax), nb_resize)):
        us = device_time_us(fn, reps=20, iters=10)
        kernels.append({"op": name, "shape": [B, h, w, Hmax, Wmax], "us": round(us, 2), "MB": round(nbytes / 1e6, 2),
                        "hbm_fraction": round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 4)})
    res["kernels"] = kernels

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"host_median_ms": host["median_ms"], "device_median_ms": device["median_ms"],
                      "host_min_max_ms": [host["min_ms"], host["max_ms"]],
                      "device_min_max_ms": [device["min_ms"], device["max_ms"]],
                      "ratio_host_over_device": res["ratio_host_over_device"],
                      "max_rel_diff_first_five_metrics": res["max_rel_diff_first_five_metrics"],
                      "kernels": kernels}), flush=True)


if __name__ == "__main__":
    main()
