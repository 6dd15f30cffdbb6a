"""Same-process A/B of the mask-feature branch's per-segment max pool and spread
(unsamflow_amd.segpool, csrc/segpool.hip) against the torch composition of the
reference's three lines on the GPU (segpool.segment_max_spread_torch).

(a) op forward + backward, fused vs composition, at the five Sintel decoder
    shapes at batch 16 (32 channels, 7x16 ... 112x256) for K = 32 and K = 128:
    after a warm-up the two paths alternate, each repeat bracketed by HIP
    events; mean / min / median / max per path.
(b) torch.cuda.max_memory_allocated of both paths in (a), beyond the inputs.
(c) the whole TrainStep(sintel_mf()) at B = 8, 448x1024, with both model
    switches off, with FUSED_SEG_POOL on, and with SHARED_MASK_FEATURE on too.
(d) warm graph-replay device times of the new kernels (kernel_timer.device_time_us)
    with algorithmic bytes -- (8C + 4) B/pixel forward, (12C + 8) backward -- and
    the fraction of 8 TB/s.

accepted = the faster path's mean is below the other's by more than the larger
of the two max - min spreads (the rule of tools/census_ab.py and ar_ab.py); a
gap that does not exceed the spread is reported as such.

Usage (GPU box, repo root): python tools/segpool_ab.py [--out profiles/segpool_ab.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from unsamflow_amd import ops, pwclite, segpool  # noqa: E402
from unsamflow_amd.config import sintel_mf  # noqa: E402
from unsamflow_amd.kernel_timer import device_time_us  # noqa: E402

HBM_BYTES_PER_S = 8e12
LEVELS = [(7, 16), (14, 32), (28, 64), (56, 128), (112, 256)]  # Sintel 448x1024, L0 .. L4


def stats(v):
    return {"mean_ms": round(statistics.fmean(v), 4), "min_ms": round(min(v), 4),
            "median_ms": round(statistics.median(v), 4), "max_ms": round(max(v), 4),
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


def verdict(ms, new, old):
    a, b = stats(ms[new]), stats(ms[old])
    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
    gap = b["mean_ms"] - a["mean_ms"]
    return {new: a, old: b, "gap_ms": round(gap, 4), "larger_spread_ms": round(spread, 4),
            f"ratio_{old}_over_{new}": round(b["mean_ms"] / a["mean_ms"], 3), "accepted": bool(gap > spread),
            "gap_exceeds_spread": bool(abs(gap) > spread)}


def brief(v):
    return {k: x for k, x in v.items() if not isinstance(x, dict)}


def segments(B, h, w, K, gen):
    """Piecewise-constant ids as harness.synthetic_pair makes them (32-pixel
    blocks at full resolution, nearest-resized to the level)."""
    H, W = 448, 1024
    ids = torch.randint(0, K, (B, 1, H // 32, W // 32), generator=gen).float()
    full = ids.repeat_interleave(32, 2).repeat_interleave(32, 3)
    return torch.nn.functional.interpolate(full, (h, w), mode="nearest").contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/segpool_ab.json")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip (c), the whole training step")
    a = ap.parse_args()
    if a.repeats < 5:
        sys.exit("--repeats must be at least 5")
    dev = torch.device("cuda:0")
    from unsamflow_amd import _lib

    res = {
        "what": "mask-feature per-segment max pool + spread: fused HIP path vs the torch one-hot composition on the "
                "GPU; HIP events, the paths alternating in one process (tools/segpool_ab.py)",
        "device": torch.cuda.get_device_name(dev),
        "build_id": _lib.build_id(),
        "repeats": a.repeats,
        "warmup": a.warmup,
    }
    B, C = 16, 32
    gen = torch.Generator().manual_seed(7)
    op_rows, kernel_rows = [], []
    for K in (32, 128):
        for lvl, (h, w) in enumerate(LEVELS):
            proj = torch.randn((B, C, h, w), generator=gen).to(dev)
            seg = segments(B, h, w, K, gen).to(dev)
            gs = torch.randn((B, C, h, w), generator=gen).to(dev)

            def run(fused):
                p = proj.detach().requires_grad_(True)
                out = segpool.segment_max_spread(p, seg, K, fused=fused)
                out.backward(gs)
                return out, p.grad

            ab = verdict(alternate({"fused": lambda: run(True), "torch": lambda: run(False)}, a.repeats, a.warmup),
                         "fused", "torch")
            mem = {}
            for name, fused in (("fused", True), ("torch", False)):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                out = run(fused)
                torch.cuda.synchronize()
                mem[name] = torch.cuda.max_memory_allocated(dev) - base
                del out
            fo, fg = run(True)
            to, tg = run(False)
            row = {"level": lvl, "shape": [B, C, h, w], "K": K, **ab,
                   "max_memory_allocated_beyond_inputs_bytes": mem,
                   "proj_bytes": proj.numel() * 4,
                   "spread_equal": bool(torch.equal(fo, to)),
                   "grad_max_abs_diff": float((fg - tg).abs().max())}
            op_rows.append(row)
            print(json.dumps({"level": lvl, "K": K, **brief(ab), "fused_mean_ms": ab["fused"]["mean_ms"],
                              "torch_mean_ms": ab["torch"]["mean_ms"], "mem": mem}), flush=True)

            # (d) the kernels alone, warm graph replay
            spread, state = ops.segpool_forward(proj, seg, K)
            px = B * h * w
            for name, fn, bpp in (("segpool_fwd", lambda: ops.segpool_forward(proj, seg, K), 8 * C + 4),
                                  ("segpool_bwd", lambda: ops.segpool_backward(proj, seg, state, gs, K), 12 * C + 8)):
                us = device_time_us(fn, reps=20, iters=10)
                kernel_rows.append({"op": name, "shape": [B, C, h, w], "K": K, "us": round(us, 2),
                                    "bytes_per_pixel": bpp, "MB": round(bpp * px / 1e6, 3),
                                    "hbm_fraction": round(bpp * px / (us * 1e-6) / HBM_BYTES_PER_S, 4)})
                print(json.dumps(kernel_rows[-1]), flush=True)
            del proj, seg, gs, spread, state, fo, fg, to, tg
    res["op_fwd_bwd"] = op_rows
    res["kernels"] = kernel_rows

    # (c) the whole step
    if not a.no_step:
        from unsamflow_amd.harness import TrainStep, synthetic_pair

        Bs, H, W = 8, 448, 1024
        img1, img2, s1, s2 = synthetic_pair(Bs, H, W, dev, with_seg=True)
        modes = {"both_off": (False, False), "pool": (True, False), "pool_and_shared": (True, True)}
        steps = {k: TrainStep(sintel_mf(), dev) for k in modes}
        saved = pwclite.FUSED_SEG_POOL, pwclite.SHARED_MASK_FEATURE

        def step(k):
            pwclite.FUSED_SEG_POOL, pwclite.SHARED_MASK_FEATURE = modes[k]
            return steps[k](img1, img2, s1, s2)

        try:
            ms = alternate({k: (lambda k=k: step(k)) for k in modes}, a.repeats, a.warmup)
        finally:
            pwclite.FUSED_SEG_POOL, pwclite.SHARED_MASK_FEATURE = saved
        sv = {"shape": [Bs, 3, H, W], "segments": 32,
              "pool_vs_both_off": verdict(ms, "pool", "both_off"),
              "pool_and_shared_vs_pool": verdict(ms, "pool_and_shared", "pool"),
              "pool_and_shared_vs_both_off": verdict(ms, "pool_and_shared", "both_off")}
        res["train_step_sintel_mf_b8"] = sv
        for k in list(sv)[2:]:
            print(json.dumps({k: brief(sv[k]), **{m: sv[k][m]["mean_ms"] for m in modes if m in sv[k]}}), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
