"""Same-process A/B of the key-object augmentation at KITTI B=8, 256x832, K=3,
crop 192x640, with a cache of 100 objects on the device
(unsamflow_amd.fake_object, csrc/fakeobj.hip) against the torch composition of
the same formulas on the GPU (fake_object.add_fake_object, then the slice).

(i)   paste + crop, fused vs torch composition + slice: after a warm-up the
      paths alternate, each repeat bracketed by HIP events; min / median / max
      per path. The reference arrangement (the cache on the host, the popped
      objects gathered and mirrored there and copied to the device every step,
      then the composition) alternates with them and is reported as its own row.
(ii)  device time of both kernels (kernel_timer.device_time_us, graph replay)
      with algorithmic bytes -- 4 B ch cw (18 + 8 K) for paste + crop (each base
      tensor read and written once; per object 4 floats at the pixel and 4 at
      the shifted position), 4 B H W (4 + 2 + 4) for the push -- and the
      fraction of 8 TB/s.
(iii) the whole TrainStep(kitti_aug_hg()) with a pre-filled cache,
      fused_fake_object True vs False, alternating, from the same seed.

accepted = the fused median is below the torch composition's median by more
than the larger of the two max - min spreads (the rule of tools/census_ab.py).

Usage (GPU box, repo root): python tools/fakeobj_ab.py [--out profiles/fakeobj_ab.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from oracle import hashrng  # noqa: E402
from tools.ar_ab import HBM_BYTES_PER_S, alternate, stats, verdict  # noqa: E402
from unsamflow_amd import fake_object as fo  # noqa: E402
from unsamflow_amd import ops  # noqa: E402
from unsamflow_amd.config import kitti_aug_hg  # noqa: E402
from unsamflow_amd.harness import synthetic_key_objects  # noqa: E402
from unsamflow_amd.kernel_timer import device_time_us  # noqa: E402


def fill(cache, B, H, W, dev, seed):
    """Push synthetic key objects (frames U[0,1), flows of a few px) until the cache is full."""
    i = 0
    while cache.count < cache.cache_size:
        mask, valid = synthetic_key_objects(B, H, W, dev, seed=seed + i, p_invalid=0.0)
        img = torch.from_numpy(hashrng.uniform((B, 3, H, W), seed + 100 + i)).to(dev)
        flow = (torch.from_numpy(hashrng.normal((B, 2, 1, 1), seed + 200 + i)) * 6.0).to(dev).expand(B, 2, H, W)
        cache.push(mask, img, flow.contiguous(), valid)
        i += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/fakeobj_ab.json")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="skip (iii), the whole training step")
    a = ap.parse_args()
    if a.repeats < 5:
        sys.exit("--repeats must be at least 5")
    dev = torch.device("cuda:0")
    B, H, W, K, crop, N = 8, 256, 832, 3, (192, 640), 100
    offsets = (37, 101)
    img1 = torch.from_numpy(hashrng.uniform((B, 3, H, W), 11)).to(dev)
    img2 = torch.from_numpy(hashrng.uniform((B, 3, H, W), 12)).to(dev)
    flow = (torch.from_numpy(hashrng.normal((B, 2, H, W), 13)) * 5.0).to(dev)
    noc = (torch.from_numpy(hashrng.uniform((B, 1, H, W), 14)) > 0.3).float().to(dev)
    g = torch.Generator().manual_seed(1)
    cache = fo.ObjectCache(N, dev, generator=g)
    fill(cache, B, H, W, dev, 500)
    slots, params = cache.pop(K * B)
    host = [t.cpu() for t in (cache.obj_mask, cache.img, cache.motion)]  # the reference keeps its cache here
    torch.cuda.synchronize()

    def reference_arrangement():
        idx = slots.long()
        mask, img, motion = host[0][idx], host[1][idx], host[2][idx] * params[:, :2]
        flip = params[:, 2] != 0
        img[flip] = img[flip].flip(dims=[3])
        mask[flip] = mask[flip].flip(dims=[3])
        return fo.paste_and_crop_torch(img1, img2, flow, noc, mask.to(dev), img.to(dev), motion.to(dev), crop,
                                       offsets)[:3]

    from unsamflow_amd import _lib

    res = {
        "what": f"key-object augmentation at B={B} {H}x{W}, K={K}, crop {crop[0]}x{crop[1]}, cache of {N} on the "
                "device: fused HIP paste + crop vs the torch composition + slice on the GPU; HIP events, the "
                "paths alternating in one process (tools/fakeobj_ab.py)",
        "device": torch.cuda.get_device_name(dev),
        "repeats": a.repeats,
        "warmup": a.warmup,
        "build_id": _lib.build_id(),
    }
    paths = {
        "fused": lambda: fo.paste_and_crop(img1, img2, flow, noc, cache, slots, params, crop, offsets, fused=True),
        "torch": lambda: fo.paste_and_crop(img1, img2, flow, noc, cache, slots, params, crop, offsets, fused=False),
        "reference": reference_arrangement,
    }
    outs = {k: fn() for k, fn in paths.items()}
    ms = alternate(paths, a.repeats, a.warmup)
    ab = verdict(ms)
    ab["reference_arrangement_host_cache_h2d"] = stats(ms["reference"])
    ab["h2d_MB_per_step_reference"] = round(4 * K * B * 4 * H * W / 1e6, 1)
    ab["max_abs_diff_fused_vs_torch"] = [float((x - y).abs().max()) for x, y in zip(outs["fused"], outs["torch"])]
    res["paste_crop"] = ab
    print(json.dumps({"paste_crop": {k: v for k, v in ab.items() if not isinstance(v, dict)},
                      "fused_median_ms": ab["fused"]["median_ms"],
                      "torch_median_ms": ab["torch_composition"]["median_ms"],
                      "reference_median_ms": ab["reference_arrangement_host_cache_h2d"]["median_ms"]}), flush=True)

    # (ii) per-kernel device times
    sd, pd = slots.to(dev), params.to(dev)
    mask, valid = synthetic_key_objects(B, H, W, dev, seed=900, p_invalid=0.0)
    push_slots = torch.arange(B, dtype=torch.int32, device=dev)
    ch, cw = crop
    sites = [
        ("fakeobj_paste_crop", lambda: ops.fakeobj_paste_crop(img1, img2, flow, noc, cache.obj_mask, cache.img,
                                                              cache.motion, sd, pd, crop, offsets),
         4 * B * ch * cw * (18 + 8 * K)),
        ("fakeobj_push", lambda: ops.fakeobj_push(mask, img1, flow, push_slots, cache.obj_mask, cache.img,
                                                  cache.motion), 4 * B * H * W * (4 + 2 + 4)),
    ]
    kernels = []
    for name, fn, nbytes in sites:
        us = device_time_us(fn, reps=20, iters=10)
        kernels.append({"op": name, "shape": [B, H, W], "us": round(us, 2), "MB": round(nbytes / 1e6, 2),
                        "hbm_fraction": round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 4)})
        print(json.dumps(kernels[-1]), flush=True)
    res["kernels"] = kernels

    # (iii) the whole step
    if not a.no_step:
        from unsamflow_amd.harness import TrainStep, synthetic_pair

        cfg = kitti_aug_hg()
        s1, s2, seg1, seg2 = synthetic_pair(B, H, W, dev, with_seg=True)
        steps = {}
        for key, fused in (("fused", True), ("torch", False)):
            st = TrainStep(cfg, dev, fused_fake_object=fused, obj_cache_size=N)
            fill(st.obj_cache, B, H, W, dev, 500)
            steps[key] = st
        sv = verdict(alternate({k: (lambda st=st: st(s1, s2, seg1, seg2, key_obj_mask=mask, key_obj_valid=valid))
                                for k, st in steps.items()}, a.repeats, a.warmup))
        res["train_step"] = sv
        print(json.dumps({"train_step": {k: v for k, v in sv.items() if k not in ("fused", "torch_composition")},
                          "fused_median_ms": sv["fused"]["median_ms"],
                          "torch_median_ms": sv["torch_composition"]["median_ms"]}), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
