"""Generate tests/golden/fake_object.npz by running the REFERENCE's
add_fake_object (transforms/ar_transforms/oc_transforms.py) and ObjectCache
(trainer/object_cache.py).

Run where a checkout of the reference is at hand (it is imported, never copied):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fakeobj.py /path/to/reference

What it captures (the reference's own code, torch CPU fp32, data only, < 128 KB):

(a) ``<case>_img1`` / ``_img2`` / ``_flow`` / ``_noc`` / ``_newmask``: K = 3 rounds
    of add_fake_object on B = 2 at 2x3, 13x21 and 17x38, chained as the trainer
    chains them (object k B + b goes to sample b in round k), with dummy segment
    maps. The motions are fractional, exactly integer, zero and wholly out of
    frame; all masks contain the image centre, one has fractional values.
(b) ``counts``: ObjectCache(cache_size=5).count after pushes of 2 objects each
    (room, room, partial fill, full, full), and ``pop_before_full``.
(c) ``pop_*``: ObjectCache.pop(4, with_aug=True) on a full cache of 5 objects of
    3x4 with its random numbers injected (``pop_idx`` for np.random.choice,
    ``pop_scale`` / ``pop_sign`` / ``pop_flip`` for the three torch.rand calls,
    one of them flipped, one reversed) -> ``pop_mask``, ``pop_img``, ``pop_motion``;
    ``pop_cache_unchanged`` records that the cache was bit-identical afterwards.

The inputs are not stored: tests/fakeobj_util regenerates them from
``<case>_shape`` and ``<case>_seed`` (oracle/hashrng.py).
"""
from __future__ import annotations

import sys
from pathlib import Path

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fakeobj_util  # noqa: E402

K = 3
# name, B, H, W, seed
CASES = [("min_2x3", 2, 2, 3, 9400), ("odd_13x21", 2, 13, 21, 9410), ("wide_17x38", 2, 17, 38, 9420)]
POP_SEED, POP_N, POP_HW = 9430, 5, (3, 4)
POP_IDX = [3, 0, 4, 1]
POP_SCALE = [0.0, 0.25, 0.5, 0.999]
POP_SIGN = [0.1, 0.9, 0.4, 0.6]
POP_FLIP = [0.2, 0.7, 0.8, 0.3]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = Path(sys.argv[1]).resolve()
    sys.path.insert(0, str(ref))
    from trainer import object_cache as ref_cache
    from transforms.ar_transforms.oc_transforms import add_fake_object

    out = {"K": np.int64(K)}
    for name, B, H, W, seed in CASES:
        img1, img2, flow, noc = fakeobj_util.base(B, H, W, seed)
        mask, src, motion = fakeobj_util.objects(K * B, H, W, seed + 5)
        seg1 = seg2 = torch.ones(B, 1, H, W)
        with torch.no_grad():
            for k in range(K):
                r = slice(k * B, (k + 1) * B)
                img1, img2, seg1, seg2, flow, noc, newmask = add_fake_object({
                    "img1_tgt": img1, "img2_tgt": img2, "full_seg1_st": seg1, "full_seg2_st": seg2,
                    "flow_tgt": flow, "noc_tgt": noc, "img_src": src[r], "obj_mask": mask[r], "motion": motion[r]})
        out[f"{name}_shape"] = np.array([B, H, W], dtype=np.int64)
        out[f"{name}_seed"] = np.int64(seed)
        for k, v in (("img1", img1), ("img2", img2), ("flow", flow), ("noc", noc), ("newmask", newmask)):
            out[f"{name}_{k}"] = v.numpy().astype(np.float32)

    # (b) count transitions
    c = ref_cache.ObjectCache(cache_size=5)
    counts, before_full = [], []
    np.random.seed(0)
    for i in range(5):
        m, im, mo = fakeobj_util.objects(2, *POP_HW, POP_SEED + 10 * i)
        c.push(m, im, mo)
        counts.append(c.count)
        before_full.append(c.pop(2) is None)
    out["counts"] = np.array(counts, dtype=np.int64)
    out["pop_before_full"] = np.array(before_full)

    # (c) the pop arithmetic with injected random numbers
    m, im, mo = fakeobj_util.objects(POP_N, *POP_HW, POP_SEED)
    c = ref_cache.ObjectCache(cache_size=POP_N)
    c.push(m, im, mo)
    assert c.count == POP_N
    snap = [t.clone() for t in (c._obj_mask_cache, c._img_cache, c._motion_cache)]
    draws = iter([torch.tensor(v) for v in (POP_SCALE, POP_SIGN, POP_FLIP)])
    real_rand, real_choice = torch.rand, np.random.choice
    torch.rand = lambda n: next(draws)
    np.random.choice = lambda size, n, replace: np.array(POP_IDX)
    try:
        pm, pi, pmo = c.pop(len(POP_IDX), with_aug=True)
    finally:
        torch.rand, np.random.choice = real_rand, real_choice
    unchanged = all(torch.equal(a, b) for a, b in zip(snap, (c._obj_mask_cache, c._img_cache, c._motion_cache)))
    out.update(pop_seed=np.int64(POP_SEED), pop_n=np.int64(POP_N), pop_hw=np.array(POP_HW, dtype=np.int64),
               pop_idx=np.array(POP_IDX, dtype=np.int64), pop_scale=np.array(POP_SCALE, dtype=np.float32),
               pop_sign=np.array(POP_SIGN, dtype=np.float32), pop_flip=np.array(POP_FLIP, dtype=np.float32),
               pop_mask=pm.numpy(), pop_img=pi.numpy(), pop_motion=pmo.numpy(),
               pop_cache_unchanged=np.array(unchanged))
    path = HERE / "fake_object.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes", "counts", counts, "unchanged", unchanged)
    assert path.stat().st_size < 128 * 1024


if __name__ == "__main__":
    main()
