"""Shared inputs of tests/test_fake_object_cpu.py, tests/test_gpu_fake_object.py
and tests/golden/make_golden_fakeobj.py: base tensors and objects regenerated
from seeds (oracle/hashrng.py), and a cache filled with given objects."""
import torch

import ar_util
from oracle import hashrng


def base(B: int, H: int, W: int, seed: int):
    """img1, img2 in [0, 1), a flow of std 5 px, a binary noc (fp32, CPU)."""
    return ar_util.inputs(B, H, W, seed)


def motions(n: int, H: int, W: int) -> torch.Tensor:
    """[n,2]: fractional, exactly integer, zero, wholly out of frame, then fractional ones."""
    fixed = [(1.3, -0.7), (2.0, -1.0), (0.0, 0.0), (3.0 * W, 0.0), (-0.45, 0.6), (0.25, 1.75)]
    rows = [fixed[j] if j < len(fixed) else (0.37 * (j - 4), -0.21 * (j - 3)) for j in range(n)]
    return torch.tensor(rows, dtype=torch.float32)


def objects(n: int, H: int, W: int, seed: int):
    """(obj_mask [n,1,H,W], img_src [n,3,H,W], motion [n,2]): rectangles that all
    contain the image centre (so the rounds overlap); object 1 has fractional
    mask values; the motions are :func:`motions`."""
    img = torch.from_numpy(hashrng.uniform((n, 3, H, W), seed))
    mask = torch.zeros(n, 1, H, W)
    for j in range(n):
        ya, yb = (j % 3) * H // 6, H - ((j + 1) % 3) * H // 6
        xa, xb = (j % 2) * W // 5, W - ((j + 1) % 2) * W // 4
        mask[j, 0, ya:yb, xa:xb] = 1.0
    if n > 1:
        mask[1] *= torch.from_numpy(hashrng.uniform((1, H, W), seed + 1))
    return mask, img, motions(n, H, W)


def filled_cache(mask, img, motion, device="cpu", cache_size=None):
    """An ObjectCache whose slot j holds object j (full unless cache_size > n)."""
    from unsamflow_amd.fake_object import ObjectCache

    n = mask.shape[0]
    c = ObjectCache(cache_size or n, device)
    c._init_cache(*mask.shape[-2:], device)
    c.obj_mask[:n] = mask.to(device)
    c.img[:n] = img.to(device)
    c.motion[:n] = motion.to(device)
    c.count = n
    return c


def plain_params(n: int, flips=None) -> torch.Tensor:
    """[n,4] host params with unit scale; ``flips`` marks mirrored objects."""
    p = torch.tensor([1.0, 1.0, 0.0, 0.0]).repeat(n, 1)
    for j in flips or []:
        p[j, 0], p[j, 2] = -1.0, 1.0
    return p
