"""Shared inputs of tests/test_ar_cpu.py, tests/test_gpu_ar.py and
tests/golden/make_golden_ar.py: explicit thetas (one sample mirrored, part of
every output outside its source) and counter-hash inputs regenerated from seeds."""
import math

import numpy as np
import torch

from oracle import hashrng


def mk(z, phi, tx, ty, s):
    """theta of zoom z, rotation phi, translation (tx, ty); s = -1 mirrors x."""
    return [s * z * math.cos(phi), s * z * math.sin(phi), s * tx, -z * math.sin(phi), z * math.cos(phi), ty]


THETA1 = [mk(0.8, 0.3, 0.1, -0.05, 1), mk(1.2, -0.02, 0.02, 0.01, -1), mk(1.1, 0.15, -0.06, 0.04, 1)]
THETA2 = [mk(0.82, 0.31, 0.11, -0.05, 1), mk(1.21, -0.025, 0.021, 0.012, -1), mk(1.11, 0.16, -0.055, 0.045, 1)]
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def explicit_thetas(B: int, shift: float = 0.0) -> torch.Tensor:
    """[2,B,6] float32: sample b takes pair b % 3; ``shift`` nudges the x translation."""
    t = torch.tensor([[THETA1[b % 3] for b in range(B)], [THETA2[b % 3] for b in range(B)]], dtype=torch.float64)
    t[:, :, 2] += shift
    return t.float()


def identity_thetas(B: int) -> torch.Tensor:
    return torch.tensor([[IDENTITY] * B] * 2, dtype=torch.float32)


def inputs(B: int, H: int, W: int, seed: int, lo: float = 0.0):
    """img1, img2 in [lo, 1), a flow of std 5 px, a binary mask (fp32, CPU)."""
    img1 = torch.from_numpy(hashrng.uniform((B, 3, H, W), seed)) * (1.0 - lo) + lo
    img2 = torch.from_numpy(hashrng.uniform((B, 3, H, W), seed + 1)) * (1.0 - lo) + lo
    flow = torch.from_numpy(hashrng.normal((B, 2, H, W), seed + 2)) * 5.0
    mask = (torch.from_numpy(hashrng.uniform((B, 1, H, W), seed + 3)) > 0.3).float()
    return img1, img2, flow, mask


def edge_distance(theta: torch.Tensor, H: int, W: int) -> np.ndarray:
    """[B,H,W] fp64: distance (px) of every output pixel's source coordinate under
    ``theta`` [B,6] from the nearest validity edge (x = 0, x = W, y = 0, y = H)."""
    from unsamflow_amd.ar import transform_coords

    xq, yq = transform_coords(theta.double(), H, W)
    d = torch.stack([xq.abs(), (xq - W).abs(), yq.abs(), (yq - H).abs()]).min(0).values
    return d.numpy()


def zeroed_fraction(theta: torch.Tensor, H: int, W: int) -> np.ndarray:
    """[B]: share of output pixels whose source coordinate lies outside."""
    from unsamflow_amd.ar import transform_coords

    xq, yq = transform_coords(theta.double(), H, W)
    return ((xq < 0) | (xq >= W) | (yq < 0) | (yq >= H)).double().mean(dim=(1, 2)).numpy()


def clear_thetas(B: int, H: int, W: int, margin: float = 2e-3) -> torch.Tensor:
    """explicit_thetas(B), its x translation nudged in steps of 0.003 until no
    output pixel's source coordinate (either frame) is within ``margin`` px of
    a validity edge: a rounding error cannot then flip a pixel's validity."""
    for i in range(100):
        th = explicit_thetas(B, 0.003 * i)
        if min(edge_distance(th[k], H, W).min() for k in range(2)) >= margin:
            return th
    raise AssertionError(f"no clear theta for {(B, H, W)}")
