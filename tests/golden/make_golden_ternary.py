"""Generate tests/golden/ternary.npz by running the REFERENCE's TernaryLoss.

Run in the survey/build container only (it imports /root/reference, which does
not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ternary.py

What it captures (the reference's own code, torch CPU fp32):
losses/loss_blocks.TernaryLoss(im, im_warp) on 4 small input pairs from the
counter-hash generator (oracle/hashrng.py), incl. the 3x5 minimum (one interior
row) and one pair multiplied by a binary visibility mask, as loss_photomatric
calls it. Inputs and outputs are stored (data only, < 64 KB).

cv2 is not importable here: a stub module is installed for import only
(TernaryLoss does not call it).
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
REF = Path("/root/reference")
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import hashrng  # noqa: E402

# name, B, H, W, masked
CASES = [("min_3x5", 1, 3, 5, False), ("odd_8x11", 2, 8, 11, False), ("even_16x24", 1, 16, 24, False),
         ("masked_9x13", 2, 9, 13, True)]


def ref_ternary():
    if str(REF) not in sys.path:
        sys.path.insert(0, str(REF))
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    from losses.loss_blocks import TernaryLoss

    return TernaryLoss


def main():
    ternary = ref_ternary()
    out = {}
    for k, (name, B, H, W, masked) in enumerate(CASES):
        im = torch.from_numpy(hashrng.uniform((B, 3, H, W), seed=9100 + 2 * k))
        im_warp = torch.from_numpy(hashrng.uniform((B, 3, H, W), seed=9101 + 2 * k))
        if masked:
            m = (torch.from_numpy(hashrng.uniform((B, 1, H, W), seed=9200 + k)) > 0.3).float()
            im, im_warp = im * m, im_warp * m
        with torch.no_grad():
            res = ternary(im, im_warp)
        out[f"{name}_im"] = im.numpy().astype(np.float32)
        out[f"{name}_im_warp"] = im_warp.numpy().astype(np.float32)
        out[f"{name}_out"] = res.numpy().astype(np.float32)
    path = HERE / "ternary.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
