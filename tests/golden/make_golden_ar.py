"""Generate tests/golden/ar_transform.npz by running the REFERENCE's
RandomAffineFlow (transforms/ar_transforms/sp_transforms.py, interpolation.py).

Run where a checkout of the reference is at hand (it is imported, never copied):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ar.py /path/to/reference

What it captures (the reference's own code, torch CPU fp32, data only, < 128 KB):

(a) ``thetas_kitti`` / ``thetas_sintel`` [2,4,6]: the theta lists of
    RandomAffineFlow.forward (apply_random_transforms_to_params for the global
    and the relative transform, then the random mirror) under
    torch.manual_seed(SEED) for the st_cfg of configs/kitti_base.json and
    configs/sintel_base.json (squeeze, vflip, +-0.2 rad) at B = 4, 256x832 /
    448x1024.
(b) ``<case>_img1_t`` / ``_img2_t`` / ``_flow_t`` / ``_mask_t``: transform_image
    and transform_flow called with the explicit thetas ``<case>_thetas`` on
    B = 2 inputs of 2x3, 12x20 and 17x38. Part of sample 0's output lies outside
    its source, sample 1 is mirrored, and no pixel's source coordinate is within
    1e-3 px of a validity edge (asserted; the x translation is nudged if not).
(c) one identity-theta case (12x20, inputs in [0.1, 1)).

The inputs are not stored: tests/ar_util.inputs regenerates them from
``<case>_shape`` and ``<case>_seed`` (oracle/hashrng.py).
"""
from __future__ import annotations

import sys
import warnings
from pathlib import Path

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ar_util  # noqa: E402
from unsamflow_amd import config  # noqa: E402

SEED = 1234
THETA_CASES = [("kitti", config.kitti_stage1_ar, 256, 832), ("sintel", config.sintel_stage1_ar, 448, 1024)]
# name, B, H, W, seed, identity
CASES = [("min_2x3", 2, 2, 3, 9300, False), ("odd_12x20", 2, 12, 20, 9310, False),
         ("wide_17x38", 2, 17, 38, 9320, False), ("identity_12x20", 2, 12, 20, 9330, True)]


def ref_module(ref: Path, st_cfg):
    if str(ref) not in sys.path:
        sys.path.insert(0, str(ref))
    from transforms.ar_transforms.sp_transforms import RandomAffineFlow

    return RandomAffineFlow(st_cfg, addnoise=False)


def ref_thetas(m, B, H, W):
    """The theta part of the reference's RandomAffineFlow.forward for two frames."""
    c = m.cfg
    lst = [m.apply_random_transforms_to_params(
        m._identity(B), max_translate=c.trans[0], min_zoom=c.zoom[0], max_zoom=c.zoom[1], min_squeeze=c.squeeze[0],
        max_squeeze=c.squeeze[1], min_rotate=c.rotate[0], max_rotate=c.rotate[1], validate_size=[H, W])]
    lst.append(m.apply_random_transforms_to_params(
        lst[-1], max_translate=c.trans[1], min_zoom=c.zoom[2], max_zoom=c.zoom[3], min_squeeze=c.squeeze[2],
        max_squeeze=c.squeeze[3], min_rotate=c.rotate[2], max_rotate=c.rotate[3], validate_size=[H, W]))
    return torch.stack(m._random_mirror(lst))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = Path(sys.argv[1]).resolve()
    warnings.filterwarnings("ignore", category=UserWarning)  # the reference resizes its out= buffers
    out = {"seed": np.int64(SEED)}
    for name, cfg_fn, H, W in THETA_CASES:
        st_cfg = cfg_fn().train.st_cfg
        m = ref_module(ref, st_cfg)
        torch.manual_seed(SEED)
        th = ref_thetas(m, 4, H, W)
        assert not bool(m.find_invalid(W, H, th.reshape(-1, 6)).any())
        out[f"thetas_{name}"] = th.numpy().astype(np.float32)
        out[f"thetas_{name}_hw"] = np.array([H, W], dtype=np.int64)

    m = ref_module(ref, config.kitti_stage1_ar().train.st_cfg)
    for name, B, H, W, seed, identity in CASES:
        th = ar_util.identity_thetas(B) if identity else ar_util.clear_thetas(B, H, W, margin=1e-3)
        if not identity:
            for k in range(2):
                assert ar_util.edge_distance(th[k], H, W).min() >= 1e-3, name
            assert ar_util.zeroed_fraction(th[0], H, W)[0] > 0.1, name  # part of sample 0 is outside
            assert th[0, 1, 0] < 0 and th[1, 1, 0] < 0, name            # sample 1 is mirrored
        img1, img2, flow, mask = ar_util.inputs(B, H, W, seed, lo=0.1 if identity else 0.0)
        with torch.no_grad():
            res = {"img1_t": m.transform_image(img1, th[0]), "img2_t": m.transform_image(img2, th[1]),
                   "flow_t": m.transform_flow(flow, th[0], th[1]), "mask_t": m.transform_image(mask, th[0])}
        out[f"{name}_thetas"] = th.numpy().astype(np.float32)
        out[f"{name}_shape"] = np.array([B, H, W], dtype=np.int64)
        out[f"{name}_seed"] = np.int64(seed)
        for k, v in res.items():
            out[f"{name}_{k}"] = v.numpy().astype(np.float32)
    path = HERE / "ar_transform.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")
    assert path.stat().st_size < 128 * 1024


if __name__ == "__main__":
    main()
