"""The census (ternary) loss entries that need no GPU: include/unsamflow_hip_census.h
is exported and bound, its version, argument rejection before any device work,
the in-tree TernaryLoss against the reference capture (tests/golden/ternary.npz,
made by tests/golden/make_golden_ternary.py), and the stage-1 configs."""
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO

HEADER = REPO / "include" / "unsamflow_hip_census.h"


@pytest.fixture(scope="module")
def lib():
    from unsamflow_amd import _lib
    from unsamflow_amd.build import build_library

    build_library()
    return _lib.load()


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(usf_\w+)\s*\(", text)))


def test_header_declares_the_census_entries():
    assert declared_symbols() == sorted(
        ["usf_census_api_version", "usf_census_loss_partials", "usf_census_loss_fwd_f32",
         "usf_census_loss_pair_fwd_f32", "usf_census_loss_bwd_f32", "usf_census_loss_pyramid_partials",
         "usf_census_loss_pyramid_fwd_f32", "usf_census_loss_pyramid_bwd_f32"])


def test_library_exports_and_binds_every_declared_symbol(lib):
    from unsamflow_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.library_path())], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (usf_\w+)", out))
    for s in declared_symbols():
        assert s in exported, s
        assert getattr(lib, s).argtypes is not None, s  # bound at load()
    assert set(_lib.CENSUS_SYMBOLS) == set(declared_symbols())
    assert not set(_lib.CENSUS_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)


def test_ctypes_signatures_match_header():
    from unsamflow_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name, (argtypes, _) in _lib.CENSUS_SYMBOLS.items():
        m = re.search(name + r"\s*\(([^)]*)\)", text)
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(argtypes), name


def test_census_api_version(lib):
    from unsamflow_amd import _lib

    assert lib.usf_census_api_version() == _lib.CENSUS_API_VERSION == 1


def test_build_id_covers_the_census_header():
    from unsamflow_amd import build

    assert "census.hip" in build.SOURCES
    assert HEADER.name in build.PUBLIC_HEADERS


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc not available")
def test_census_kernels_fit_their_register_budget():
    """No census kernel spills to scratch; the forward with the gradient basis
    stays within 96 VGPRs (5 waves/SIMD) and none of them uses more LDS than the
    finalisation's reduction slots."""
    import sys

    sys.path.insert(0, str(REPO / "tools"))
    import kernel_resources

    res = kernel_resources.resources(REPO / "unsamflow_amd" / "csrc" / "census.hip")
    fwd = [r for r in res if "census_fwd_kernel" in r[0]]
    assert len(fwd) == 4 and len(res) == 6, [r[0] for r in res]
    for name, vgpr, lds, scratch in res:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 96 and lds <= 64, (name, vgpr, lds)


def test_partials_size(lib):
    # {T, sum m} per strip: 60 own columns, at least 4 rows
    assert lib.usf_census_loss_partials(2, 9, 61) == 2 * 2 * 3 * 2
    assert lib.usf_census_loss_partials(0, 9, 61) == 0


# argument order of the usf_photo_loss_* twins with one weight; dummy non-null pointers (never dereferenced)
def _fwd(L, src=1, tgt=1, mask=1, flow=1, fbs=32, part=1, out=1, basis=None, B=1, C=3, H=4, W=4, pad=1):
    return L.usf_census_loss_fwd_f32(src, tgt, mask, flow, fbs, part, out, basis, B, C, H, W, pad, 1.0, None)


def _pair(L, im1=1, im2=1, m1=1, m2=1, flow=1, fbs=64, part=1, out=1, basis=None, B=1, C=3, H=4, W=4, pad=1):
    return L.usf_census_loss_pair_fwd_f32(im1, im2, m1, m2, flow, fbs, part, out, basis, B, C, H, W, pad, 1.0, None)


# every pointer of _fwd on a 16-byte boundary: the base of the alignment cases
_AL = dict(src=16, tgt=16, mask=16, flow=16, part=16, out=16)


def _pyr(L, n, B=1, C=3, pad=1, H=4, W=4, part=1, nfloats=1 << 20, out=1, im1=True, ptr=1, bad=None):
    """``ptr``: the fake device pointer of every scale; ``bad``: im2 of scale 1 instead."""
    import ctypes

    ptrs = (ctypes.c_void_p * 4)(ptr, ptr, ptr, ptr)
    if bad is not None:
        return L.usf_census_loss_pyramid_fwd_f32(n, ptrs, (ctypes.c_void_p * 4)(ptr, bad, ptr, ptr), ptrs, ptrs, ptrs,
                                                 (ctypes.c_longlong * 4)(*[4 * H * W] * 4), (ctypes.c_int * 4)(*[H] * 4),
                                                 (ctypes.c_int * 4)(*[W] * 4), part, nfloats, out, None, B, C, pad, 1.0,
                                                 None)
    Hs, Ws = (ctypes.c_int * 4)(H, H, H, H), (ctypes.c_int * 4)(W, W, W, W)
    fbs = (ctypes.c_longlong * 4)(*[4 * H * W] * 4)
    return L.usf_census_loss_pyramid_fwd_f32(n, ptrs if im1 else None, ptrs, ptrs, ptrs, ptrs, fbs, Hs, Ws, part,
                                             nfloats, out, None, B, C, pad, 1.0, None)


def _pyr_bwd(L, n, basis=True, ptr=1, coef=None, bad=None):
    """``ptr``: every fake device pointer; ``coef``: its own; ``bad``: grad_flow of scale 1 instead."""
    import ctypes

    ptrs = (ctypes.c_void_p * 4)(ptr, ptr, ptr, ptr)
    gflow = ptrs if bad is None else (ctypes.c_void_p * 4)(ptr, bad, ptr, ptr)
    hw = (ctypes.c_int * 4)(4, 4, 4, 4)
    return L.usf_census_loss_pyramid_bwd_f32(n, ptrs if basis else None, ptr if coef is None else coef, ptr, gflow, hw,
                                             hw, 1, None)


@pytest.mark.parametrize(
    "call,needle",
    [
        (lambda L: _fwd(L, src=None), "null input"),
        (lambda L: _fwd(L, flow=None), "null input"),
        (lambda L: _fwd(L, out=None), "null output"),
        (lambda L: _fwd(L, part=None), "null output"),
        (lambda L: _fwd(L, C=1), "C=1"),
        (lambda L: _fwd(L, C=4), "C=4"),
        (lambda L: _fwd(L, H=2), "no interior pixel"),
        (lambda L: _fwd(L, W=2), "no interior pixel"),
        (lambda L: _fwd(L, pad=7), "pad_mode 7"),
        (lambda L: _fwd(L, B=0), "non-positive"),
        (lambda L: _fwd(L, B=2, fbs=31), "< 2*H*W"),
        (lambda L: _fwd(L, H=16384, W=16384), "too large"),
        (lambda L: _pair(L, m2=None), "null input"),
        (lambda L: _pair(L, im2=None), "null input"),
        (lambda L: _pair(L, out=None), "null output"),
        (lambda L: _pair(L, C=2), "C=2"),
        (lambda L: _pair(L, H=2), "no interior pixel"),
        (lambda L: _pair(L, pad=-1), "pad_mode -1"),
        (lambda L: _pair(L, B=2, fbs=32), "< 4*H*W"),
        (lambda L: _pair(L, H=16384, W=16384), "too large"),
        (lambda L: L.usf_census_loss_bwd_f32(1, None, 1, 1, 1, 4, 4, 1, None), "null pointer"),
        (lambda L: L.usf_census_loss_bwd_f32(1, 1, 1, 1, 1, 4, 4, 3, None), "ndir=3"),
        (lambda L: L.usf_census_loss_bwd_f32(1, 1, 1, 1, 1, 0, 4, 1, None), "non-positive"),
        (lambda L: _pyr(L, 0), "nscale 0"),
        (lambda L: _pyr(L, 5), "nscale 5"),
        (lambda L: _pyr(L, 2, im1=False), "null array"),
        (lambda L: _pyr(L, 2, C=1), "C=1"),
        (lambda L: _pyr(L, 2, W=2), "no interior pixel"),
        (lambda L: _pyr(L, 2, pad=3), "pad_mode 3"),
        (lambda L: _pyr(L, 2, nfloats=3), "partials of 3 floats"),
        (lambda L: _pyr(L, 2, out=None), "null out"),
        (lambda L: _pyr_bwd(L, 0), "nscale 0"),
        (lambda L: _pyr_bwd(L, 5), "nscale 5"),
        (lambda L: _pyr_bwd(L, 2, basis=False), "null pointer"),
        # the alignment contract (include/unsamflow_hip_census.h): 20 where 16 bytes are required, 18 where 4
        (lambda L: _fwd(L, **{**_AL, "src": 20}), "src must be 16-byte aligned"),
        (lambda L: _fwd(L, **{**_AL, "mask": 24}), "mask must be 16-byte aligned"),
        (lambda L: _fwd(L, **{**_AL, "flow": 18}), "flow must be 4-byte aligned"),
        (lambda L: _fwd(L, **{**_AL, "out": 18}), "out must be 4-byte aligned"),
        (lambda L: _fwd(L, **{**_AL, "basis": 20}), "grad_basis must be 16-byte aligned"),
        (lambda L: _pair(L, im1=16, im2=20, m1=16, m2=16, flow=16, part=16, out=16), "im2 must be 16-byte aligned"),
        (lambda L: _pair(L, im1=16, im2=16, m1=16, m2=16, flow=18, part=16, out=16), "flow must be 4-byte aligned"),
        (lambda L: _pair(L, im1=16, im2=16, m1=16, m2=16, flow=16, part=24, out=16), "partials must be 16-byte aligned"),
        (lambda L: L.usf_census_loss_bwd_f32(20, 16, 16, 16, 1, 4, 4, 1, None), "grad_basis must be 16-byte aligned"),
        (lambda L: L.usf_census_loss_bwd_f32(16, 18, 16, 16, 1, 4, 4, 1, None), "coef must be 4-byte aligned"),
        (lambda L: L.usf_census_loss_bwd_f32(16, 16, 16, 24, 1, 4, 4, 2, None), "grad_flow must be 16-byte aligned"),
        (lambda L: _pyr(L, 2, part=16, out=16, ptr=16, bad=20), "im2 must be 16-byte aligned"),
        (lambda L: _pyr(L, 2, part=16, out=18, ptr=16), "out must be 4-byte aligned"),
        (lambda L: _pyr_bwd(L, 2, ptr=16, bad=20), "grad_flow must be 16-byte aligned"),
        (lambda L: _pyr_bwd(L, 2, ptr=16, coef=18), "coef must be 4-byte aligned"),
    ],
)
def test_invalid_arguments_rejected_without_launch(lib, call, needle):
    assert call(lib) == -1
    msg = lib.usf_last_error_string().decode()
    assert needle in msg, msg


def test_pyramid_partials_rejects_bad_counts(lib):
    import ctypes

    hw = (ctypes.c_int * 4)(8, 8, 8, 8)
    assert lib.usf_census_loss_pyramid_partials(0, hw, hw, 1) == 0
    assert lib.usf_census_loss_pyramid_partials(5, hw, hw, 1) == 0
    assert lib.usf_census_loss_pyramid_partials(2, hw, hw, 1) == 2 * 2 * lib.usf_census_loss_partials(1, 8, 8)


def test_ternary_loss_matches_reference_capture():
    """flow_loss.TernaryLoss == the reference's losses/loss_blocks.TernaryLoss
    on the captured inputs (fp32 CPU both; rtol 1e-6)."""
    import torch

    from unsamflow_amd.flow_loss import TernaryLoss

    path = GOLDEN / "ternary.npz"
    if not path.exists():
        pytest.skip("tests/golden/ternary.npz not captured")
    g = dict(np.load(path, allow_pickle=False))
    names = sorted(k[:-4] for k in g if k.endswith("_out"))
    assert len(names) == 4 and "min_3x5" in names and any(n.startswith("masked") for n in names)
    for n in names:
        out = TernaryLoss(torch.from_numpy(g[n + "_im"]), torch.from_numpy(g[n + "_im_warp"])).numpy()
        assert out.shape == g[n + "_out"].shape
        np.testing.assert_allclose(out, g[n + "_out"], rtol=1e-6, atol=1e-9, err_msg=n)
        assert g[n + "_out"].max() > 0.01, n


@pytest.mark.parametrize("name", ["kitti_stage1", "sintel_stage1"])
def test_stage1_configs_carry_the_reference_overrides(name):
    from unsamflow_amd import config

    cfg, base = getattr(config, name)(), getattr(config, name.replace("stage1", "base"))()
    over = {"occ_from_back": False, "w_l1": 0.0, "w_ssim": 0.0, "w_ternary": 1.0}
    for k, v in over.items():
        assert cfg.loss[k] == v and type(cfg.loss[k]) is type(v), k
    assert {k: v for k, v in cfg.loss.items() if k not in over} == {k: v for k, v in base.loss.items() if k not in over}
    assert cfg.model == base.model and cfg.train == base.train and cfg.data == base.data


def test_images_requiring_grad_are_refused():
    import torch

    from unsamflow_amd.census import ternary_loss, ternary_loss_pair, ternary_loss_pyramid

    im = torch.zeros(1, 3, 4, 4, requires_grad=True)
    z, m, f = torch.zeros(1, 3, 4, 4), torch.ones(1, 1, 4, 4), torch.zeros(1, 4, 4, 4)
    with pytest.raises(NotImplementedError):
        ternary_loss(f[:, :2], im, z, m)
    with pytest.raises(NotImplementedError):
        ternary_loss_pair(f, z, im, m, m)
    with pytest.raises(NotImplementedError):
        ternary_loss_pyramid([f], [im], [z], [m], [m])
