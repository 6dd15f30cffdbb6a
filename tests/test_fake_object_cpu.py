"""The key-object augmentation without a GPU: the torch composition of
add_fake_object and the ObjectCache against the reference capture
(tests/golden/fake_object.npz, made by tests/golden/make_golden_fakeobj.py),
include/unsamflow_hip_fakeobj.h exported and bound, argument rejection before
any device work, the configs and a CPU TrainStep that fills its cache and pastes."""
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fakeobj_util
from conftest import REPO, load_golden

HEADER = REPO / "include" / "unsamflow_hip_fakeobj.h"
SYMBOLS = ["usf_fakeobj_api_version", "usf_fakeobj_paste_crop_f32", "usf_fakeobj_push_partials",
           "usf_fakeobj_push_f32"]
CASES = ["min_2x3", "odd_13x21", "wide_17x38"]


@pytest.fixture(scope="module")
def lib():
    from unsamflow_amd import _lib
    from unsamflow_amd.build import build_library

    build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return load_golden("fake_object.npz")


def _case(golden, name):
    B, H, W = (int(v) for v in golden[name + "_shape"])
    seed, K = int(golden[name + "_seed"]), int(golden["K"])
    return fakeobj_util.base(B, H, W, seed), fakeobj_util.objects(K * B, H, W, seed + 5), (B, H, W, K)


# ------------------------------------------------------------- composition --
@pytest.mark.parametrize("name", CASES)
def test_composition_matches_the_reference_capture(golden, name):
    """K rounds chained as the trainer chains them, every output at atol 1e-6
    (observed at most 1.2e-7 against the reference; the headroom is for another
    summation order of the bilinear taps)."""
    from unsamflow_amd import fake_object as fo

    (img1, img2, flow, noc), (mask, src, motion), (B, H, W, K) = _case(golden, name)
    full = fo.paste_and_crop_torch(img1, img2, flow, noc, mask, src, motion, (H, W), (0, 0))
    imgs, fl, nc, newmask = full
    got = {"img1": imgs[:, :3], "img2": imgs[:, 3:], "flow": fl, "noc": nc, "newmask": newmask}
    for k, v in got.items():
        cap = golden[f"{name}_{k}"]
        assert tuple(v.shape) == cap.shape and v.dtype == torch.float32
        err = float(np.abs(v.numpy() - cap).max())
        print(f"[fakeobj] {name} {k}: |fp32-cap|={err:.3e} max|cap|={np.abs(cap).max():.3e}")
        assert err <= 1e-6, (name, k, err)
    # the capture shows what it is meant to: pasted pixels, a changed flow, a grown noc
    assert float((got["img1"] - img1).abs().max()) > 0.1 and float((got["flow"] - flow).abs().max()) > 1.0
    assert float(got["noc"].sum()) > float(noc.sum())


def test_add_fake_object_keeps_the_dict_interface(golden):
    from unsamflow_amd import fake_object as fo

    (img1, img2, flow, noc), (mask, src, motion), (B, H, W, K) = _case(golden, "odd_13x21")
    d = {"img1_tgt": img1, "img2_tgt": img2, "flow_tgt": flow, "noc_tgt": noc, "img_src": src[:B],
         "obj_mask": mask[:B], "motion": motion[:B]}
    out = fo.add_fake_object(d)
    assert len(out) == 7 and out[2] is None and out[3] is None
    seg = torch.ones(B, 1, H, W) * 3.0
    out2 = fo.add_fake_object(dict(d, full_seg1_st=seg, full_seg2_st=seg))
    assert float(out2[2].max()) == 4.0 and out2[3].shape == seg.shape
    for a, b in zip((out[0], out[1], out[4], out[5], out[6]), (out2[0], out2[1], out2[4], out2[5], out2[6])):
        assert torch.equal(a, b)
    # fp64 runs too, and the crop is the slice of the full result
    d64 = {k: v.double() for k, v in d.items()}
    assert fo.add_fake_object(d64)[0].dtype == torch.float64
    full = fo.paste_and_crop_torch(img1, img2, flow, noc, mask, src, motion, (H, W), (0, 0))
    crop = fo.paste_and_crop_torch(img1, img2, flow, noc, mask, src, motion, (5, 7), (3, 9))
    for a, b in zip(full[:3], crop[:3]):
        assert torch.equal(a[:, :, 3:8, 9:16], b)


def test_round_order_is_visible(golden):
    from unsamflow_amd import fake_object as fo

    (img1, img2, flow, noc), (mask, src, motion), (B, H, W, K) = _case(golden, "odd_13x21")
    cache = fakeobj_util.filled_cache(mask, src, motion)
    p = fakeobj_util.plain_params(2 * B)
    fwd = torch.arange(2 * B, dtype=torch.int32)
    rev = torch.cat([fwd[B:], fwd[:B]])
    a = fo.paste_and_crop(img1, img2, flow, noc, cache, fwd, p, (H, W), (0, 0))
    b = fo.paste_and_crop(img1, img2, flow, noc, cache, rev, p, (H, W), (0, 0))
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    assert torch.equal(a[2], b[2])  # the maximum does not care


# ------------------------------------------------------------------- cache --
def test_cache_counts_follow_the_reference(golden):
    from unsamflow_amd.fake_object import ObjectCache

    H, W = (int(v) for v in golden["pop_hw"])
    seed = int(golden["pop_seed"])
    c = ObjectCache(5, "cpu", generator=torch.Generator().manual_seed(1))
    for i, (count, none) in enumerate(zip(golden["counts"], golden["pop_before_full"])):
        m, im, mo = fakeobj_util.objects(2, H, W, seed + 10 * i)
        flow = mo.view(2, 2, 1, 1).expand(2, 2, H, W).contiguous()
        before = None if c.obj_mask is None else (c.obj_mask.clone(), c.img.clone(), c.motion.clone())
        prev = c.count
        c.push(m, im, flow, torch.tensor([True, True]))
        assert c.count == int(count) and (c.pop(2) is None) == bool(none), i
        if before is None:
            continue
        changed = [j for j in range(5) if not torch.equal(before[0][j], c.obj_mask[j])
                   or not torch.equal(before[1][j], c.img[j])]
        if prev <= 3:  # room: the next slots in order
            assert changed == [prev, prev + 1]
        elif prev == 4:  # partial fill: the last slot gets object 0, one earlier slot object 1
            assert 4 in changed and len(changed) == 2 and torch.equal(c.img[4], im[0])
            other = [j for j in changed if j != 4][0]
            assert torch.equal(c.img[other], im[1]) and torch.equal(c.obj_mask[other], m[1])
        else:  # full: two distinct slots
            assert len(changed) == 2
            assert sorted(torch.equal(c.img[j], im[k]) for j in changed for k in range(2)) == [False, False, True, True]
    # a constant flow's masked mean is that flow (object 1's mask is fractional)
    j = [j for j in range(5) if torch.equal(c.img[j], im[1])][0]
    np.testing.assert_allclose(c.motion[j].numpy(), mo[1].numpy(), rtol=1e-6)


def test_pop_arithmetic_matches_the_reference(golden):
    from unsamflow_amd import fake_object as fo

    H, W = (int(v) for v in golden["pop_hw"])
    n = int(golden["pop_n"])
    assert bool(golden["pop_cache_unchanged"])  # the reference's flips act on copies
    m, im, mo = fakeobj_util.objects(n, H, W, int(golden["pop_seed"]))
    cache = fakeobj_util.filled_cache(m, im, mo)
    params = fo.pop_arithmetic(*(torch.from_numpy(golden[k]) for k in ("pop_scale", "pop_sign", "pop_flip")))
    slots = torch.from_numpy(golden["pop_idx"]).to(torch.int32)
    assert params[:, 2].tolist() == [0.0, 1.0, 1.0, 0.0] and (params[:, 1] < 0).tolist() == [False, True, False, True]
    gm, gi, gmo = cache.gather(slots, params)
    assert np.array_equal(gm.numpy(), golden["pop_mask"]) and np.array_equal(gi.numpy(), golden["pop_img"])
    assert np.array_equal(gmo.numpy(), golden["pop_motion"])  # the same fp32 products, bit for bit


def test_pop_draws_leave_the_cache_unchanged_and_wait_for_a_full_cache():
    from unsamflow_amd.fake_object import ObjectCache

    m, im, mo = fakeobj_util.objects(6, 5, 7, 11)
    flow = mo.view(6, 2, 1, 1).expand(6, 2, 5, 7).contiguous()
    g = torch.Generator().manual_seed(5)
    c = ObjectCache(6, "cpu", generator=g)
    assert c.pop(2) is None and c.pop_tensors(2) is None and c.obj_mask is None
    c.push(m[:4], im[:4], flow[:4], torch.ones(4, dtype=torch.bool))
    state = g.get_state()
    assert c.pop(2) is None and torch.equal(g.get_state(), state)  # no draw while filling
    c.push(m[4:], im[4:], flow[4:], torch.ones(2, dtype=torch.bool))
    assert c.count == 6
    snap = [t.clone() for t in (c.obj_mask, c.img, c.motion)]
    flipped = 0
    for _ in range(4):
        slots, params = c.pop(6)
        assert slots.dtype == torch.int32 and slots.device.type == "cpu" and sorted(slots.tolist()) == list(range(6))
        assert params.shape == (6, 4) and params.dtype == torch.float32 and params.device.type == "cpu"
        s = params[:, 1].abs()
        assert bool(((s >= 0.8) & (s < 1.5)).all()) and torch.equal(params[:, 0].abs(), s)
        assert torch.equal(params[:, 0] == -params[:, 1], params[:, 2] == 1.0)
        flipped += int(params[:, 2].sum())
        pm, pi, pmo = c.gather(slots, params)
        j = int(slots[0])
        want = m[j].flip(dims=[2]) if params[0, 2] else m[j]
        assert torch.equal(pm[0], want)
    assert 0 < flipped < 24
    assert all(torch.equal(a, b) for a, b in zip(snap, (c.obj_mask, c.img, c.motion)))
    # the draws of a pop: randperm, then three rand(n)
    g2 = torch.Generator().manual_seed(9)
    c.generator = torch.Generator().manual_seed(9)
    slots, params = c.pop(3)
    assert torch.equal(slots, torch.randperm(6, generator=g2)[:3].to(torch.int32))
    draws = [torch.rand(3, generator=g2) for _ in range(3)]
    from unsamflow_amd.fake_object import pop_arithmetic

    assert torch.equal(params, pop_arithmetic(*draws))
    assert torch.equal(c.pop(2, with_aug=False)[1], fakeobj_util.plain_params(2))


def test_push_validity():
    from unsamflow_amd.fake_object import ObjectCache

    m, im, mo = fakeobj_util.objects(3, 5, 7, 12)
    flow = mo.view(3, 2, 1, 1).expand(3, 2, 5, 7).contiguous()
    c = ObjectCache(4, "cpu")
    c.push(m, im, flow, torch.zeros(3, dtype=torch.bool))  # no valid sample: a no-op
    assert c.count == 0 and c.obj_mask is None
    c.push(m, im, flow, torch.tensor([True, False, True]))
    assert c.count == 2 and torch.equal(c.img[0], im[0]) and torch.equal(c.img[1], im[2])
    assert float(c.img[2:].abs().max()) == 0.0
    # a CPU mask may carry the reference's NaN marker instead
    nan = m.clone()
    nan[0] = float("nan")
    c.push(nan, im, flow)
    assert c.count == 4 and torch.equal(c.img[2], im[1]) and torch.equal(c.img[3], im[2])
    with pytest.raises(ValueError, match="host bool"):
        c.push(m, im, flow, torch.ones(3))
    with pytest.raises(ValueError, match="synchronise"):
        c.push(m.to("meta"), im, flow)


# ------------------------------------------------------ library and header --
def header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def test_header_declares_exactly_the_bound_symbols():
    from unsamflow_amd import _lib, build

    declared = sorted(set(re.findall(r"\b(usf_\w+)\s*\(", header_text())))
    assert declared == sorted(SYMBOLS) == sorted(_lib.FAKEOBJ_SYMBOLS)
    others = (set(_lib.EXPORTED_SYMBOLS) | set(_lib.CENSUS_SYMBOLS) | set(_lib.AR_SYMBOLS) | set(_lib.SEGPOOL_SYMBOLS)
              | set(_lib.HG_SYMBOLS) | set(_lib.CONVEPI_SYMBOLS))
    assert not set(_lib.FAKEOBJ_SYMBOLS) & others
    for name, (argtypes, _) in _lib.FAKEOBJ_SYMBOLS.items():
        m = re.search(name + r"\s*\(([^)]*)\)", header_text())
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(argtypes), name
    text = HEADER.read_text()
    bit = int(re.search(r"#define USF_DEVERR_FAKEOBJ_BAD_SLOT (\d+)", text).group(1))
    assert bit == _lib.DEVERR_FAKEOBJ_BAD_SLOT == 16 and bit not in (1, 2, _lib.DEVERR_SEGPOOL_BAD_ID,
                                                                      _lib.DEVERR_HG_BAD_ID)
    assert int(re.search(r"#define USF_FAKEOBJ_MAX_K (\d+)", text).group(1)) == _lib.FAKEOBJ_MAX_K == 8
    assert "fakeobj.hip" in build.SOURCES and HEADER.name in build.PUBLIC_HEADERS


def test_library_exports_and_binds_the_entries(lib):
    from unsamflow_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.library_path())], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (usf_\w+)", out))
    for s in SYMBOLS:
        assert s in exported, s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.usf_fakeobj_api_version() == _lib.FAKEOBJ_API_VERSION == 1
    assert lib.usf_abi_version() == 8  # the main ABI is untouched
    # {sum m, sum u m, sum v m} per workgroup of 1024 pixels of one sample
    assert lib.usf_fakeobj_push_partials(2, 64, 96) == 3 * 2 * 6
    assert lib.usf_fakeobj_push_partials(3, 2, 3) == 3 * 3
    assert lib.usf_fakeobj_push_partials(0, 8, 8) == 0


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc not available")
def test_fakeobj_kernels_do_not_spill():
    """Paste + crop, the push and its finalisation: no scratch, at most 64 VGPRs
    (8 waves/SIMD), LDS only for the reductions' slots."""
    import sys

    sys.path.insert(0, str(REPO / "tools"))
    import kernel_resources

    res = kernel_resources.resources(REPO / "unsamflow_amd" / "csrc" / "fakeobj.hip")
    assert len(res) == 3 and sum("fakeobj_paste_crop_kernel" in r[0] for r in res) == 1, [r[0] for r in res]
    for name, vgpr, lds, scratch in res:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 64 and lds <= 96, (name, vgpr, lds)


# dummy non-null pointers (never dereferenced: every call is rejected before a launch)
def _paste(L, img1=1, img2=1, flow=1, fbs=24, noc=1, cm=1, ci=1, cmo=1, slot=1, param=1, o1=1, of=1, on=1, B=1, H=3,
           W=4, K=3, size=4, y0=0, x0=0, ch=3, cw=4):
    return L.usf_fakeobj_paste_crop_f32(img1, img2, flow, fbs, noc, cm, ci, cmo, slot, param, o1, of, on, B, H, W, K,
                                        size, y0, x0, ch, cw, None)


# every pointer on a 16-byte boundary: the base of the alignment cases
_PASTE16 = dict(img1=16, img2=16, flow=16, noc=16, cm=16, ci=16, cmo=16, slot=16, param=16, o1=16, of=16, on=16)
_PUSH16 = dict(mask=16, img=16, flow=16, slot=16, cm=16, ci=16, cmo=16, part=16)


def _push(L, mask=1, img=1, flow=1, fbs=24, slot=1, cm=1, ci=1, cmo=1, part=1, B=1, H=3, W=4, size=4):
    return L.usf_fakeobj_push_f32(mask, img, flow, fbs, slot, cm, ci, cmo, part, B, H, W, size, None)


@pytest.mark.parametrize(
    "call,needle",
    [
        (lambda L: _paste(L, K=0), "K=0 outside"),
        (lambda L: _paste(L, K=9), "K=9 outside"),
        (lambda L: _paste(L, y0=1), "outside the 3x4 image"),
        (lambda L: _paste(L, x0=2, cw=3), "outside the 3x4 image"),
        (lambda L: _paste(L, y0=-1, ch=2), "outside the 3x4 image"),
        (lambda L: _paste(L, ch=0), "outside the 3x4 image"),
        (lambda L: _paste(L, x0=2 ** 31 - 1, cw=2), "outside the 3x4 image"),
        (lambda L: _paste(L, H=1, ch=1), "H, W >= 2"),
        (lambda L: _paste(L, W=1, cw=1), "H, W >= 2"),
        (lambda L: _paste(L, B=0), "non-positive"),
        (lambda L: _paste(L, B=2, fbs=23), "< 2*H*W"),
        (lambda L: _paste(L, size=0), "cache_size=0"),
        (lambda L: _paste(L, img1=None), "null input"),
        (lambda L: _paste(L, cm=None), "null input"),
        (lambda L: _paste(L, cmo=None), "null input"),
        (lambda L: _paste(L, slot=None), "null input"),
        (lambda L: _paste(L, param=None), "null input"),
        (lambda L: _paste(L, o1=None), "null output"),
        (lambda L: _paste(L, on=None), "null output"),
        (lambda L: _push(L, mask=None), "null input"),
        (lambda L: _push(L, slot=None), "null input"),
        (lambda L: _push(L, ci=None), "null output"),
        (lambda L: _push(L, cmo=None), "null output"),
        (lambda L: _push(L, part=None), "null output"),
        (lambda L: _push(L, H=1), "H, W >= 2"),
        (lambda L: _push(L, B=0), "non-positive"),
        (lambda L: _push(L, size=-2), "cache_size=-2"),
        (lambda L: _push(L, B=70000), "B=70000"),
        # the alignment contract (include/unsamflow_hip_fakeobj.h): 20 where 16 bytes are required, 18 where 4
        (lambda L: _paste(L, **{**_PASTE16, "img2": 20}), "img2 must be 16-byte aligned"),
        (lambda L: _paste(L, **{**_PASTE16, "ci": 18}), "cache_img must be 4-byte aligned"),
        (lambda L: _paste(L, **{**_PASTE16, "flow": 18}), "flow must be 4-byte aligned"),
        (lambda L: _paste(L, **{**_PASTE16, "cmo": 18}), "cache_motion must be 4-byte aligned"),
        (lambda L: _paste(L, **{**_PASTE16, "param": 18}), "param must be 4-byte aligned"),
        (lambda L: _paste(L, **{**_PASTE16, "on": 20}), "noc_ot must be 16-byte aligned"),
        (lambda L: _push(L, **{**_PUSH16, "mask": 20}), "obj_mask must be 16-byte aligned"),
        (lambda L: _push(L, **{**_PUSH16, "cm": 18}), "cache_mask must be 4-byte aligned"),
        (lambda L: _push(L, **{**_PUSH16, "slot": 18}), "slot must be 4-byte aligned"),
        (lambda L: _push(L, **{**_PUSH16, "flow": 18}), "flow must be 4-byte aligned"),
        (lambda L: _push(L, **{**_PUSH16, "part": 24}), "partials must be 16-byte aligned"),
    ],
)
def test_invalid_arguments_rejected_without_launch(lib, call, needle):
    assert call(lib) == -1
    msg = lib.usf_last_error_string().decode()
    assert needle in msg, msg


def test_ops_refuse_cpu_tensors_and_bad_tables():
    from unsamflow_amd import ops

    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fakeobj_paste_crop(z(1, 3, 4, 6), z(1, 3, 4, 6), z(1, 2, 4, 6), z(1, 1, 4, 6), z(2, 1, 4, 6), z(2, 3, 4, 6),
                               z(2, 2), z(1, dtype=torch.int32), z(1, 4), (4, 6), (0, 0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.fakeobj_push(z(1, 1, 4, 6), z(1, 3, 4, 6), z(1, 2, 4, 6), z(1, dtype=torch.int32), z(2, 1, 4, 6),
                         z(2, 3, 4, 6), z(2, 2))


# ------------------------------------------------------- configs and step --
@pytest.mark.parametrize("name,base", [("kitti_aug", "kitti_stage1_ar"), ("sintel_aug", "sintel_stage1_ar"),
                                       ("kitti_aug_hg", "kitti_stage2_hg"), ("sintel_aug_hg", "sintel_stage2_hg")])
def test_aug_configs_add_the_key_object_keys_only(name, base):
    from unsamflow_amd import config

    cfg, b = getattr(config, name)(), getattr(config, base)()
    assert cfg.train.key_obj_aug is True and cfg.train.key_obj_count == 3 and cfg.train.w_ar == 0.1
    assert b.train.key_obj_aug is False and "key_obj_count" not in b.train  # the existing configs are as they were
    assert cfg.loss == b.loss and cfg.model == b.model and cfg.data == b.data
    rest = {k: v for k, v in cfg.train.items() if k not in ("key_obj_aug", "key_obj_count", "w_ar")}
    assert rest == {k: v for k, v in b.train.items() if k not in ("key_obj_aug", "w_ar")}


def test_synthetic_key_objects():
    from unsamflow_amd.harness import synthetic_key_objects

    mask, valid = synthetic_key_objects(16, 64, 128, "cpu", seed=3)
    again, valid2 = synthetic_key_objects(16, 64, 128, "cpu", seed=3)
    assert mask.shape == (16, 1, 64, 128) and valid.dtype == torch.bool and valid.device.type == "cpu"
    assert torch.equal(valid, valid2) and torch.equal(mask.nan_to_num(-1.0), again.nan_to_num(-1.0))
    assert 0 < int(valid.sum()) < 16
    for b in range(16):
        if valid[b]:
            assert set(mask[b].unique().tolist()) == {0.0, 1.0} and float(mask[b].mean()) >= 0.005
        else:
            assert bool(torch.isnan(mask[b]).all())
    assert torch.equal(~torch.isnan(mask[:, 0, 0, 0]), valid)
    assert bool(synthetic_key_objects(4, 64, 128, "cpu", seed=3, p_invalid=0.0)[1].all())


def _cpu_step(cfg, **kw):
    from oracle.torch_ref import (OracleCorrelation, oracle_flow_warp, oracle_occu_mask_backward,
                                  oracle_occu_mask_bidirection)
    from unsamflow_amd.harness import TrainStep

    step = TrainStep(cfg, "cpu", corr_module=OracleCorrelation(4), warp_fn=oracle_flow_warp,
                     occ_backward_fn=oracle_occu_mask_backward,
                     loss_kwargs=dict(occ_bidir_fn=oracle_occu_mask_bidirection), **kw)
    with torch.no_grad():
        for p in step.module.parameters():
            p.mul_(0.02)
    return step


def test_cpu_train_step_fills_the_cache_then_pastes(monkeypatch):
    from unsamflow_amd import config, fake_object
    from unsamflow_amd.harness import synthetic_key_objects, synthetic_pair

    B, H, W = 2, 64, 128
    img1, img2, _, _ = synthetic_pair(B, H, W, "cpu")
    mask, valid = synthetic_key_objects(B, H, W, "cpu", seed=8, p_invalid=0.0)
    cfg = config.kitti_aug()
    # PWCLite's pyramid needs multiples of 64: a 32-row crop fails in the model's own upsampling
    # (with or without this feature), so the crop is 64x64 as in tests/test_ar_cpu.py
    cfg.train.ot_size = [64, 64]
    # a pop takes key_obj_count * B DISTINCT objects (the reference's np.random.choice(replace=False)
    # raises otherwise): 2 rounds of B = 2 from the cache of 4
    cfg.train.key_obj_count = 2
    step = _cpu_step(cfg, obj_cache_size=4)
    plain_cfg = config.kitti_stage1_ar()
    plain_cfg.train.ot_size = [64, 64]
    plain_cfg.train.w_ar = 0.1
    plain = _cpu_step(plain_cfg)
    pastes = []
    real = fake_object.paste_and_crop
    monkeypatch.setattr(fake_object, "paste_and_crop", lambda *a, **k: (pastes.append(len(a[5])), real(*a, **k))[1])

    first = step(img1, img2, key_obj_mask=mask, key_obj_valid=valid)
    assert step.obj_cache.count == 2 and pastes == []
    # still filling: the step of today, bit for bit
    assert float(first) == float(plain(img1, img2)) and float(step.l_ot) == float(plain.l_ot)
    for a, b in zip(step.module.parameters(), plain.module.parameters()):
        assert torch.equal(a, b)
    second = step(img1, img2, key_obj_mask=mask, key_obj_valid=valid)
    assert step.obj_cache.count == 4 and pastes == [] and torch.isfinite(second)
    third = step(img1, img2, key_obj_mask=mask, key_obj_valid=valid)
    assert pastes == [2 * B] and step.obj_cache.count == 4  # key_obj_count rounds of B objects
    assert torch.isfinite(third) and torch.isfinite(step.l_ot) and float(step.l_ot) > 0
    assert bool(torch.isfinite(step.obj_cache.motion).all())
