"""The stage-1 augmentation branch without a GPU: include/unsamflow_hip_ar.h is
exported and bound, argument rejection before any device work, the theta
sampler and the torch composition of the transform against the reference
capture (tests/golden/ar_transform.npz, made by tests/golden/make_golden_ar.py),
the AR loss's torch path against a hand-written fp64 formula, random_crop, the
configs and a CPU TrainStep with the branch on."""
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ar_util
from conftest import REPO, load_golden

HEADER = REPO / "include" / "unsamflow_hip_ar.h"
SYMBOLS = ["usf_ar_api_version", "usf_ar_transform_f32", "usf_ar_loss_partials", "usf_ar_loss_fwd_f32",
           "usf_ar_loss_bwd_f32"]


@pytest.fixture(scope="module")
def lib():
    from unsamflow_amd import _lib
    from unsamflow_amd.build import build_library

    build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return load_golden("ar_transform.npz")


def header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def test_header_declares_exactly_the_bound_symbols():
    from unsamflow_amd import _lib

    declared = sorted(set(re.findall(r"\b(usf_\w+)\s*\(", header_text())))
    assert declared == sorted(SYMBOLS) == sorted(_lib.AR_SYMBOLS)
    assert not set(_lib.AR_SYMBOLS) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.CENSUS_SYMBOLS))
    for name, (argtypes, _) in _lib.AR_SYMBOLS.items():
        m = re.search(name + r"\s*\(([^)]*)\)", header_text())
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(argtypes), name


def test_library_exports_and_binds_the_entries(lib):
    from unsamflow_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.library_path())], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (usf_\w+)", out))
    for s in SYMBOLS:
        assert s in exported, s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.usf_ar_api_version() == _lib.AR_API_VERSION == 1
    assert lib.usf_abi_version() == 8


def test_build_id_covers_the_ar_sources():
    from unsamflow_amd import build

    assert "ar.hip" in build.SOURCES and HEADER.name in build.PUBLIC_HEADERS
    before = build.build_id()
    build.SOURCES.remove("ar.hip")
    try:
        assert build.build_id() != before
    finally:
        build.SOURCES.insert(build.SOURCES.index("census.hip") + 1, "ar.hip")
    assert build.build_id() == before


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc not available")
def test_ar_kernels_do_not_spill():
    """The transform, both loss instantiations of each direction and the
    finalisation: no scratch, at most 64 VGPRs (8 waves/SIMD), LDS only for the
    reductions' slots."""
    import sys

    sys.path.insert(0, str(REPO / "tools"))
    import kernel_resources

    res = kernel_resources.resources(REPO / "unsamflow_amd" / "csrc" / "ar.hip")
    assert len(res) == 6 and sum("ar_transform_kernel" in r[0] for r in res) == 1, [r[0] for r in res]
    for name, vgpr, lds, scratch in res:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 64 and lds <= 64, (name, vgpr, lds)


def test_partials_size(lib):
    # {sum l, sum noc} per workgroup of 1024 pixels of one sample
    assert lib.usf_ar_loss_partials(2, 64, 96) == 2 * 2 * 6
    assert lib.usf_ar_loss_partials(3, 2, 3) == 2 * 3
    assert lib.usf_ar_loss_partials(0, 8, 8) == 0


# dummy non-null pointers (never dereferenced: every call is rejected before a launch)
def _tf(L, img1=1, img2=1, flow=1, fbs=24, mask=1, theta=1, o1=1, o2=1, of=1, om=1, B=1, H=3, W=4):
    return L.usf_ar_transform_f32(img1, img2, flow, fbs, mask, theta, None, None, o1, o2, of, om, B, H, W, None)


def _fwd(L, pred=1, target=1, ts=(24, 12, 4), noc=1, ns=(12, 4), part=1, out=1, B=1, H=3, W=4, eps=0.0, q=1.0):
    return L.usf_ar_loss_fwd_f32(pred, target, *ts, noc, *ns, None, part, out, B, H, W, eps, q, None)


def _bwd(L, pred=1, target=1, ts=(24, 12, 4), noc=1, ns=(12, 4), coef=1, gl=1, gp=1, B=1, H=3, W=4, eps=0.0, q=1.0):
    return L.usf_ar_loss_bwd_f32(pred, target, *ts, noc, *ns, coef, gl, gp, B, H, W, eps, q, None)


# every pointer of _tf on a 16-byte boundary: the base of the alignment cases
_TF16 = dict(img1=16, img2=16, flow=16, mask=16, theta=16, o1=16, o2=16, of=16, om=16)


@pytest.mark.parametrize(
    "call,needle",
    [
        (lambda L: _tf(L, img1=None), "null input"),
        (lambda L: _tf(L, theta=None), "null input"),
        (lambda L: _tf(L, o1=None), "null output"),
        (lambda L: _tf(L, of=None), "null output"),
        (lambda L: _tf(L, om=None), "null output"),
        (lambda L: _tf(L, H=1), "H, W >= 2"),
        (lambda L: _tf(L, W=1), "H, W >= 2"),
        (lambda L: _tf(L, B=0), "non-positive"),
        (lambda L: _tf(L, B=-3), "non-positive"),
        (lambda L: _tf(L, B=2, fbs=23), "< 2*H*W"),
        (lambda L: _tf(L, H=16384, W=16384), "too large"),
        (lambda L: _fwd(L, pred=None), "null input"),
        (lambda L: _fwd(L, noc=None), "null input"),
        (lambda L: _fwd(L, out=None), "null output"),
        (lambda L: _fwd(L, part=None), "null output"),
        (lambda L: _fwd(L, H=1), "H, W >= 2"),
        (lambda L: _fwd(L, B=0), "non-positive"),
        (lambda L: _fwd(L, q=0.0), "q=0"),
        (lambda L: _fwd(L, q=-1.0), "q=-1"),
        (lambda L: _fwd(L, q=float("nan")), "need q > 0"),
        (lambda L: _fwd(L, eps=-0.5), "eps=-0.5"),
        (lambda L: _fwd(L, ts=(24, 12, -4)), "negative stride"),
        (lambda L: _fwd(L, ns=(-1, 4)), "negative stride"),
        (lambda L: _bwd(L, target=None), "null input"),
        (lambda L: _bwd(L, coef=None), "null input"),
        (lambda L: _bwd(L, gl=None), "null input"),
        (lambda L: _bwd(L, gp=None), "null output"),
        (lambda L: _bwd(L, W=1), "H, W >= 2"),
        (lambda L: _bwd(L, B=0), "non-positive"),
        (lambda L: _bwd(L, q=0.0), "q=0"),
        # the alignment contract (include/unsamflow_hip_ar.h): 20 where 16 bytes are required, 18 where 4
        (lambda L: _tf(L, **{**_TF16, "img2": 20}), "img2 must be 16-byte aligned"),
        (lambda L: _tf(L, **{**_TF16, "flow": 18}), "flow must be 4-byte aligned"),
        (lambda L: _tf(L, **{**_TF16, "theta": 18}), "theta must be 4-byte aligned"),
        (lambda L: _tf(L, **{**_TF16, "of": 24}), "flow_t must be 16-byte aligned"),
        (lambda L: _fwd(L, pred=18, target=16, noc=16, part=16, out=16), "pred must be 4-byte aligned"),
        (lambda L: _fwd(L, pred=20, target=18, noc=16, part=16, out=16), "target must be 4-byte aligned"),
        (lambda L: _fwd(L, pred=16, target=16, noc=16, part=20, out=16), "partials must be 16-byte aligned"),
        (lambda L: _fwd(L, pred=16, target=16, noc=16, part=16, out=18), "out must be 4-byte aligned"),
        (lambda L: _bwd(L, pred=16, target=16, noc=18, coef=16, gl=16, gp=16), "noc must be 4-byte aligned"),
        (lambda L: _bwd(L, pred=16, target=16, noc=16, coef=18, gl=16, gp=16), "coef must be 4-byte aligned"),
        (lambda L: _bwd(L, pred=20, target=20, noc=20, coef=20, gl=20, gp=20), "grad_pred must be 16-byte aligned"),
    ],
)
def test_invalid_arguments_rejected_without_launch(lib, call, needle):
    assert call(lib) == -1
    msg = lib.usf_last_error_string().decode()
    assert needle in msg, msg


def test_ops_refuse_what_the_abi_cannot_express():
    """A non-unit column stride (the entries take batch, channel and row
    strides only), q <= 0, wrong shapes and CPU tensors: refused before the library is touched."""
    from unsamflow_amd import ops

    pred, tgt, noc = torch.zeros(1, 2, 4, 6), torch.zeros(1, 2, 4, 12), torch.ones(1, 1, 4, 12)
    with pytest.raises(ValueError, match="column stride 2"):
        ops.ar_loss_forward(pred, tgt[..., ::2], noc[..., :6])
    with pytest.raises(ValueError, match="column stride 2"):
        ops.ar_loss_backward(pred, tgt[..., :6], noc[..., ::2], torch.zeros(2), torch.ones(1))
    with pytest.raises(ValueError, match="q > 0"):
        ops.ar_loss_forward(pred, tgt[..., :6], noc[..., :6], q=0.0)
    with pytest.raises(ValueError, match="shape"):
        ops.ar_loss_forward(pred, tgt, noc[..., :6])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ar_loss_forward(pred, tgt[..., :6], noc[..., :6])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ar_transform(torch.zeros(1, 3, 4, 6), torch.zeros(1, 3, 4, 6), pred, noc[..., :6],
                         ar_util.identity_thetas(1))


# ------------------------------------------------------------------ thetas --
@pytest.mark.parametrize("name", ["kitti", "sintel"])
def test_sample_thetas_equal_the_reference_under_its_seed(golden, name):
    from unsamflow_amd import ar, config

    st_cfg = getattr(config, f"{name}_stage1_ar")().train.st_cfg
    ref = golden[f"thetas_{name}"]
    H, W = (int(v) for v in golden[f"thetas_{name}_hw"])
    torch.manual_seed(int(golden["seed"]))
    th = ar.sample_thetas(st_cfg, ref.shape[1], H, W)
    assert th.shape == ref.shape == (2, 4, 6) and th.dtype == torch.float32 and th.device.type == "cpu"
    np.testing.assert_allclose(th.numpy(), ref, rtol=0, atol=1e-6)
    # an explicit generator in the same state draws the same thetas
    g = torch.Generator().manual_seed(int(golden["seed"]))
    assert torch.equal(ar.sample_thetas(st_cfg, ref.shape[1], H, W, generator=g), th)
    if name == "sintel":  # squeeze, vflip and +-0.2 rad leave their mark
        assert np.abs(ref[0, :, 1]).max() > 0.05 and (ref[0, :, 4] < 0).any()


@pytest.mark.parametrize("name,H,W", [("kitti", 256, 832), ("sintel", 448, 1024), ("sintel", 33, 70)])
def test_every_sampled_theta_is_valid(name, H, W):
    from unsamflow_amd import ar, config

    st_cfg = getattr(config, f"{name}_stage1_ar")().train.st_cfg
    g = torch.Generator().manual_seed(7)
    for _ in range(5):
        th = ar.sample_thetas(st_cfg, 8, H, W, generator=g)
        assert not bool(ar.find_invalid(th.reshape(-1, 6), H, W).any())
        assert bool(torch.isfinite(th).all())
    # find_invalid does reject: a shift by a whole image leaves the source
    bad = torch.tensor([[1.0, 0.0, 2.5, 0.0, 1.0, 0.0]])
    assert bool(ar.find_invalid(bad, H, W).all())


# --------------------------------------------------------------- transform --
TENSORS = ["img1_t", "img2_t", "flow_t", "mask_t"]
CASES = ["min_2x3", "odd_12x20", "wide_17x38", "identity_12x20"]


def _case(golden, name):
    B, H, W = (int(v) for v in golden[name + "_shape"])
    inp = ar_util.inputs(B, H, W, int(golden[name + "_seed"]), lo=0.1 if name.startswith("identity") else 0.0)
    return inp, torch.from_numpy(golden[name + "_thetas"]), (B, H, W)


@pytest.mark.parametrize("name", CASES)
def test_torch_composition_matches_the_reference_capture(golden, name):
    """Per tensor: max|fp32 - capture| <= max|capture - fp64| (the restatement is
    no further from the reference than the reference is from exact arithmetic)
    and max|capture - fp64| <= 1e-4 max(1, max|capture|)."""
    from unsamflow_amd import ar

    inp, th, (B, H, W) = _case(golden, name)
    o32 = ar.spatial_transform(*inp, th)
    o64 = ar.spatial_transform(*[t.double() for t in inp], th)
    for k, a, b in zip(TENSORS, o32, o64):
        cap = golden[f"{name}_{k}"]
        assert a.dtype == torch.float32 and b.dtype == torch.float64 and tuple(a.shape) == cap.shape
        d32 = float(np.abs(a.numpy() - cap).max())
        d64 = float(np.abs(cap - b.numpy()).max())
        print(f"[ar] {name} {k}: |fp32-cap|={d32:.3e} |cap-fp64|={d64:.3e} max|cap|={np.abs(cap).max():.3e}")
        assert d32 <= d64, (name, k, d32, d64)
        assert d64 <= 1e-4 * max(1.0, float(np.abs(cap).max())), (name, k, d64)
    if not name.startswith("identity"):
        assert ar_util.zeroed_fraction(th[0], H, W)[0] > 0.1 and th[0, 1, 0] < 0
        zeroed = (golden[f"{name}_img1_t"][0] == 0).all(axis=0).mean()
        assert zeroed == pytest.approx(ar_util.zeroed_fraction(th[0], H, W)[0], abs=1e-9)


def test_identity_thetas_return_the_inputs(golden):
    """Images and mask within 2e-6 (inputs in [0.1, 1]); no pixel zeroed. The
    flow passes through ~12 rounded operations on coordinates of magnitude up to
    W + max|u| < 64 px: 16 ulp of that binade = 16 * 2^-23 * 64 = 1.2e-4."""
    from unsamflow_amd import ar

    (img1, img2, flow, mask), th, (B, H, W) = _case(golden, "identity_12x20")
    assert torch.equal(th, ar_util.identity_thetas(B)) and float(img1.min()) >= 0.1
    o1, o2, of, om = ar.spatial_transform(img1, img2, flow, mask, th)
    for name, a, b in (("img1", o1, img1), ("img2", o2, img2), ("mask", om, mask)):
        err = float((a - b).abs().max())
        print(f"[ar] identity {name}: {err:.3e}")
        assert err <= 2e-6, (name, err)
    assert float(o1.min()) > 0.09 and float(o2.min()) > 0.09
    assert W + float(flow.abs().max()) < 64
    assert float((of - flow).abs().max()) <= 16 * 2.0 ** -23 * 64
    assert float((of.abs().sum(1) == 0).float().sum()) == 0


def test_noise_is_added_then_clamped(golden):
    from unsamflow_amd import ar

    inp, th, (B, H, W) = _case(golden, "odd_12x20")
    n1 = torch.from_numpy(ar_util.hashrng.normal((B, 3, H, W), 77)) * 0.5
    n2 = torch.from_numpy(ar_util.hashrng.normal((B, 3, H, W), 78)) * 0.5
    base = ar.spatial_transform(*inp, th)
    out = ar.spatial_transform(*inp, th, n1, n2)
    assert torch.equal(out[0], (base[0] + n1).clamp(0, 1)) and torch.equal(out[1], (base[1] + n2).clamp(0, 1))
    assert torch.equal(out[2], base[2]) and torch.equal(out[3], base[3])
    assert float(out[0].min()) == 0.0 and float(out[0].max()) == 1.0


def test_module_keeps_the_reference_dict_interface():
    from unsamflow_amd import ar, config

    st_cfg = config.kitti_stage1_ar().train.st_cfg
    B, H, W = 2, 16, 24
    img1, img2, flow, mask = ar_util.inputs(B, H, W, 5)
    g = torch.Generator().manual_seed(3)
    m = ar.RandomAffineFlow(st_cfg, addnoise=False, generator=g)
    out = m({"imgs": [img1, img2], "flows_f": [flow], "masks_f": [mask]})  # no full_segs key: accepted
    th = ar.sample_thetas(st_cfg, B, H, W, generator=torch.Generator().manual_seed(3))
    ref = ar.spatial_transform(img1, img2, flow, mask, th)
    for a, b in zip(out["imgs"] + out["flows_f"] + out["masks_f"], ref):
        assert torch.equal(a, b)
    assert "full_segs" not in out
    # three frames with segment maps: the general composition, the reference's list handling
    g = torch.Generator().manual_seed(3)
    m = ar.RandomAffineFlow(st_cfg, addnoise=True, generator=g)
    seg = torch.ones(B, 1, H, W)
    out = m({"imgs": [img1, img2, img1], "full_segs": [seg, seg, seg], "flows_f": [flow, flow], "masks_f": [mask]})
    assert len(out["imgs"]) == 3 and len(out["full_segs"]) == 3 and len(out["flows_f"]) == 0
    assert out["imgs"][0].shape == img1.shape and 0.0 <= float(out["imgs"][0].min())
    assert float(out["imgs"][0].max()) <= 1.0


# ----------------------------------------------------------------- AR loss --
def _loss_inputs(B=2, H=9, W=14, seed=50):
    pred = torch.from_numpy(ar_util.hashrng.normal((B, 2, H, W), seed)) * 3.0
    target = torch.from_numpy(ar_util.hashrng.normal((B, 2, H, W), seed + 1)) * 3.0
    noc = (torch.from_numpy(ar_util.hashrng.uniform((B, 1, H, W), seed + 2)) > 0.4).float()
    target[:, :, 2:5, 3:8] = pred[:, :, 2:5, 3:8]  # a block of exact agreement
    return pred, target, noc


def _hand_loss(pred, target, noc, eps, q, denom=None):
    """fp64 by hand: (value, gradient w.r.t. pred)."""
    p, t, n = pred.double().numpy(), target.double().numpy(), noc.double().numpy()
    d = p - t
    N = d.size
    D = (n.mean() if denom is None else float(denom)) + 1e-7
    val = (((np.abs(d) + eps) ** q) * n).sum() / N / D
    with np.errstate(divide="ignore", invalid="ignore"):
        g = q * (np.abs(d) + eps) ** (q - 1) * np.sign(d) * n / (N * D)
    g[np.broadcast_to(d == 0, g.shape)] = 0.0
    return val, g


@pytest.mark.parametrize("eps,q", [(0.0, 1.0), (0.01, 0.4)])
@pytest.mark.parametrize("with_denom", [False, True])
def test_ar_loss_torch_path_matches_hand_formula(eps, q, with_denom):
    from unsamflow_amd import ar

    pred, target, noc = _loss_inputs()
    denom = torch.tensor(0.37, dtype=torch.float64) if with_denom else None
    p = pred.double().requires_grad_(True)
    loss = ar.ar_loss(p, target.double(), noc.double(), eps, q, denom)
    loss.backward()
    val, g = _hand_loss(pred, target, noc, eps, q, None if denom is None else 0.37)
    np.testing.assert_allclose(float(loss.detach()), val, rtol=1e-12)
    np.testing.assert_allclose(p.grad.numpy(), g, rtol=1e-10, atol=1e-18)
    assert float(p.grad[:, :, 2:5, 3:8].abs().max()) == 0.0  # pred == target: exactly 0
    # fp32: the value within fp32 summation error of the fp64 one
    l32 = ar.ar_loss(pred, target, noc, eps, q, None if denom is None else denom.float())
    np.testing.assert_allclose(float(l32), val, rtol=2e-5)


def test_ar_loss_on_a_crop_view():
    from unsamflow_amd import ar

    pred, target, noc = _loss_inputs(2, 16, 24, 60)
    g = torch.Generator().manual_seed(1)
    _, tc, nc = ar.random_crop(torch.zeros(2, 6, 16, 24), target, noc, (9, 14), g)
    assert not tc.is_contiguous() and tc.stride(-1) == 1
    p = pred[:, :, :9, :14].double().contiguous().requires_grad_(True)
    loss = ar.ar_loss(p, tc.double(), nc.double(), 0.0, 1.0)
    loss.backward()
    val, grad = _hand_loss(p.detach(), tc.contiguous(), nc.contiguous(), 0.0, 1.0)
    np.testing.assert_allclose(float(loss.detach()), val, rtol=1e-12)
    np.testing.assert_allclose(p.grad.numpy(), grad, rtol=1e-10, atol=1e-18)


def test_ar_loss_refuses_gradients_into_target_or_mask():
    from unsamflow_amd import ar

    pred, target, noc = _loss_inputs()
    with pytest.raises(NotImplementedError):
        ar.ar_loss(pred, target.clone().requires_grad_(True), noc)
    with pytest.raises(NotImplementedError):
        ar.ar_loss(pred, target, noc.clone().requires_grad_(True))


def test_random_crop():
    from unsamflow_amd import ar

    imgs, flow, noc = torch.rand(2, 6, 16, 24), torch.rand(2, 2, 16, 24), torch.rand(2, 1, 16, 24)
    g = torch.Generator().manual_seed(0)
    seen = set()
    for _ in range(20):
        a, b, c = ar.random_crop(imgs, flow, noc, (9, 14), g)
        assert a.shape == (2, 6, 9, 14) and b.shape == (2, 2, 9, 14) and c.shape == (2, 1, 9, 14)
        off = a.storage_offset()
        y1, x1 = off // 24, off % 24
        assert 0 <= y1 < 16 - 9 and 0 <= x1 < 24 - 14  # randint's half-open range, as the reference
        assert torch.equal(a, imgs[:, :, y1:y1 + 9, x1:x1 + 14]) and torch.equal(b, flow[:, :, y1:y1 + 9, x1:x1 + 14])
        assert torch.equal(c, noc[:, :, y1:y1 + 9, x1:x1 + 14])
        assert a.data_ptr() == imgs[:, :, y1:, x1:].data_ptr()  # a view, not a copy
        seen.add((y1, x1))
    assert len(seen) > 5
    # an equal dimension: offset 0 (the reference's randint(0, 0) raises)
    a, b, c = ar.random_crop(imgs, flow, noc, (16, 14), g)
    assert a.shape == (2, 6, 16, 14) and a.storage_offset() < 24
    a, b, c = ar.random_crop(imgs, flow, noc, (16, 24), g)
    assert a is imgs and b is flow and c is noc
    with pytest.raises(ValueError):
        ar.random_crop(imgs, flow, noc, (17, 24), g)


# ------------------------------------------------------- configs and step --
@pytest.mark.parametrize("name,ot_size,rot,vflip", [("kitti", [192, 640], [-0.01, 0.01, -0.01, 0.01], False),
                                                    ("sintel", [320, 704], [-0.2, 0.2, -0.015, 0.015], True)])
def test_stage1_ar_configs_carry_the_json_values(name, ot_size, rot, vflip):
    from unsamflow_amd import config

    cfg, s1 = getattr(config, f"{name}_stage1_ar")(), getattr(config, f"{name}_stage1")()
    t = cfg.train
    assert (t.w_ar, t.ar_eps, t.ar_q, t.mask_st) == (0.02, 0.0, 1.0, True)
    assert t.run_atst is True and t.run_st is True and t.run_ot is True and t.key_obj_aug is False
    assert t.ot_size == ot_size and t.st_cfg.rotate == rot and t.st_cfg.vflip is vflip
    assert t.st_cfg.add_noise is True and t.st_cfg.hflip is True and len(t.st_cfg.zoom) == 4
    assert cfg.loss == s1.loss and cfg.model == s1.model and cfg.data == s1.data
    assert {k: v for k, v in t.items() if k in s1.train} == dict(s1.train)  # the base train keys are untouched
    assert "run_atst" not in s1.train and "st_cfg" not in s1.train


@pytest.fixture(scope="module")
def cpu_steps():
    """One step each at 1x64x128 from one seed: the AR step, the AR step with
    w_ar = 0, and the stage-1 step without the branch (oracle-backed ops). A
    freshly initialised PWCLite answers noise frames with bias-driven flows of
    several pixels in both directions, which the bidirectional check calls
    occluded everywhere (loss 0, mask 0); the weights are scaled by 0.02 so the
    flows are small, the mask is 1 and every term has something to measure."""
    from oracle.torch_ref import (OracleCorrelation, oracle_flow_warp, oracle_occu_mask_backward,
                                  oracle_occu_mask_bidirection)
    from unsamflow_amd.config import kitti_stage1, kitti_stage1_ar
    from unsamflow_amd.harness import TrainStep, synthetic_pair

    img1, img2, _, _ = synthetic_pair(1, 64, 128, "cpu")
    out = {}
    for key in ("ar", "w0", "plain"):
        cfg = kitti_stage1() if key == "plain" else kitti_stage1_ar()
        if key != "plain":
            cfg.train.ot_size = [64, 64]
        if key == "w0":
            cfg.train.w_ar = 0.0
        step = TrainStep(cfg, "cpu", corr_module=OracleCorrelation(4), warp_fn=oracle_flow_warp,
                         occ_backward_fn=oracle_occu_mask_backward,
                         loss_kwargs=dict(occ_bidir_fn=oracle_occu_mask_bidirection))
        with torch.no_grad():
            for p in step.module.parameters():
                p.mul_(0.02)
        calls = []
        fwd = step.module.forward
        step.module.forward = lambda *a, _f=fwd, **k: (calls.append((tuple(a[0].shape), k.get("with_bk"))), _f(*a, **k))[1]
        before = [p.detach().clone() for p in step.module.parameters()]
        loss = step(img1, img2)
        out[key] = (step, loss, before, calls)
    return out


def test_cpu_train_step_runs_the_three_passes(cpu_steps):
    step, loss, before, calls = cpu_steps["ar"]
    assert calls == [((1, 3, 64, 128), True), ((1, 3, 64, 128), False), ((1, 3, 64, 64), False)]
    assert torch.isfinite(loss)
    for l in (step.l_atst, step.l_ot):
        assert l is not None and not l.requires_grad and torch.isfinite(l) and float(l) > 0
    assert any(not torch.equal(a, p) for a, p in zip(before, step.module.parameters()))
    plain = cpu_steps["plain"]
    assert plain[0].has_ar is False and plain[0].l_atst is None and len(plain[3]) == 1
    expect = float(plain[1]) + 0.02 * (float(step.l_atst) + float(step.l_ot))
    assert float(loss) == pytest.approx(expect, rel=1e-6)


def test_cpu_train_step_with_zero_weight_equals_the_plain_step(cpu_steps):
    assert len(cpu_steps["w0"][3]) == 3 and float(cpu_steps["plain"][1]) > 0
    assert float(cpu_steps["w0"][1]) == float(cpu_steps["plain"][1])
