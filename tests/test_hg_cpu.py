"""The homography smoothness loss without a GPU: the torch restatement of the
reference's loop against the golden captured from the reference with a stub
estimator (tests/golden/make_golden_hg.py), unFlowLoss running it on the CPU,
the numpy RANSAC recovering planted homographies, include/unsamflow_hip_hg.h
exported and bound, argument rejection before any device work, and the stage-2
configs."""
import re
import subprocess

import numpy as np
import pytest
import torch

import hg_util as hu
from conftest import REPO, load_golden

HEADER = REPO / "include" / "unsamflow_hip_hg.h"
SYMBOLS = ["usf_hg_api_version", "usf_hg_workspace_bytes", "usf_hg_fit_f32", "usf_hg_loss_partials",
           "usf_hg_loss_fwd_f32", "usf_hg_loss_bwd_f32"]
EINVAL = -1  # USF_EINVAL


@pytest.fixture(scope="module")
def lib():
    from unsamflow_amd import _lib
    from unsamflow_amd.build import build_library

    build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return load_golden("hg_smooth.npz")


# ----------------------------------------------------------------- golden --
@pytest.mark.parametrize("name", list(hu.GOLDEN_CASES))
def test_torch_loop_reproduces_the_reference(golden, name):
    """Same stub estimator, same inputs: the order of the estimator calls, each call's point count and H,
    the loss and dloss/dflo of the reference's own smooth_homography."""
    from unsamflow_amd.homography import smooth_homography_torch

    flow, seg, occ = hu.golden_inputs(name)
    for k, t in (("flow", flow), ("seg", seg), ("occ", occ)):
        assert np.array_equal(golden[f"{name}_{k}"], t.numpy()), k  # the stored inputs are the regenerated ones
    calls, samples = [], []
    stub = hu.stub_estimator(calls)

    def estimator(p1, p2, thr, sample, slot):
        samples.append(sample)
        return stub(p1, p2, thr)

    flo = flow.clone().requires_grad_(True)
    loss = smooth_homography_torch(flo, seg, occ, float(golden["thr"]), hu.GOLDEN_CASES[name][3], estimator)
    (grad,) = torch.autograd.grad(loss, flo)
    assert samples == golden[f"{name}_call_sample"].tolist()
    assert [c[0] for c in calls] == golden[f"{name}_call_npts"].tolist()
    assert len(calls) > 0
    np.testing.assert_allclose(np.array([c[1] for c in calls]), golden[f"{name}_call_H"], rtol=1e-9, atol=1e-12)
    want, gwant = float(golden[f"{name}_loss"]), golden[f"{name}_grad"]
    scale = max(abs(want), 1.0)
    print(f"[hg] {name}: loss {float(loss.detach()):.9g} golden {want:.9g} "
          f"grad err {np.abs(grad.numpy() - gwant).max():.3e}")
    assert abs(float(loss.detach()) - want) <= 1e-6 * scale
    assert np.abs(grad.numpy() - gwant).max() <= 1e-6 * scale
    if name == "b2_24x40":
        assert want > 0 and np.count_nonzero(gwant) > 0


def test_num_segments_none_reads_the_maximum(golden):
    from unsamflow_amd.homography import smooth_homography_torch

    flow, seg, occ = hu.golden_inputs("b2_24x40")
    a = smooth_homography_torch(flow, seg, occ, 0.5, None, hu.stub_estimator([]))
    b = smooth_homography_torch(flow, seg, occ, 0.5, 12, hu.stub_estimator([]))  # ids without a pixel change nothing
    assert float(a) == float(b) == pytest.approx(float(golden["b2_24x40_loss"]), abs=1e-6)


# ------------------------------------------------------------- unFlowLoss --
def _loss_inputs(seed, B=1, h=64, w=96):
    g = torch.Generator().manual_seed(seed)
    f12, s1, o1, K, _ = hu.planted_scene(4100)
    f21, s2, o2, _, _ = hu.planted_scene(4300)
    top = torch.cat([f12[:B], f21[:B]], 1)
    flows = [top] + [torch.zeros(B, 4, h >> i, w >> i) for i in range(1, 5)]
    # the occlusion masks are the scene's: the bidirectional check of two unrelated flows occludes everything
    occ = lambda a, b: (o1 if a.storage_offset() == 0 else o2)[:B]  # noqa: E731
    return flows, torch.rand(B, 3, h, w, generator=g), torch.rand(B, 3, h, w, generator=g), s1[:B], s2[:B], occ


def test_unflowloss_runs_homography_smoothness_on_the_cpu():
    from oracle.torch_ref import oracle_flow_warp
    from unsamflow_amd.config import kitti_stage2_hg
    from unsamflow_amd.flow_loss import unFlowLoss
    from unsamflow_amd.homography import smooth_homography_torch

    cfg = kitti_stage2_hg().loss
    flows, im1, im2, s1, s2, occ = _loss_inputs(3)
    loss_fn = unFlowLoss(cfg, warp_fn=oracle_flow_warp, occ_bidir_fn=occ)
    flows[0].requires_grad_(True)
    loss, l_ph, l_sm, _, vis1, vis2 = loss_fn(flows, im1, im2, full_seg1=s1, full_seg2=s2)
    top = flows[0].detach()
    a = smooth_homography_torch(top[:, :2], s1, 1 - vis1, cfg.ransac_threshold)
    b = smooth_homography_torch(top[:, 2:], s2, 1 - vis2, cfg.ransac_threshold)
    assert cfg.ransac_threshold == 0.5
    l_sm, l_ph, total = float(l_sm.detach()), float(l_ph.detach()), float(loss.detach())
    assert l_sm == pytest.approx(float((a + b) / 2.0), rel=1e-6)
    assert l_sm > 0
    assert total == pytest.approx(l_ph + 0.1 * l_sm, rel=1e-5)
    loss.sum().backward()
    assert torch.isfinite(flows[0].grad).all()
    # without the segment maps it stays an error that says what is missing
    with pytest.raises(NotImplementedError, match="segment maps"):
        loss_fn(flows, im1, im2)


# -------------------------------------------------------- numpy estimator --
def test_numpy_ransac_recovers_the_planted_homographies():
    """The scene of the GPU recovery test: the final inlier set is the planted one, the 60 % segment is
    rejected, the 2x2 block is fitted from its 4 points, and H acts as the fp64 refit on the inliers
    of the winning hypothesis to 1e-3 px over the whole image."""
    from unsamflow_amd import homography as hg

    flow, seg, occ, K, planted = hu.planted_scene()
    px = hu.all_pixels(64, 96)
    worst = 0.0
    for (b, k), want in planted.items():
        p1, p2 = hu.slot_pairs(flow, seg, occ, b, k)
        slot = 6 - k  # any slot: the stream is a function of it
        info = {}
        H, mask = hg.ransac_homography_np(p1, p2, 0.5, b, slot, info=info)
        assert H is not None and H.dtype == np.float32
        if want["kind"] == "outliers":
            assert mask.mean() < 0.5
            continue
        assert np.array_equal(mask, want["inliers"]), (b, k)
        Hs, valid = hg.hypotheses_np(p1, p2, b, slot)
        assert valid[info["best_j"]]
        inl0 = hg.inliers_np(Hs[info["best_j"]], p1, p2, 0.5)
        H_ref = hg.refit_homography_np(p1[inl0], p2[inl0])
        if want["kind"] == "block":
            # four points 1 px apart fix a homography whose denominator crosses zero inside the image, so
            # its action is compared where the fit lives: on the block's own pixels
            assert mask.sum() == 4
            worst = max(worst, float(np.abs(hu.apply_h(H, p1.astype(np.float64))
                                            - hu.apply_h(H_ref, p1.astype(np.float64))).max()))
            continue
        worst = max(worst, float(np.abs(hu.apply_h(H, px) - hu.apply_h(H_ref, px)).max()))
        # and close to the planted plane inside the segment (0.02 px noise on > 500 inliers)
        assert np.abs(hu.apply_h(H, p1.astype(np.float64)) - hu.apply_h(want["H"], p1.astype(np.float64))).max() < 0.02
    print(f"[hg] numpy estimator: max |H p - H_ref p| = {worst:.3e} px")
    assert worst <= 1e-3


def test_hash_stream_is_the_headers():
    """q_t = ((mix(mix(seed) + c) >> 32) * n_rel) >> 32 with c = ((sample * 8 + slot) << 34) | (j << 2) | t."""
    from unsamflow_amd.homography import hypothesis_positions

    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    q = hypothesis_positions(1000, 3, 5, n_hyp=7, seed=99)
    for j in range(7):
        for t in range(4):
            c = ((3 * 8 + 5) << 34) | (j << 2) | t
            assert q[j, t] == ((mix((mix(99) + c) & M) >> 32) * 1000) >> 32
    assert q.min() >= 0 and q.max() < 1000
    assert "0x9E3779B97F4A7C15" in HEADER.read_text() and "<< 34" in HEADER.read_text()


def test_public_op_on_cpu_is_the_composition():
    from unsamflow_amd import homography as hg

    flow, seg, occ = hu.golden_inputs("b1_5x7")
    assert float(hg.smooth_homography(flow, seg, occ, 0.5)) == float(hg.smooth_homography_torch(flow, seg, occ, 0.5))
    with pytest.raises(RuntimeError, match="no CPU path"):
        hg.smooth_homography(flow, seg, occ, 0.5, 4, fused=True)


# ------------------------------------------------------------------ C ABI --
def header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def test_header_declares_exactly_the_bound_symbols():
    from unsamflow_amd import _lib, build

    declared = sorted(set(re.findall(r"\b(usf_\w+)\s*\(", header_text())))
    assert declared == sorted(SYMBOLS) == sorted(_lib.HG_SYMBOLS)
    others = set(_lib.EXPORTED_SYMBOLS) | set(_lib.CENSUS_SYMBOLS) | set(_lib.AR_SYMBOLS) | set(_lib.SEGPOOL_SYMBOLS)
    assert not set(_lib.HG_SYMBOLS) & others
    for name, (argtypes, _) in _lib.HG_SYMBOLS.items():
        m = re.search(name + r"\s*\(([^)]*)\)", header_text())
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(argtypes), name
    text = HEADER.read_text()
    assert int(re.search(r"#define USF_HG_API_VERSION (\d+)", text).group(1)) == _lib.HG_API_VERSION
    assert int(re.search(r"#define USF_HG_MAX_K (\d+)", text).group(1)) == _lib.HG_MAX_K == _lib.SEGPOOL_MAX_K
    assert int(re.search(r"#define USF_HG_SLOTS (\d+)", text).group(1)) == _lib.HG_SLOTS == 6
    assert int(re.search(r"#define USF_HG_RECORD_WORDS (\d+)", text).group(1)) == _lib.HG_RECORD_WORDS
    assert int(re.search(r"#define USF_HG_DEFAULT_HYP (\d+)", text).group(1)) == _lib.HG_DEFAULT_HYP == 256
    bit = int(re.search(r"#define USF_DEVERR_HG_BAD_ID (\d+)", text).group(1))
    assert bit == _lib.DEVERR_HG_BAD_ID == 8 and bit != _lib.DEVERR_SEGPOOL_BAD_ID
    for code, name in enumerate(["ACCEPTED", "FEW_RELIABLE", "LOW_RELIABLE", "LOW_INLIER", "DEGENERATE", "EMPTY"]):
        assert int(re.search(rf"#define USF_HG_{name} (\d+)", text).group(1)) == code
    assert len(_lib.HG_STATUS) == 6
    assert "hg.hip" in build.SOURCES and HEADER.name in build.PUBLIC_HEADERS


def test_library_exports_and_binds_the_entries(lib):
    from unsamflow_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.library_path())], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (usf_\w+)", out))
    for s in SYMBOLS:
        assert s in exported, s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.usf_hg_api_version() == _lib.HG_API_VERSION == 1
    assert lib.usf_abi_version() == _lib.ABI_VERSION == 8  # the main header and its version are untouched


def test_workspace_and_partials_queries(lib):
    # [B][3][K] statistics, [B][6][n_hyp] scores, [B][6][n_hyp][12] hypotheses, [B][HW] list, in 32-bit words
    assert lib.usf_hg_workspace_bytes(2, 24, 40, 9, 256) == 4 * (2 * 27 + 2 * 6 * 256 * 13 + 2 * 960)
    assert lib.usf_hg_workspace_bytes(1, 5, 7, 3, 1) % 8 == 0
    for bad in [(0, 5, 7, 3, 8), (1, 0, 7, 3, 8), (1, 5, 7, 0, 8), (1, 5, 7, 1025, 8), (1, 5, 7, 3, 0)]:
        assert lib.usf_hg_workspace_bytes(*bad) == 0, bad
    assert lib.usf_hg_loss_partials(2, 33, 47) == 2 * 2  # 1024 pixels per workgroup
    assert lib.usf_hg_loss_partials(0, 3, 4) == 0


# dummy non-null pointers (never dereferenced: every call is rejected before a launch)
def _fit(L, flow=8, fbs=24, seg=8, occ=8, K=5, thr=0.5, n_hyp=16, rec=8, ws=8, wsb=1 << 30, B=1, H=3, W=4):
    return L.usf_hg_fit_f32(flow, fbs, seg, occ, K, thr, n_hyp, 0, rec, ws, wsb, B, H, W, None)


@pytest.mark.parametrize("kw,what", [
    (dict(K=0), "K=0"), (dict(K=1025), "K=1025"), (dict(n_hyp=0), "n_hyp=0"), (dict(thr=0.0), "thr"),
    (dict(thr=-1.0), "thr"), (dict(thr=float("nan")), "thr"), (dict(flow=None), "null input"),
    (dict(seg=None), "null input"), (dict(occ=None), "null input"), (dict(rec=None), "null output"),
    (dict(ws=None), "null output"), (dict(wsb=16), "workspace"), (dict(fbs=23), "flow_bstride"),
    (dict(B=0), "shape"), (dict(ws=12), "aligned"),
    # the alignment contract (include/unsamflow_hip_hg.h): 20 where 16 bytes are required, 18 where 4
    (dict(flow=16, seg=20, occ=16, rec=16, ws=16), "seg must be 16-byte aligned"),
    (dict(flow=16, seg=16, occ=24, rec=16, ws=16), "occ must be 16-byte aligned"),
    (dict(flow=18, seg=16, occ=16, rec=16, ws=16), "flow must be 4-byte aligned"),
    (dict(flow=16, seg=16, occ=16, rec=18, ws=16), "records not 4-byte"),
])
def test_fit_rejects_bad_arguments_before_the_device(lib, kw, what):
    assert _fit(lib, **kw) == EINVAL
    assert what in lib.usf_last_error_string().decode()


def test_loss_entries_reject_bad_arguments_before_the_device(lib):
    fwd = lambda **k: lib.usf_hg_loss_fwd_f32(*[{**dict(flow=8, fbs=24, seg=8, rec=8, part=8, out=8, B=1, H=3, W=4),  # noqa: E731
                                                 **k}[n] for n in ("flow", "fbs", "seg", "rec", "part", "out", "B", "H", "W")], None)
    bwd = lambda **k: lib.usf_hg_loss_bwd_f32(*[{**dict(flow=8, fbs=24, seg=8, rec=8, g=8, gf=8, B=1, H=3, W=4),  # noqa: E731
                                                 **k}[n] for n in ("flow", "fbs", "seg", "rec", "g", "gf", "B", "H", "W")], None)
    for fn, outs in ((fwd, ("part", "out")), (bwd, ("gf",))):
        for name in ("flow", "seg", "rec"):
            assert fn(**{name: None}) == EINVAL and "null input" in lib.usf_last_error_string().decode()
        for name in outs:
            assert fn(**{name: None}) == EINVAL and "null output" in lib.usf_last_error_string().decode()
        assert fn(fbs=5) == EINVAL and "flow_bstride" in lib.usf_last_error_string().decode()
        assert fn(H=0) == EINVAL
    assert bwd(g=None) == EINVAL and "null input" in lib.usf_last_error_string().decode()
    # the alignment contract: 20 where 16 bytes are required, 18 where 4 are
    al = dict(flow=16, seg=16, rec=16)
    for call, kw, what in ((fwd, dict(seg=20), "seg must be 16-byte aligned"),
                           (fwd, dict(flow=18), "flow must be 4-byte aligned"),
                           (fwd, dict(out=18), "out must be 4-byte aligned"),
                           (fwd, dict(part=20), "partials not 8-byte aligned"),
                           (bwd, dict(seg=24), "seg must be 16-byte aligned"),
                           (bwd, dict(g=18), "grad_loss must be 4-byte aligned"),
                           (bwd, dict(gf=20), "grad_flow must be 16-byte aligned")):
        base = {**al, **(dict(part=16, out=16) if call is fwd else dict(g=16, gf=16))}
        assert call(**{**base, **kw}) == EINVAL
        assert what in lib.usf_last_error_string().decode(), (kw, lib.usf_last_error_string())


def test_hg_kernels_do_not_spill():
    """No kernel of hg.hip uses scratch -- the fp64 8x8 solves included, which stay in registers (144 VGPRs
    for the one-lane-per-hypothesis solve, 200 for the refit)."""
    import shutil
    import sys

    if shutil.which("/opt/rocm/bin/hipcc") is None:
        pytest.skip("hipcc not available")
    sys.path.insert(0, str(REPO / "tools"))
    import kernel_resources

    res = kernel_resources.resources(REPO / "unsamflow_amd" / "csrc" / "hg.hip")
    assert len(res) == 10, [r[0] for r in res]
    for name, vgpr, lds, scratch in res:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 256 and lds <= 16384, (name, vgpr, lds)


# ----------------------------------------------------------------- config --
def test_stage2_configs_carry_the_json_values():
    from unsamflow_amd.config import kitti_stage1_ar, kitti_stage2_hg, sintel_stage1_ar, sintel_stage2_hg

    k, s = kitti_stage2_hg(), sintel_stage2_hg()
    for cfg, base in ((k, kitti_stage1_ar()), (s, sintel_stage1_ar())):
        assert cfg.loss.smooth_type == "homography" and cfg.loss.w_sm == 0.1
        assert cfg.train.w_ar == 0.1 and cfg.train.key_obj_aug is False
        changed = {key for key in cfg.loss if cfg.loss.get(key) != base.loss.get(key)}
        assert changed <= {"smooth_type", "w_sm", "ransac_threshold"}
        assert {key for key in cfg.train if cfg.train[key] != base.train[key]} == {"w_ar"}
    assert k.loss.ransac_threshold == 0.5 and "ransac_threshold" not in s.loss
    from unsamflow_amd.flow_loss import unFlowLoss

    assert unFlowLoss(s.loss).cfg.ransac_threshold == 3
