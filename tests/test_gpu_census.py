"""Fused census (ternary) loss (unsamflow_amd.census, csrc/census.hip) vs the
reference composition on the CPU: torch grid_sample on norm_grid coordinates
(oracle_flow_warp) + flow_loss.TernaryLoss under loss_photomatric's normaliser,
evaluated in fp32 and again in fp64 on the same inputs.

Loss value against the fp64 composition: rtol 2e-5 (the photometric figure).

Flow gradient: the reference's own fp32 rounding is large for this loss (its
fp32 vs fp64 gradients differ by 6e-6 .. 4e-4 of max|grad| on these shapes), so
the bound comes from the reference inside the test:
    e_ref = max|g_fp32 - g_fp64|       (the CPU composition)
    max|g_gpu - g_fp64| <= max(4 e_ref, 2e-4 max|g_fp64|)
The factor 4 covers another summation and contraction order of the same fp32
quantities; the floor is the photometric gradient tolerance. A missing or
mis-signed term is an error of order max|grad|. Every figure is printed before
it is asserted (pytest -s)."""
import numpy as np
import pytest
import torch

from oracle import hashrng
from oracle.torch_ref import oracle_flow_warp

pytestmark = pytest.mark.gpu


def _ref_term(flow, src, tgt, mask, pad, w=1.0):
    """w * TernaryLoss(rec m, tgt m).mean() / (m.mean() + 1e-6) (flow_loss.py:33-50, w_ternary only)."""
    from unsamflow_amd.flow_loss import TernaryLoss

    rec = oracle_flow_warp(src, flow, pad=pad)
    return w * TernaryLoss(rec * mask, tgt * mask).mean() / (mask.mean() + 1e-6)


def _ref_both(fn, flow):
    """(loss_fp64, grad_fp32, grad_fp64) of fn(flow, dtype) on the CPU."""
    out = []
    for dt in (torch.float32, torch.float64):
        f = flow.detach().clone().to(dt).requires_grad_(True)
        loss = fn(f, dt)
        loss.backward()
        out.append((float(loss.detach()), f.grad.double().numpy()))
    return out[1][0], out[0][1], out[1][1]


def _check_grad(name, g_gpu, g32, g64):
    e_ref = float(np.abs(g32 - g64).max())
    gmax = float(np.abs(g64).max())
    err = float(np.abs(np.asarray(g_gpu, dtype=np.float64) - g64).max())
    bound = max(4.0 * e_ref, 2e-4 * gmax)
    print(f"[census] {name}: err={err:.3e} e_ref={e_ref:.3e} err/e_ref={err / max(e_ref, 1e-300):.3f} "
          f"max|g|={gmax:.3e} bound={bound:.3e}")
    assert err <= bound, (name, err, e_ref, gmax)


def _inputs(B, H, W, scale, mkind, seed):
    src = torch.from_numpy(hashrng.uniform((B, 3, H, W), seed))
    tgt = torch.from_numpy(hashrng.uniform((B, 3, H, W), seed + 1))
    flow = torch.from_numpy(hashrng.symmetric((B, 4, H, W), seed + 2, scale))
    if mkind == "ones":
        mask = torch.ones(B, 1, H, W)
    elif mkind == "zero":
        mask = torch.zeros(B, 1, H, W)
    else:
        mask = (torch.from_numpy(hashrng.uniform((B, 1, H, W), seed + 3)) > 0.2).float()
    return src, tgt, flow, mask


CASES = [
    # (B, H, W, flow scale, mask kind, pad)
    (1, 3, 5, 1.0, "rand", "border"),     # one interior row
    (2, 4, 70, 2.0, "rand", "border"),    # two strips, the strip-row minimum
    (2, 5, 60, 2.0, "ones", "border"),    # exactly one strip
    (2, 9, 61, 2.0, "rand", "zeros"),     # one column into a second strip
    (2, 17, 29, 6.0, "rand", "border"),   # flow piling on the border clip
    (2, 33, 47, 3.0, "rand", "zeros"),
    (2, 24, 40, 2.0, "zero", "border"),   # loss 0 and gradient exactly 0
    (8, 32, 104, 4.0, "rand", "border"),  # the smallest production scale
]


@pytest.mark.parametrize("B,H,W,scale,mkind,pad", CASES)
def test_ternary_loss_matches_reference_composition(hip_device, B, H, W, scale, mkind, pad):
    from unsamflow_amd.census import ternary_loss

    src, tgt, flow, mask = _inputs(B, H, W, scale, mkind, 100 + H + W)
    l64, g32, g64 = _ref_both(lambda f, dt: _ref_term(f[:, :2], src.to(dt), tgt.to(dt), mask.to(dt), pad), flow)

    d = hip_device
    fd = flow.to(d).requires_grad_(True)
    out = ternary_loss(fd[:, :2], src.to(d), tgt.to(d), mask.to(d), pad, 1.0)
    out.backward()
    g = fd.grad.cpu().numpy()
    print(f"[census] {(B, H, W, pad, mkind)}: loss gpu={float(out):.9g} fp64={l64:.9g}")
    assert float(fd.grad[:, 2:].abs().max()) == 0.0  # the untouched flow half
    if mkind == "zero":
        assert float(out) == 0.0 and l64 == 0.0
        assert float(fd.grad.abs().max()) == 0.0 and float(np.abs(g64).max()) == 0.0
        return
    np.testing.assert_allclose(float(out), l64, rtol=2e-5, atol=0)
    _check_grad(f"single {(B, H, W, pad)}", g, g32, g64)


PAIR_CASES = [(2, 24, 40, 2.0, "border"), (1, 3, 5, 1.0, "border"), (2, 9, 61, 2.0, "zeros")]


def _pair_inputs(B, H, W, scale, seed):
    im1 = torch.from_numpy(hashrng.uniform((B, 3, H, W), seed))
    im2 = torch.from_numpy(hashrng.uniform((B, 3, H, W), seed + 1))
    flow = torch.from_numpy(hashrng.symmetric((B, 4, H, W), seed + 2, scale))
    m1 = (torch.from_numpy(hashrng.uniform((B, 1, H, W), seed + 3)) > 0.2).float()
    m2 = (torch.from_numpy(hashrng.uniform((B, 1, H, W), seed + 4)) > 0.3).float()
    return im1, im2, flow, m1, m2


@pytest.mark.parametrize("B,H,W,scale,pad", PAIR_CASES)
def test_ternary_pair_matches_single_directions_and_reference(hip_device, B, H, W, scale, pad):
    """Both with_bk directions in one launch == the two single-direction calls
    bit for bit, and == the reference composition of each direction."""
    from unsamflow_amd.census import ternary_loss, ternary_loss_pair

    im1, im2, flow, m1, m2 = _pair_inputs(B, H, W, scale, 300 + H + W)
    d = hip_device
    fp = flow.to(d).requires_grad_(True)
    lp = ternary_loss_pair(fp, im1.to(d), im2.to(d), m1.to(d), m2.to(d), pad, 1.0)
    (lp[0] * 0.7 + lp[1] * 1.3).backward()

    fs = flow.to(d).requires_grad_(True)
    l0 = ternary_loss(fs[:, :2], im2.to(d), im1.to(d), m1.to(d), pad, 1.0)
    l1 = ternary_loss(fs[:, 2:], im1.to(d), im2.to(d), m2.to(d), pad, 1.0)
    (l0 * 0.7 + l1 * 1.3).backward()
    assert torch.equal(lp.detach().cpu(), torch.stack([l0, l1]).detach().cpu())
    assert torch.equal(fp.grad.cpu(), fs.grad.cpu())

    losses = {}

    def ref(f, dt):
        r0 = _ref_term(f[:, :2], im2.to(dt), im1.to(dt), m1.to(dt), pad)
        r1 = _ref_term(f[:, 2:], im1.to(dt), im2.to(dt), m2.to(dt), pad)
        losses[dt] = [float(r0), float(r1)]
        return r0 * 0.7 + r1 * 1.3

    _, g32, g64 = _ref_both(ref, flow)
    print(f"[census] pair {(B, H, W, pad)}: loss gpu={lp.tolist()} fp64={losses[torch.float64]}")
    np.testing.assert_allclose(lp.detach().cpu().numpy(), losses[torch.float64], rtol=2e-5, atol=0)
    _check_grad(f"pair {(B, H, W, pad)}", fp.grad.cpu().numpy(), g32, g64)


@pytest.mark.parametrize("pad", ["border", "zeros"])
@pytest.mark.parametrize("B,sizes", [(2, [(64, 208), (32, 104), (16, 52), (8, 26)]), (2, [(33, 47), (17, 24)])])
def test_ternary_pyramid_equals_per_scale_pairs(hip_device, B, sizes, pad):
    """ternary_loss_pyramid (one forward and one backward launch for every
    scale) gives the per-scale ternary_loss_pair results bit for bit."""
    from unsamflow_amd.census import ternary_loss_pair, ternary_loss_pyramid

    flows, i1, i2, m1, m2 = [], [], [], [], []
    for k, (H, W) in enumerate(sizes):
        a, b, f, x, y = _pair_inputs(B, H, W, 3.0, 950 + 10 * k)
        for lst, t in zip((i1, i2, flows, m1, m2), (a, b, f, x, y)):
            lst.append(t.to(hip_device))
    fa = [f.clone().requires_grad_(True) for f in flows]
    fb = [f.clone().requires_grad_(True) for f in flows]
    lp = ternary_loss_pyramid(fa, i1, i2, m1, m2, pad)
    ref = torch.stack([ternary_loss_pair(f, a, b, x, y, pad) for f, a, b, x, y in zip(fb, i1, i2, m1, m2)])
    assert lp.shape == (len(sizes), 2) and float(lp.min()) > 0
    assert torch.equal(lp, ref)
    wts = torch.arange(1, 2 * len(sizes) + 1, device=hip_device, dtype=torch.float32).view(-1, 2)
    (lp * wts).sum().backward()
    (ref * wts).sum().backward()
    for a, b in zip(fa, fb):
        assert float(a.grad.abs().max()) > 0
        assert torch.equal(a.grad, b.grad)


def test_ternary_loss_is_deterministic(hip_device):
    from unsamflow_amd.census import ternary_loss_pair

    im1, im2, flow, m1, m2 = (t.to(hip_device) for t in _pair_inputs(2, 33, 130, 3.0, 40))
    res = []
    for _ in range(2):
        f = flow.clone().requires_grad_(True)
        lp = ternary_loss_pair(f, im1, im2, m1, m2, "border")
        lp.sum().backward()
        res.append((lp.detach().clone(), f.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_ternary_forward_only_matches_grad_forward(hip_device):
    """The no-grad instantiation (no basis) computes the same loss value (up to
    FMA contraction choices of the two instantiations)."""
    from unsamflow_amd import ops

    B, H, W = 2, 40, 72
    src, tgt, flow, mask = (t.to(hip_device) for t in _inputs(B, H, W, 3.0, "rand", 7))
    flow = flow[:, :2]
    a, basis = ops.census_loss_forward(src, tgt, mask, flow, "border", need_grad=True)
    b, none = ops.census_loss_forward(src, tgt, mask, flow, "border", need_grad=False)
    assert none is None and basis.shape == (B, 2, H, W)
    assert float(a[0]) > 0
    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-6, atol=0)


@pytest.fixture(scope="module")
def stage1_setup(hip_device):
    """Images, five pyramid flows and the GPU's own occlusion masks (B=2, top 64x208)."""
    from unsamflow_amd import warp_utils

    B, H, W = 2, 64, 208
    img1 = torch.from_numpy(hashrng.uniform((B, 3, H, W), 11))
    img2 = torch.from_numpy(hashrng.uniform((B, 3, H, W), 12))
    flows = [torch.from_numpy(hashrng.symmetric((B, 4, H >> i, W >> i), 20 + i, 3.0 / (1 << i))) for i in range(5)]
    top = flows[0].to(hip_device)
    # the thresholded masks carry no gradient; the fp64 run takes the device's, so a
    # pixel on the threshold cannot differ between the runs
    occ = [warp_utils.get_occu_mask_bidirection(top[:, :2], top[:, 2:]).cpu().double(),
           warp_utils.get_occu_mask_bidirection(top[:, 2:], top[:, :2]).cpu().double()]
    return img1, img2, flows, occ


@pytest.mark.parametrize("weights", [(0.0, 0.0, 1.0), (0.15, 0.85, 0.5)])
def test_stage1_unflowloss_fused_matches_torch_path(hip_device, stage1_setup, weights):
    """unFlowLoss(kitti_stage1().loss) with the fused census op == the library
    warp + torch census composition (fused_photometric=False), value and
    per-level flow gradients (bounded through a CPU fp64 run), with the census
    term alone and with mixed weights."""
    from unsamflow_amd.config import kitti_stage1
    from unsamflow_amd.flow_loss import unFlowLoss

    img1, img2, flows, occ = stage1_setup
    cfg = kitti_stage1().loss
    cfg.w_l1, cfg.w_ssim, cfg.w_ternary = weights
    d = hip_device
    res = []
    for fused in (True, False):
        fl = [f.to(d).requires_grad_(True) for f in flows]
        loss = unFlowLoss(cfg, fused_photometric=fused)(fl, img1.to(d), img2.to(d))[0].sum()
        loss.backward()
        res.append((float(loss), [None if f.grad is None else f.grad.cpu().numpy() for f in fl]))
    (lf, gf), (lt, gt) = res

    it = iter(occ)
    f64 = [f.double().requires_grad_(True) for f in flows]
    l64 = unFlowLoss(cfg, warp_fn=oracle_flow_warp, occ_bidir_fn=lambda a, b: next(it))(
        f64, img1.double(), img2.double())[0].sum()
    l64.backward()
    print(f"[census] unFlowLoss {weights}: fused={lf:.9g} torch={lt:.9g} fp64={float(l64):.9g}")
    np.testing.assert_allclose(lf, lt, rtol=2e-5)
    np.testing.assert_allclose(lf, float(l64), rtol=2e-5)
    for i, (a, b, c) in enumerate(zip(gf, gt, f64)):  # the 5th level has photometric weight 0 (no gradient at all)
        assert (a is None) == (b is None) == (c.grad is None)
        if a is not None:
            _check_grad(f"unFlowLoss {weights} level {i}", a, b.astype(np.float64), c.grad.numpy())
    assert gf[4] is None and gf[0] is not None


def test_stage1_unflowloss_launches_the_census_pyramid(hip_device, stage1_setup, monkeypatch):
    """With the census term alone the fused path is the census pyramid op (no L1/SSIM launch)."""
    from unsamflow_amd import kernel_timer
    from unsamflow_amd.config import kitti_stage1
    from unsamflow_amd.flow_loss import unFlowLoss

    img1, img2, flows, _ = stage1_setup
    d = hip_device
    seen = []
    orig = kernel_timer.timed

    def spy(op, *a, **k):
        seen.append(op)
        return orig(op, *a, **k)

    monkeypatch.setattr(kernel_timer, "timed", spy)
    fl = [f.to(d).requires_grad_(True) for f in flows]
    unFlowLoss(kitti_stage1().loss)(fl, img1.to(d), img2.to(d))[0].sum().backward()
    assert "census_pyr_grad" in seen and "census_pyr_bwd" in seen
    assert not [s for s in seen if s.startswith("photo_")]


def test_ternary_pair_graph_replay(hip_device):
    """One single-stream capture of a pair forward + backward, after an eager
    warm-up, replayed twice: bit-identical to eager."""
    from unsamflow_amd import ops

    im1, im2, flow, m1, m2 = (t.to(hip_device) for t in _pair_inputs(2, 33, 130, 3.0, 60))
    gl = torch.tensor([0.7, 1.3], device=hip_device)

    def fn():
        out, basis = ops.census_loss_pair_forward(flow, im1, im2, m1, m2, "border", 1.0, need_grad=True)
        return out, ops.census_loss_backward(basis, out, gl)

    ref = [t.clone() for t in fn()]
    torch.cuda.synchronize()
    assert float(ref[1].abs().max()) > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, ref):
            assert torch.equal(a, b)
    del graph
