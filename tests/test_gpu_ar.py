"""The fused stage-1 augmentation branch (unsamflow_amd.ar, csrc/ar.hip) on the
GPU against the torch composition of the same formulas evaluated on the CPU in
fp32 and again in fp64 on the same inputs.

Transform: the bound comes from the reference inside the test, per tensor:
    e_ref = max|cpu_fp32 - fp64|,   max|gpu - fp64| <= 4 e_ref
(the factor 4 covers another rounding of the same fp32 quantities). Only pixels
whose fp64 source coordinate lies within 1e-3 px of a validity edge (x = 0, W or
y = 0, H) may be excluded -- there a rounding error zeroes or keeps a pixel --
and the thetas are chosen so that none is (asserted).

AR loss: the value against fp64 at rtol 2e-5 (the project's figure for fused
loss values); the gradient max|g_gpu - g64| <= max(4 e_ref, 2e-4 max|g64|) with
e_ref = max|g_cpu_fp32 - g64|, as tests/test_gpu_census.py.

Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest
import torch

import ar_util
from oracle import hashrng

pytestmark = pytest.mark.gpu

TENSORS = ["img1_t", "img2_t", "flow_t", "mask_t"]
SHAPES = [(1, 2, 3), (2, 13, 21), (3, 33, 70), (2, 64, 96)]


@pytest.fixture(scope="module")
def transform_refs():
    """Per shape: inputs, thetas and the CPU fp32 / fp64 compositions (computed once, never modified)."""
    from unsamflow_amd import ar

    refs = {}
    for B, H, W in SHAPES:
        inp = ar_util.inputs(B, H, W, 400 + H + W)
        th = ar_util.clear_thetas(B, H, W)
        o32 = ar.spatial_transform(*inp, th)
        o64 = ar.spatial_transform(*[t.double() for t in inp], th)
        refs[(B, H, W)] = (inp, th, o32, o64)
    return refs


def _check_transform(name, outs, o32, o64, keep1, keep2):
    for k, g, a, b in zip(TENSORS, outs, o32, o64):
        keep = (keep2 if k == "img2_t" else keep1)[:, None].expand_as(b)
        e_ref = float((a.double() - b)[keep].abs().max())
        err = float((g.cpu().double() - b)[keep].abs().max())
        print(f"[ar] {name} {k}: err={err:.3e} e_ref={e_ref:.3e} max|ref|={float(b.abs().max()):.3e}")
        assert tuple(g.shape) == tuple(b.shape)
        assert err <= 4.0 * e_ref, (name, k, err, e_ref)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_transform_matches_fp64_composition(hip_device, transform_refs, B, H, W):
    from unsamflow_amd import ar

    inp, th, o32, o64 = transform_refs[(B, H, W)]
    keep = [torch.from_numpy(ar_util.edge_distance(th[k], H, W) >= 1e-3) for k in range(2)]
    for k in range(2):
        excluded = 1.0 - float(keep[k].double().mean())
        assert excluded <= 0.01 and excluded == 0.0, (k, excluded)  # the CPU composition excludes none
    if B > 1:  # per-sample different thetas, sample 1 mirrored, part of sample 0 outside its source
        assert th[0, 1, 0] < 0 < th[0, 0, 0] and ar_util.zeroed_fraction(th[0], H, W)[0] > 0.1
    outs = ar.spatial_transform(*[t.to(hip_device) for t in inp], th)
    assert all(o.is_cuda and o.is_contiguous() for o in outs)
    _check_transform(f"{(B, H, W)}", outs, o32, o64, keep[0], keep[1])
    # the zeroed pixels are the composition's
    assert torch.equal(outs[0].cpu() == 0, o32[0] == 0) and torch.equal(outs[3].cpu() == 0, o32[3] == 0)


def test_transform_takes_a_flow_channel_slice_in_place(hip_device, transform_refs):
    """flows_12[0] of the harness is a channel slice of the [B,4,H,W] flow: batch stride 4*H*W, no copy."""
    from unsamflow_amd import ar

    inp, th, o32, o64 = transform_refs[(2, 13, 21)]
    img1, img2, flow, mask = (t.to(hip_device) for t in inp)
    flow4 = torch.cat([flow, flow + 100.0], 1)
    a = ar.spatial_transform(img1, img2, flow, mask, th)
    b = ar.spatial_transform(img1, img2, flow4[:, :2], mask, th)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_identity_thetas_on_the_gpu(hip_device):
    from unsamflow_amd import ar

    B, H, W = 2, 12, 20
    inp = ar_util.inputs(B, H, W, 9330, lo=0.1)
    th = ar_util.identity_thetas(B)
    o32 = ar.spatial_transform(*inp, th)
    o64 = ar.spatial_transform(*[t.double() for t in inp], th)
    outs = ar.spatial_transform(*[t.to(hip_device) for t in inp], th)
    all_px = torch.ones(B, H, W, dtype=torch.bool)
    _check_transform("identity", outs, o32, o64, all_px, all_px)  # no exclusion
    assert float(outs[0].min()) > 0.09 and float(outs[1].min()) > 0.09  # no pixel zeroed
    assert float((outs[0].cpu() - inp[0]).abs().max()) <= 2e-6


def test_noise_is_added_and_clamped_in_the_kernel(hip_device, transform_refs):
    inp, th, _, _ = transform_refs[(3, 33, 70)]
    from unsamflow_amd import ar

    B, H, W = 3, 33, 70
    d = hip_device
    n1 = (torch.from_numpy(hashrng.normal((B, 3, H, W), 77)) * 0.5).to(d)
    n2 = (torch.from_numpy(hashrng.normal((B, 3, H, W), 78)) * 0.5).to(d)
    dev_in = [t.to(d) for t in inp]
    base = ar.spatial_transform(*dev_in, th)
    out = ar.spatial_transform(*dev_in, th, n1, n2)
    only1 = ar.spatial_transform(*dev_in, th, n1, None)
    for o, b, n in ((out[0], base[0], n1), (out[1], base[1], n2)):
        want = (b + n).clamp(0.0, 1.0)
        assert float(o.min()) >= 0.0 and float(o.max()) <= 1.0
        assert float(o.min()) == 0.0 and float(o.max()) == 1.0  # the clamp is exercised at both ends
        # within 1 ulp: one fp32 addition, then the clamp
        ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126, device=d)) * 2.0 ** -23
        assert bool(((o - want).abs() <= ulp).all())
    assert torch.equal(out[2], base[2]) and torch.equal(out[3], base[3])
    assert torch.equal(only1[0], out[0]) and torch.equal(only1[1], base[1])


# ----------------------------------------------------------------- AR loss --
def _loss_inputs(B, H, W, seed):
    pred = torch.from_numpy(hashrng.normal((B, 2, H, W), seed)) * 3.0
    target = torch.from_numpy(hashrng.normal((B, 2, H, W), seed + 1)) * 3.0
    noc = (torch.from_numpy(hashrng.uniform((B, 1, H, W), seed + 2)) > 0.4).float()
    return pred, target, noc


def _cpu_refs(pred, target, noc, eps, q, denom):
    """(loss_fp64, grad_fp32, grad_fp64) of the torch composition on the CPU."""
    from unsamflow_amd import ar

    out = []
    for dt in (torch.float32, torch.float64):
        p = pred.detach().to(dt).requires_grad_(True)
        loss = ar.ar_loss_torch(p, target.to(dt), noc.to(dt), eps, q, None if denom is None else denom.to(dt))
        loss.backward()
        out.append((float(loss.detach()), p.grad.double().numpy()))
    return out[1][0], out[0][1], out[1][1]


def _check_loss(name, loss, grad, l64, g32, g64):
    e_ref = float(np.abs(g32 - g64).max())
    gmax = float(np.abs(g64).max())
    err = float(np.abs(grad.cpu().double().numpy() - g64).max())
    bound = max(4.0 * e_ref, 2e-4 * gmax)
    print(f"[ar] {name}: loss gpu={float(loss):.9g} fp64={l64:.9g} grad err={err:.3e} e_ref={e_ref:.3e} "
          f"max|g|={gmax:.3e} bound={bound:.3e}")
    np.testing.assert_allclose(float(loss), l64, rtol=2e-5, atol=0)
    assert err <= bound, (name, err, e_ref, gmax)


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("eps,q", [(0.0, 1.0), (0.01, 0.4)])
@pytest.mark.parametrize("with_denom", [False, True])
def test_ar_loss_matches_fp64(hip_device, B, H, W, eps, q, with_denom):
    from unsamflow_amd import ar

    pred, target, noc = _loss_inputs(B, H, W, 500 + H + W)
    if H >= 13:  # a block of exact agreement: sign(0) = 0
        target[:, :, 2:7, 3:11] = pred[:, :, 2:7, 3:11]
    denom = torch.tensor([0.37]) if with_denom else None
    l64, g32, g64 = _cpu_refs(pred, target, noc, eps, q, denom)
    d = hip_device
    p = pred.to(d).requires_grad_(True)
    loss = ar.ar_loss(p, target.to(d), noc.to(d), eps, q, None if denom is None else denom.to(d))
    loss.backward()
    _check_loss(f"{(B, H, W)} q={q} eps={eps} denom={with_denom}", loss.detach(), p.grad, l64, g32, g64)
    if H >= 13:
        assert float(p.grad[:, :, 2:7, 3:11].abs().max()) == 0.0
        assert float(p.grad.abs().max()) > 0.0


@pytest.mark.parametrize("eps,q", [(0.0, 1.0), (0.01, 0.4)])
def test_ar_loss_reads_a_crop_view_in_place(hip_device, eps, q):
    """The third pass: target and mask are 32x64 windows of 64x96 tensors at a
    non-zero offset, read through their strides (no copy)."""
    from unsamflow_amd import ar, ops

    B, H, W, y1, x1, ch, cw = 2, 64, 96, 5, 17, 32, 64
    _, target, noc = _loss_inputs(B, H, W, 700)
    pred = torch.from_numpy(hashrng.normal((B, 2, ch, cw), 703)) * 3.0
    win = (slice(None), slice(None), slice(y1, y1 + ch), slice(x1, x1 + cw))
    l64, g32, g64 = _cpu_refs(pred, target[win], noc[win], eps, q, None)
    d = hip_device
    td, nd = target.to(d), noc.to(d)
    seen = []
    orig = ops.ar_loss_forward

    def spy(pred_, target_, noc_, *a, **k):
        seen.append((target_.data_ptr(), target_.stride(), noc_.data_ptr(), noc_.stride()))
        return orig(pred_, target_, noc_, *a, **k)

    ops.ar_loss_forward = spy
    try:
        p = pred.to(d).requires_grad_(True)
        loss = ar.ar_loss(p, td[win], nd[win], eps, q)
    finally:
        ops.ar_loss_forward = orig
    loss.backward()
    assert seen == [(td[win].data_ptr(), (2 * H * W, H * W, W, 1), nd[win].data_ptr(), (H * W, H * W, W, 1))]
    _check_loss(f"crop q={q}", loss.detach(), p.grad, l64, g32, g64)
    # the same numbers as from a contiguous copy of the window
    p2 = pred.to(d).requires_grad_(True)
    loss2 = ar.ar_loss(p2, td[win].contiguous(), nd[win].contiguous(), eps, q)
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(p2.grad, p.grad)


def test_ar_loss_is_deterministic_and_refuses_target_gradients(hip_device):
    from unsamflow_amd import ar

    pred, target, noc = (t.to(hip_device) for t in _loss_inputs(3, 33, 70, 800))
    res = []
    for _ in range(2):
        p = pred.clone().requires_grad_(True)
        loss = ar.ar_loss(p, target, noc, 0.01, 0.4)
        loss.backward()
        res.append((loss.detach().clone(), p.grad.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    with pytest.raises(NotImplementedError):
        ar.ar_loss(pred, target.clone().requires_grad_(True), noc)
    with pytest.raises(NotImplementedError):
        ar.ar_loss(pred, target, noc.clone().requires_grad_(True))


def test_transform_and_loss_graph_replay(hip_device, transform_refs):
    """Transform + loss forward + backward captured once after an eager warm-up,
    replayed on new contents of the static inputs: equal to eager."""
    from unsamflow_amd import ops

    d = hip_device
    B, H, W = 2, 64, 96
    inp, th, _, _ = transform_refs[(B, H, W)]
    static = [t.to(d) for t in inp] + [th.to(d)]
    pred = (torch.from_numpy(hashrng.normal((B, 2, H, W), 900)) * 3.0).to(d)
    gl = torch.tensor([0.7], device=d)

    def fn():
        i1, i2, fl, mk = ops.ar_transform(*static)
        out = ops.ar_loss_forward(pred, fl, mk, 0.0, 1.0)
        return i1, i2, fl, mk, out, ops.ar_loss_backward(pred, fl, mk, out, gl, 0.0, 1.0)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    new = ar_util.inputs(B, H, W, 950)
    for k in range(2):
        if k == 1:  # new contents of the static inputs, another theta
            for dst, src in zip(static, list(new) + [ar_util.clear_thetas(B, H, W).flip(1)]):
                dst.copy_(src)
            pred.mul_(-0.5)
        graph.replay()
        torch.cuda.synchronize()
        ref = [t.clone() for t in fn()]
        torch.cuda.synchronize()
        assert float(ref[5].abs().max()) > 0
        for a, b in zip(out, ref):
            assert torch.equal(a, b)
    del graph


# -------------------------------------------------------------------- step --
@pytest.fixture(scope="module")
def ar_step_cfg():
    from unsamflow_amd.config import kitti_stage1_ar

    cfg = kitti_stage1_ar()
    cfg.train.ot_size = [64, 128]
    return cfg


def _scaled_step(cfg, device, **kw):
    """A freshly initialised PWCLite answers noise frames with flows the
    bidirectional check calls occluded everywhere; small weights give small
    flows, a mask of ones and terms that measure something."""
    from unsamflow_amd.harness import TrainStep

    step = TrainStep(cfg, device, **kw)
    with torch.no_grad():
        for p in step.module.parameters():
            p.mul_(0.02)
    return step


def test_fused_step_matches_the_torch_composition(hip_device, ar_step_cfg, monkeypatch):
    """TrainStep(kitti_stage1_ar()) at B=2, 128x192 from one seed, fused against
    fused_ar=False: loss, l_atst and l_ot at rtol 1e-4; one transform launch and
    two AR loss forwards per step."""
    from unsamflow_amd import ops
    from unsamflow_amd.harness import synthetic_pair

    img1, img2, _, _ = synthetic_pair(2, 128, 192, hip_device)
    counts = {"ar_transform": 0, "ar_loss_forward": 0, "ar_loss_backward": 0}
    for name in counts:
        orig = getattr(ops, name)

        def spy(*a, _n=name, _f=orig, **k):
            counts[_n] += 1
            return _f(*a, **k)

        monkeypatch.setattr(ops, name, spy)
    res = {}
    for fused in (True, False):
        step = _scaled_step(ar_step_cfg, hip_device, fused_ar=fused)
        for k in counts:
            counts[k] = 0
        loss = step(img1, img2)
        res[fused] = (float(loss), float(step.l_atst), float(step.l_ot), dict(counts))
    print(f"[ar] step fused={res[True][:3]} torch={res[False][:3]} rel diff="
          f"{[abs(a - b) / abs(b) for a, b in zip(res[True][:3], res[False][:3])]}")
    assert res[True][3] == {"ar_transform": 1, "ar_loss_forward": 2, "ar_loss_backward": 2}
    assert res[False][3] == {"ar_transform": 0, "ar_loss_forward": 0, "ar_loss_backward": 0}
    for a, b in zip(res[True][:3], res[False][:3]):
        assert b > 0 and np.isfinite(a)
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=0)


def test_graphed_step_refuses_the_ar_branch(hip_device, ar_step_cfg):
    from unsamflow_amd.harness import GraphedTrainStep, TrainStep, synthetic_pair

    img1, img2, _, _ = synthetic_pair(1, 64, 128, hip_device)
    step = TrainStep(ar_step_cfg, hip_device, capturable=True)
    with pytest.raises(NotImplementedError):
        GraphedTrainStep(step, img1, img2)
