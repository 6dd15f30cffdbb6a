"""The per-segment max pool and spread kernels (csrc/segpool.hip) on the GPU
against ``segment_max_spread_torch`` on the CPU in fp32 and fp64.

Forward: comparisons and copies only, so ``spread`` equals the CPU fp32
composition exactly (torch.equal: a zero's sign is not part of the contract).
Backward: max|g_gpu - g64| <= max(4 e_ref, 2e-4 max|g64|) with e_ref =
max|g_cpu_fp32 - g64|, as tests/test_gpu_ar.py and test_gpu_census.py; and
grad_proj is 0 exactly where the fp64 gradient is. fp32 values cast to fp64 keep
their equalities, so both references see the same ties. No element is excluded.

Model level: sintel_mf at 1x128x256 with the pooling switch and the shared
mask-feature switch on against off."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import segpool_util as su

pytestmark = pytest.mark.gpu

# (B, C, h, w, K): the smallest shapes at which each mechanism can go wrong
ONE_PIXEL = (1, 1, 1, 1, 1)       # a negative value; the segment covers the sample: no clamp at 0
WHOLE = (2, 3, 5, 7, 4)           # sample 0: one id, all values negative; sample 1 mixed
L0 = (2, 32, 7, 16, 32)           # Sintel L0
WIDE = (2, 5, 9, 70, 300)         # rows longer than a wave, not a multiple of 4; K > 256; most ids absent
NOISE = (1, 8, 28, 64, 64)        # an independent id per pixel: 64 runs per wave step
L4 = (1, 32, 112, 256, 40)        # one full L4 sample, 8-pixel blocks: the multi-workgroup merge
MAXK = (1, 2, 4, 8, 1024)         # K at the limit
SHAPES = [ONE_PIXEL, WHOLE, L0, WIDE, NOISE, L4, MAXK]


def _segments(shape, gen):
    B, C, h, w, K = shape
    if shape == ONE_PIXEL:
        return torch.zeros(1, 1, 1, 1)
    if shape == WHOLE:
        seg = su.block_segments(B, h, w, K, 2, gen)
        seg[0] = 2.0
        return seg
    if shape == WIDE:
        return su.block_segments(B, h, w, K, 3, gen, ids=[3, 17, 150, 299])
    if shape == NOISE:
        return su.block_segments(B, h, w, K, 1, gen)
    if shape == L4:
        return su.block_segments(B, h, w, K, 8, gen)
    if shape == MAXK:
        return su.block_segments(B, h, w, K, 2, gen, ids=[0, 511, 1023])
    return su.block_segments(B, h, w, K, 2, gen)


def _inputs(shape, quantised):
    B, C, h, w, K = shape
    gen = torch.Generator().manual_seed(1000 + 2 * SHAPES.index(shape) + quantised)
    seg = _segments(shape, gen)
    proj = su.values((B, C, h, w), gen, quantised)
    if shape in (ONE_PIXEL, WHOLE):
        proj[0] = -proj[0].abs() - 0.25
    if quantised and shape != ONE_PIXEL:
        su.force_negative_segment(proj, seg, B - 1, 0)
    gs = torch.randn((B, C, h, w), generator=gen)
    return proj, seg, gs


def _composition(proj, seg, gs, K, dtype):
    from unsamflow_amd.segpool import segment_max_spread_torch

    p = proj.to(dtype).requires_grad_(True)
    out = segment_max_spread_torch(p, seg, K)
    (g,) = torch.autograd.grad(out, p, gs.to(dtype))
    return out.detach(), g


_REFS = {}


def _reference(shape, quantised):
    """(inputs, spread32, g32, g64) on the CPU, computed once per case."""
    key = (shape, quantised)
    if key not in _REFS:
        proj, seg, gs = _inputs(shape, quantised)
        out32, g32 = _composition(proj, seg, gs, shape[4], torch.float32)
        out64, g64 = _composition(proj, seg, gs, shape[4], torch.float64)
        assert torch.equal(out32.double(), out64)
        _REFS[key] = ((proj, seg, gs), out32, g32, g64)
    return _REFS[key]


def _gpu(proj, seg, gs, K, d):
    from unsamflow_amd.segpool import segment_max_spread

    p = proj.to(d).requires_grad_(True)
    out = segment_max_spread(p, seg.to(d), K)
    (g,) = torch.autograd.grad(out, p, gs.to(d))
    torch.cuda.synchronize(d)
    return out.detach().cpu(), g.cpu()


def _check_gradient(tag, g, g32, g64):
    e_ref = float((g32.double() - g64).abs().max())
    gmax = float(g64.abs().max())
    err = float((g.double() - g64).abs().max())
    bound = max(4.0 * e_ref, 2e-4 * gmax)
    print(f"[segpool] {tag}: grad err={err:.3e} e_ref={e_ref:.3e} max|g64|={gmax:.3e} bound={bound:.3e}")
    assert err <= bound, (tag, err, e_ref, gmax)
    assert torch.equal(g == 0, g64 == 0), tag


@pytest.mark.parametrize("quantised", [False, True], ids=["randn", "quantised"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_exact_and_gradient_within_bound(hip_device, shape, quantised):
    from unsamflow_amd import ops

    (proj, seg, gs), out32, g32, g64 = _reference(shape, quantised)
    if quantised and shape != ONE_PIXEL:  # ties, exact zeros and an all-negative partial segment all occur
        assert su.input_features(proj, seg, shape[4]) == (True, True, True)
    if shape == WIDE:
        assert 299.0 in seg and len(torch.unique(seg)) <= 4
    if shape in (ONE_PIXEL, WHOLE):
        assert (out32[0] < 0).all()  # no clamp at 0 where one id covers the sample
    out, g = _gpu(proj, seg, gs, shape[4], hip_device)
    assert ops.device_errors(hip_device) == 0
    assert torch.equal(out, out32)
    _check_gradient(f"{shape} quantised={quantised}", g, g32, g64)


@pytest.mark.parametrize("shape", [L4, NOISE], ids=["L4", "noise"])
def test_two_calls_agree_bit_for_bit(hip_device, shape):
    proj, seg, gs = _inputs(shape, True)
    a = _gpu(proj, seg, gs, shape[4], hip_device)
    b = _gpu(proj, seg, gs, shape[4], hip_device)
    assert a[0].view(torch.int32).equal(b[0].view(torch.int32))
    assert a[1].view(torch.int32).equal(b[1].view(torch.int32))
    assert float(a[1].abs().max()) > 0


def test_other_layouts_and_integer_ids(hip_device):
    """channels_last activations (TrainStep(channels_last=True)) and int64 ids:
    made dense NCHW fp32 in the wrapper, same result."""
    from unsamflow_amd.segpool import segment_max_spread

    (proj, seg, gs), out32, _, _ = _reference(L0, False)
    d = hip_device
    p = proj.to(d).contiguous(memory_format=torch.channels_last)
    assert not p.is_contiguous()
    assert torch.equal(segment_max_spread(p, seg.to(d).long(), L0[4]).cpu(), out32)
    assert torch.equal(segment_max_spread(p, seg.to(d)).cpu(), out32)  # K read back from the ids


def test_bad_ids_are_flagged_and_ignored(hip_device):
    """id = K, id = -1 and id = 2.5: spread 0 and no gradient there, the rest as if
    those pixels belonged to no segment, USF_DEVERR_SEGPOOL_BAD_ID raised and cleared."""
    from unsamflow_amd import _lib, ops

    B, C, h, w, K = 2, 3, 6, 10, 5
    gen = torch.Generator().manual_seed(77)
    seg = su.block_segments(B, h, w, K, 2, gen)
    proj = su.values((B, C, h, w), gen, True)
    gs = torch.randn((B, C, h, w), generator=gen)
    bad = torch.zeros(B, 1, h, w, dtype=torch.bool)
    for (b, y, x), v in {(0, 1, 3): float(K), (1, 0, 0): -1.0, (1, 5, 9): 2.5}.items():
        seg[b, 0, y, x] = v
        bad[b, 0, y, x] = True

    def reference(dtype):
        p = proj.to(dtype).requires_grad_(True)
        onehot = F.one_hot(torch.where(bad, torch.zeros_like(seg), seg).long(), K) * (~bad)[..., None]
        pooled = torch.amax(onehot * p[..., None], dim=(2, 3))
        out = (onehot * pooled[:, :, None, None, :]).sum(dim=-1)
        (g,) = torch.autograd.grad(out, p, gs.to(dtype))
        return out.detach(), g

    out32, g32 = reference(torch.float32)
    _, g64 = reference(torch.float64)
    assert ops.device_errors(hip_device) == 0
    out, g = _gpu(proj, seg, gs, K, hip_device)  # returns normally
    assert torch.equal(out, out32)
    everywhere = bad.expand(B, C, h, w)
    assert (out[everywhere] == 0).all() and (g[everywhere] == 0).all()
    _check_gradient("bad ids", g, g32, g64)
    assert ops.device_errors(hip_device, clear=False) == _lib.DEVERR_SEGPOOL_BAD_ID
    assert ops.device_errors(hip_device) == _lib.DEVERR_SEGPOOL_BAD_ID
    assert ops.device_errors(hip_device) == 0  # cleared


def test_memory_is_independent_of_k(hip_device):
    """Forward + backward at (2,32,28,64,64) allocate at most 4 x proj beyond the
    inputs and grad_spread (spread, grad_proj, the tables); the composition's
    [B,C,h,w,K] products alone are 64 x."""
    from unsamflow_amd.segpool import segment_max_spread

    d = hip_device
    B, C, h, w, K = 2, 32, 28, 64, 64
    gen = torch.Generator().manual_seed(3)
    seg = su.block_segments(B, h, w, K, 4, gen).to(d)
    proj = torch.randn((B, C, h, w), generator=gen).to(d).requires_grad_(True)
    gs = torch.randn((B, C, h, w), generator=gen).to(d)
    torch.cuda.synchronize(d)
    torch.cuda.reset_peak_memory_stats(d)
    base = torch.cuda.memory_allocated(d)
    out = segment_max_spread(proj, seg, K)
    out.backward(gs)
    torch.cuda.synchronize(d)
    extra = torch.cuda.max_memory_allocated(d) - base
    nbytes = proj.numel() * 4
    print(f"[segpool] memory: extra={extra} B = {extra / nbytes:.2f} x proj")
    assert extra <= 4 * nbytes + (1 << 20), (extra, nbytes)
    assert float(proj.grad.abs().max()) > 0


def test_graph_replay(hip_device):
    """Forward + backward with num_segments given, captured once after an eager
    warm-up and replayed on new contents of the same buffers: equal to eager."""
    from unsamflow_amd import ops
    from unsamflow_amd.segpool import segment_max_spread

    d = hip_device
    shape = (2, 8, 12, 20, 9)
    B, C, h, w, K = shape
    gen = torch.Generator().manual_seed(41)
    static = [su.values((B, C, h, w), gen, True).to(d), su.block_segments(B, h, w, K, 3, gen).to(d),
              torch.randn((B, C, h, w), generator=gen).to(d)]

    def fn():
        proj, seg, gs = static
        spread, state = ops.segpool_forward(proj, seg, K)
        with torch.no_grad():
            public = segment_max_spread(proj, seg, K)  # no host sync with K given
        return spread, public, ops.segpool_backward(proj, seg, state, gs, K)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    for k in range(2):
        new = [su.values((B, C, h, w), gen, k == 1), su.block_segments(B, h, w, K, 2 + k, gen),
               torch.randn((B, C, h, w), generator=gen)]
        for dst, src in zip(static, new):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        ref = [t.clone() for t in fn()]
        torch.cuda.synchronize()
        assert float(ref[2].abs().max()) > 0
        for a, b in zip(out, ref):
            assert a.view(torch.int32).equal(b.view(torch.int32))
        want, _ = _composition(new[0], new[1], new[2], K, torch.float32)
        assert torch.equal(out[0].cpu(), want) and torch.equal(out[1].cpu(), want)
    del graph


# ------------------------------------------------------------------- model --
@pytest.fixture(scope="module")
def model_runs(hip_device):
    """sintel_mf at 1x128x256: flows and parameter gradients of one forward_loss +
    backward under (pooling switch, shared mask-feature switch)."""
    from oracle.hashrng import hash_init_
    from unsamflow_amd import pwclite
    from unsamflow_amd.config import sintel_mf
    from unsamflow_amd.harness import TrainStep, synthetic_pair

    d = hip_device
    img1, img2, s1, s2 = synthetic_pair(1, 128, 256, d, seed=61, with_seg=True)
    saved = pwclite.FUSED_SEG_POOL, pwclite.SHARED_MASK_FEATURE
    runs = {}

    def run(pool, shared):
        pwclite.FUSED_SEG_POOL, pwclite.SHARED_MASK_FEATURE = pool, shared
        step = TrainStep(sintel_mf(), d)
        hash_init_(step.module, seed=3)
        loss, flows = step.forward_loss(img1, img2, s1, s2)
        loss.backward()
        torch.cuda.synchronize(d)
        return ([f.detach().cpu() for f in flows],
                {n: p.grad.double().cpu() for n, p in step.module.named_parameters()})

    # the convolution library's default solvers are not reproducible from call to
    # call (the feature pyramid alone differs in its last bits between two passes);
    # its deterministic ones are, and only then can two runs be compared bit for bit
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for pool, shared in ((False, False), (True, False), (True, True)):
            runs[(pool, shared)] = run(pool, shared)
        again = run(False, False)[0]
        assert all(torch.equal(a, b) for a, b in zip(again, runs[(False, False)][0])), \
            "the composition run does not reproduce itself"
    finally:
        pwclite.FUSED_SEG_POOL, pwclite.SHARED_MASK_FEATURE = saved
        torch.backends.cudnn.deterministic = det
    return runs


def _check_grads(got, want):
    n_mask = 0
    for n, gw in want.items():
        n_mask += "mask" in n
        ga = float(gw.abs().sum())
        assert abs(float(got[n].sum()) - float(gw.sum())) <= 2e-3 * ga + 1e-8, n
        assert abs(float(got[n].abs().sum()) - ga) <= 2e-3 * ga + 1e-8, n
    assert n_mask > 0  # the mask-feature branch's own parameters took part


def test_model_pooling_switch(model_runs):
    """FUSED_SEG_POOL on against off: the five flows bit-identical, gradient sums
    within tests/test_gpu_fullsize.py's bound."""
    (f_off, g_off), (f_on, g_on) = model_runs[(False, False)], model_runs[(True, False)]
    assert len(f_on) == len(f_off) == 5
    print("[segpool] pooling switch: max|flow_on - flow_off| per level =",
          [float((a - b).abs().max()) for a, b in zip(f_on, f_off)])
    for a, b in zip(f_on, f_off):
        assert float(b.abs().max()) > 0
        assert torch.equal(a, b)
    _check_grads(g_on, g_off)


def test_model_shared_mask_feature_switch(model_runs):
    """SHARED_MASK_FEATURE on against off: flows within test_gpu_fullsize.py's
    atol 1e-4 / rtol 1e-3, gradients within its bound."""
    (f_off, g_off), (f_on, g_on) = model_runs[(True, False)], model_runs[(True, True)]
    print("[segpool] shared mask feature: flows bitwise equal =",
          [bool(torch.equal(a, b)) for a, b in zip(f_on, f_off)])
    for a, b in zip(f_on, f_off):
        np.testing.assert_allclose(a.numpy(), b.numpy(), atol=1e-4, rtol=1e-3)
    _check_grads(g_on, g_off)
