"""The conv epilogues on the GPU (csrc/convepi.hip): the in-place bias + LeakyReLU
pass bit-identical to ``add_`` + ``leaky_relu_``, the input gradient bit-identical
to ``leaky_relu_backward``, the bias gradient against the fp64 sum within the
fp32 summation bound of the kernel's own order, deterministic, and conv_block's
autograd wiring eager and under graph capture.

The bias-gradient bound: a lane's 16 accumulators each take at most
USF_CONVEPI_CHAIN = 64 terms in sequence (one per tile; the kernel's chain
length is the issue's 64); everything after is a pairwise tree over P leaves:
a plane edge's up to 4 floats, the 16 accumulators, the 256 lanes of a
workgroup and the parts of a split channel. |err| <= 2 (64 + ceil(log2 P))
2^-24 sum|gin|, the factor 2 over the standard bound.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SLOPE = 0.1


def _consts():
    from unsamflow_amd import _lib

    return _lib.CONVEPI_TILE_SLOTS, _lib.CONVEPI_CHAIN


def _parts(B, C, H, W):
    from unsamflow_amd import _lib

    n = int(_lib.load().usf_convepi_bwd_workspace(B, C, H, W))
    assert n >= 0 and n % C == 0
    return max(1, n // C)


def _split_shape():
    """(3, 5, 3, W) on the split path with a ragged last part, from the kernel's
    constants: H*W = 4 (nsm - 1) + 1 is odd (every plane start misaligned
    differently, the last slot of each plane holds one float) and the channel's
    B * nsm slots are two whole tiles plus one float4 and three floats."""
    tile, _ = _consts()
    B, C, H = 3, 5, 3
    assert (2 * tile + 4) % B == 0
    nsm = (2 * tile + 4) // B
    hw = 4 * (nsm - 1) + 1
    assert hw % H == 0 and (hw + 6) // 4 == nsm
    shape = (B, C, H, hw // H)
    assert _parts(*shape) == 3  # two whole tiles and the ragged third, one part each
    return shape


def _looping_shape():
    """(1, C, 7, W) where a workgroup takes two tiles in sequence: four tiles per
    channel (the last one ragged, H*W odd) and more than USF_CONVEPI_TARGET_WGS
    tiles over all channels, the smallest such shape (270 MB a tensor)."""
    from unsamflow_amd import _lib

    tile, _ = _consts()
    C = _lib.CONVEPI_TARGET_WGS // 3 + 1  # 4 C tiles: above the target, at most twice
    hw = 4 * (3 * tile + 6) + 1  # nsm = 3 tiles + 7 slots
    assert hw % 7 == 0
    shape = (1, C, 7, hw // 7)
    assert _parts(*shape) == 2
    return shape


def _shapes():
    return [((1, 1, 1, 1), SLOPE), ((2, 3, 5, 7), SLOPE), ((16, 192, 4, 13), SLOPE), ((16, 2, 4, 13), 1.0),
            (_split_shape(), SLOPE), ((2, 3, 5, 7), 1.0), (_looping_shape(), SLOPE)]


def _bias_bound(gin, shape):
    _, chain = _consts()
    P = 4 * 16 * 256 * _parts(*shape)
    return 2 * (chain + math.ceil(math.log2(P))) * 2.0 ** -24 * gin.double().abs().sum(dim=(0, 2, 3))


def _check_bias(gbias, gin, shape):
    want = gin.double().sum(dim=(0, 2, 3))
    err = (gbias.double() - want).abs()
    bound = _bias_bound(gin, shape)
    print(f"{shape}: bias-gradient max err {err.max().item():.3e}, bound at that channel "
          f"{bound[err.argmax()].item():.3e}")
    assert (err <= bound).all(), (shape, err.max().item())


def _inputs(shape, dev, seed, zeros=False):
    g = torch.Generator(device=dev).manual_seed(seed)
    B, C, H, W = shape
    raw = torch.randn(shape, device=dev, generator=g)
    bias = torch.randn(C, device=dev, generator=g)
    gout = torch.randn(shape, device=dev, generator=g)
    if zeros:  # half of y exactly 0, some of those -0.0
        pick = torch.rand(shape, device=dev, generator=g)
        raw = torch.where(pick < 0.5, -bias.view(1, -1, 1, 1).expand(shape), raw)
    return raw, bias, gout


@pytest.mark.parametrize("case", range(7))
def test_forward_is_bit_identical_and_in_place(hip_device, case):
    from unsamflow_amd import ops

    shape, slope = _shapes()[case]
    raw, bias, _ = _inputs(shape, hip_device, case)
    want = raw + bias.view(1, -1, 1, 1)
    if slope != 1.0:
        want = F.leaky_relu(want, slope)
    ptr = raw.data_ptr()
    out = ops.conv_epilogue_forward(raw, bias, slope)
    assert out is raw and raw.data_ptr() == ptr
    assert torch.equal(raw, want)


# the seven shapes, and the split-path shape again with a batch-strided gradient
@pytest.mark.parametrize("case,strided", [(i, False) for i in range(7)] + [(4, True)])
def test_backward_matches_aten_and_the_fp64_sum(hip_device, case, strided):
    from unsamflow_amd import ops

    shape, slope = _shapes()[case]
    B, C, H, W = shape
    raw, bias, gout = _inputs(shape, hip_device, 10 + case)
    if strided:  # a channel slice of a wider (concat) gradient: planes dense, samples strided
        big = torch.randn(B, C + 9, H, W, device=hip_device)
        big[:, 5:5 + C] = gout
        gout = big[:, 5:5 + C]
        assert not gout.is_contiguous()
    act = slope != 1.0
    y = ops.conv_epilogue_forward(raw, bias, slope) if act else None
    gin, gbias = ops.conv_epilogue_backward(gout, y, slope)
    if act:
        assert gin.is_contiguous()
        assert torch.equal(gin, torch.ops.aten.leaky_relu_backward(gout.contiguous(), y, slope, True))
    else:
        assert gin is gout  # passed on unchanged
    _check_bias(gbias, gin, shape)
    _, again = ops.conv_epilogue_backward(gout, y, slope)
    assert torch.equal(gbias, again)  # deterministic: the same bits


def test_zeros_and_negative_zeros_in_y(hip_device):
    from unsamflow_amd import ops

    shape = _split_shape()
    raw, bias, gout = _inputs(shape, hip_device, 40, zeros=True)
    y = ops.conv_epilogue_forward(raw.clone(), bias, SLOPE)
    assert torch.equal(y, F.leaky_relu(raw + bias.view(1, -1, 1, 1), SLOPE))
    frac = (y == 0).float().mean().item()
    assert 0.4 < frac < 0.6
    y[:, :, 0, ::3] = -0.0
    y[:, :, 1, ::5] = 0.0
    assert (torch.signbit(y) & (y == 0)).any()
    gin, gbias = ops.conv_epilogue_backward(gout, y, SLOPE)
    assert torch.equal(gin, torch.ops.aten.leaky_relu_backward(gout, y, SLOPE, True))
    _check_bias(gbias, gin, shape)


def test_no_bias_gradient_no_workspace(hip_device, monkeypatch):
    """needs_input_grad honoured: a frozen bias gets no gradient and the backward
    asks for no workspace (and allocates none)."""
    from unsamflow_amd import _lib, ops
    from unsamflow_amd.conv_epilogue import bias_act_

    shape = _split_shape()
    assert _parts(*shape) > 1
    lib = _lib.load()
    asked = []

    class Spy:
        def __getattr__(self, name):
            if name == "usf_convepi_bwd_workspace":
                asked.append(name)
            return getattr(lib, name)

    raw, bias, gout = _inputs(shape, hip_device, 50)
    monkeypatch.setattr(_lib, "load", lambda: Spy())
    x = raw.clone().requires_grad_(True)
    y = bias_act_(x * 1.0, bias, SLOPE)  # bias does not require grad
    (gx,) = torch.autograd.grad(y, x, gout)
    assert asked == []
    assert torch.equal(gx, torch.ops.aten.leaky_relu_backward(gout, y.detach(), SLOPE, True))
    gin, gbias = ops.conv_epilogue_backward(gout, y.detach(), SLOPE, need_bias=False)
    assert gbias is None and asked == [] and torch.equal(gin, gx)
    b2 = bias.clone().requires_grad_(True)
    y2 = bias_act_(x * 1.0, b2, SLOPE)
    y2.backward(gout)
    assert asked and b2.grad is not None


def _block_run(blk, x, gout):
    for p in blk.parameters():
        p.grad = None
    xi = x.clone().requires_grad_(True)
    out = blk(xi)
    out.backward(gout)
    return out.detach().clone(), xi.grad.clone(), blk[0].weight.grad.clone(), blk[0].bias.grad.clone()


@pytest.mark.parametrize("relu", [True, False])
def test_conv_block_fused_equals_composition(hip_device, relu, monkeypatch):
    from unsamflow_amd import pwclite

    torch.manual_seed(7)
    blk = pwclite.conv_block(4, 4, relu=relu).to(hip_device)
    x = torch.randn(2, 4, 6, 8, device=hip_device)
    gout = torch.randn(2, 4, 6, 8, device=hip_device)
    seen = []
    from unsamflow_amd import ops

    fwd = ops.conv_epilogue_forward
    monkeypatch.setattr(ops, "conv_epilogue_forward", lambda *a: (seen.append(1), fwd(*a))[1])
    on = _block_run(blk, x, gout)
    assert seen == [1]  # the fused op ran
    monkeypatch.setattr(pwclite, "FUSED_CONV_EPILOGUE", False)
    off = _block_run(blk, x, gout)
    assert seen == [1]
    assert torch.equal(on[0], off[0])
    # MIOpen's weight gradient is not bit-stable: the tolerances of test_gpu_harness.py's parameters
    torch.testing.assert_close(on[1], off[1], atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(on[2], off[2], atol=1e-5, rtol=1e-4)
    gin = torch.ops.aten.leaky_relu_backward(gout, on[0], SLOPE, True) if relu else gout
    _check_bias(on[3], gin, (2, 4, 6, 8))
    _check_bias(off[3], gin, (2, 4, 6, 8))


def test_graph_capture_and_replay_equal_eager(hip_device):
    """One fused conv_block forward and backward captured once and replayed three
    times: the workspace of the split bias gradient is a plain allocation of the
    capture's pool."""
    from unsamflow_amd import pwclite

    torch.manual_seed(9)
    B, C, H, W = _split_shape()
    blk = pwclite.conv_block(2, C).to(hip_device)
    x = torch.randn(B, 2, H, W, device=hip_device)
    gout = torch.randn(B, C, H, W, device=hip_device)
    eager = _block_run(blk, x, gout)
    sx = x.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (MIOpen's solver search)
        blk(sx).backward(gout)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    for p in blk.parameters():
        p.grad = None
    sx.grad = None
    with torch.cuda.graph(graph):
        out = blk(sx)
        out.backward(gout)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0])
        torch.testing.assert_close(sx.grad, eager[1], atol=1e-5, rtol=1e-4)
        torch.testing.assert_close(blk[0].weight.grad, eager[2], atol=1e-5, rtol=1e-4)
        assert torch.equal(blk[0].bias.grad, eager[3])  # the same input gradient bits, the same order
