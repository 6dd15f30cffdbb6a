"""The conv epilogues without a GPU: include/unsamflow_hip_convepi.h exported and
bound, argument rejection before any device work, the workspace sizes of the
bias-gradient split, and conv_block keeping its layout, its state-dict keys and
its CPU composition."""
import re
import subprocess

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import REPO, load_golden

HEADER = REPO / "include" / "unsamflow_hip_convepi.h"
SYMBOLS = ["usf_convepi_api_version", "usf_convepi_fwd_f32", "usf_convepi_bwd_f32", "usf_convepi_bwd_workspace"]


@pytest.fixture(scope="module")
def lib():
    from unsamflow_amd import _lib
    from unsamflow_amd.build import build_library

    build_library()
    return _lib.load()


def header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


# ------------------------------------------------------------------ C ABI --
def test_header_declares_exactly_the_bound_symbols():
    from unsamflow_amd import _lib

    declared = sorted(set(re.findall(r"\b(usf_\w+)\s*\(", header_text())))
    assert declared == sorted(SYMBOLS) == sorted(_lib.CONVEPI_SYMBOLS)
    others = (set(_lib.EXPORTED_SYMBOLS) | set(_lib.CENSUS_SYMBOLS) | set(_lib.AR_SYMBOLS) | set(_lib.SEGPOOL_SYMBOLS)
              | set(_lib.HG_SYMBOLS))
    assert not set(_lib.CONVEPI_SYMBOLS) & others
    for name, (argtypes, _) in _lib.CONVEPI_SYMBOLS.items():
        m = re.search(name + r"\s*\(([^)]*)\)", header_text())
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(argtypes), name
    text = HEADER.read_text()
    assert int(re.search(r"#define USF_CONVEPI_API_VERSION (\d+)", text).group(1)) == _lib.CONVEPI_API_VERSION
    assert int(re.search(r"#define USF_CONVEPI_TILE_SLOTS (\d+)", text).group(1)) == _lib.CONVEPI_TILE_SLOTS
    assert int(re.search(r"#define USF_CONVEPI_CHAIN (\d+)", text).group(1)) == _lib.CONVEPI_CHAIN == 64
    assert int(re.search(r"#define USF_CONVEPI_TARGET_WGS (\d+)", text).group(1)) == _lib.CONVEPI_TARGET_WGS


def test_library_exports_and_binds_the_entries(lib):
    from unsamflow_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.library_path())], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (usf_\w+)", out))
    for s in SYMBOLS:
        assert s in exported, s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.usf_convepi_api_version() == _lib.CONVEPI_API_VERSION == 1
    assert lib.usf_abi_version() == _lib.ABI_VERSION == 8
    assert "#define USF_ABI_VERSION 8" in (REPO / "include" / "unsamflow_hip.h").read_text()


def test_build_lists_the_convepi_sources():
    from unsamflow_amd import build

    assert "convepi.hip" in build.SOURCES and HEADER.name in build.PUBLIC_HEADERS


def test_workspace_follows_the_split(lib):
    """0 where one workgroup owns a channel; C * parts where the channel's tiles
    (1024 slots of 16 bytes over B * ceil((H*W + 3) / 4) slots) are split."""
    from unsamflow_amd import _lib

    ws = lib.usf_convepi_bwd_workspace
    assert ws(1, 1, 1, 1) == 0 and ws(2, 3, 5, 7) == 0 and ws(16, 192, 4, 13) == 0 and ws(16, 2, 4, 13) == 0
    # the two large levels of the workload: split, every part within the chain cap
    for B, C, H, W in [(16, 16, 128, 416), (16, 32, 64, 208), (16, 128, 64, 208)]:
        n = ws(B, C, H, W)
        tiles = -(-B * ((H * W + 6) // 4) // _lib.CONVEPI_TILE_SLOTS)
        assert n > 0 and n % C == 0
        parts = n // C
        assert 1 < parts <= tiles and -(-tiles // parts) <= _lib.CONVEPI_CHAIN
        assert C * parts >= 1024  # enough workgroups for 256 compute units
    assert ws(0, 1, 1, 1) == -1 and ws(1, 1, 1, -3) == -1


def _fwd(L, y=16, bias=4, B=1, C=2, H=3, W=4, slope=0.1):
    return L.usf_convepi_fwd_f32(y, bias, B, C, H, W, slope, None)


def _bwd(L, go=4, gbs=24, y=16, gin=32, gb=4, ws=None, nws=0, B=1, C=2, H=3, W=4, slope=0.1):
    return L.usf_convepi_bwd_f32(go, gbs, y, gin, gb, ws, nws, B, C, H, W, slope, None)


# dummy non-null pointers (never dereferenced: every call is rejected before a launch)
@pytest.mark.parametrize(
    "call,needle",
    [
        (lambda L: _fwd(L, y=None), "null pointer"),
        (lambda L: _fwd(L, bias=None), "null pointer"),
        (lambda L: _fwd(L, y=20), "16-byte"),
        (lambda L: _fwd(L, bias=6), "4-byte aligned"),
        (lambda L: _fwd(L, slope=0.0), "must be > 0"),
        (lambda L: _fwd(L, slope=-0.1), "must be > 0"),
        (lambda L: _fwd(L, slope=float("nan")), "must be > 0"),
        (lambda L: _fwd(L, B=0), "non-positive"),
        (lambda L: _fwd(L, W=0), "non-positive"),
        (lambda L: _fwd(L, H=16384, W=16384, C=32), "too large"),
        (lambda L: _bwd(L, go=None), "grad_out null"),
        (lambda L: _bwd(L, go=6), "grad_out null or misaligned"),
        (lambda L: _bwd(L, gbs=23), "gout_bstride=23"),
        (lambda L: _bwd(L, y=None), "16-byte aligned tensors with an activation"),
        (lambda L: _bwd(L, gin=None), "16-byte aligned tensors with an activation"),
        (lambda L: _bwd(L, gin=36), "16-byte aligned tensors with an activation"),
        (lambda L: _bwd(L, slope=1.0), "NULL without"),
        (lambda L: _bwd(L, slope=1.0, y=None, gin=None, gb=None), "nothing to compute"),
        (lambda L: _bwd(L, slope=0.0), "must be > 0"),
        (lambda L: _bwd(L, gb=6), "grad_bias misaligned"),
        (lambda L: _bwd(L, B=16, C=16, H=128, W=416, gbs=16 * 128 * 416), "workspace of"),
        (lambda L: _bwd(L, B=16, C=16, H=128, W=416, gbs=16 * 128 * 416, ws=64, nws=16), "short"),
        (lambda L: _bwd(L, C=0), "non-positive"),
        # the alignment contract (include/unsamflow_hip_convepi.h): 20 where 16 bytes are required, 18 where 4
        (lambda L: _fwd(L, y=20), "y must be 16-byte"),
        (lambda L: _fwd(L, bias=18), "bias 4-byte aligned"),
        (lambda L: _bwd(L, go=18), "misaligned, or gout_bstride"),
        (lambda L: _bwd(L, y=20), "16-byte aligned tensors"),
        (lambda L: _bwd(L, gin=24), "16-byte aligned tensors"),
        (lambda L: _bwd(L, gb=18), "misaligned, or workspace"),
    ],
)
def test_invalid_arguments_rejected_without_launch(lib, call, needle):
    assert call(lib) == -1
    msg = lib.usf_last_error_string().decode()
    assert needle in msg, msg


def test_ops_refuse_bad_tensors_before_the_library():
    from unsamflow_amd import ops

    y, bias = torch.zeros(1, 2, 3, 4), torch.zeros(2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.conv_epilogue_forward(y, bias, 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.conv_epilogue_backward(y, y, 0.1)


# ------------------------------------------------------------------- model --
def test_conv_block_keeps_its_layout():
    from unsamflow_amd import pwclite

    blk = pwclite.conv_block(3, 5, stride=2)
    assert isinstance(blk, nn.Sequential) and len(blk) == 2
    assert isinstance(blk[0], nn.Conv2d) and isinstance(blk[1], nn.LeakyReLU)
    assert blk[1].negative_slope == 0.1 and blk[1].inplace
    assert list(blk.state_dict()) == ["0.weight", "0.bias"]
    head = pwclite.conv_block(3, 2, relu=False)
    assert len(head) == 1 and list(head.state_dict()) == ["0.weight", "0.bias"]
    assert pwclite.FUSED_CONV_EPILOGUE is True and pwclite.FUSED_UP_WARP is True


@pytest.mark.parametrize("relu", [True, False])
def test_conv_block_on_cpu_is_the_composition(relu, monkeypatch):
    """CPU tensors never reach the fused op: the Sequential's own result, bit for
    bit, in the output and in every gradient, whatever the switch says."""
    from unsamflow_amd import pwclite

    torch.manual_seed(3)
    blk = pwclite.conv_block(4, 6, 3, 1, 2, relu=relu)
    x = torch.randn(2, 4, 6, 8)

    def run():
        for p in blk.parameters():
            p.grad = None
        xi = x.clone().requires_grad_(True)
        out = blk(xi)
        out.square().sum().backward()
        return out.detach(), xi.grad, blk[0].weight.grad.clone(), blk[0].bias.grad.clone()

    on = run()
    want = F.conv2d(x, blk[0].weight, blk[0].bias, 1, 2, 2)
    assert torch.equal(on[0], F.leaky_relu(want, 0.1) if relu else want)
    monkeypatch.setattr(pwclite, "FUSED_CONV_EPILOGUE", False)
    for a, b in zip(on, run()):
        assert torch.equal(a, b)


def test_reference_layout_state_dict_still_loads():
    """The parameter names of the reference checkpoint layout (recorded in the
    golden file) are the model's keys, and a state dict under them loads."""
    from oracle.torch_ref import OracleCorrelation, oracle_flow_warp
    from unsamflow_amd.config import kitti_base
    from unsamflow_amd.pwclite import ConvBlock, PWCLite

    names = [str(n) for n in load_golden("pwclite_kitti.npz")["param_names"]]
    model = PWCLite(kitti_base().model, corr_module=OracleCorrelation(4), warp_fn=oracle_flow_warp)
    assert list(model.state_dict().keys()) == names
    sd = {n: torch.full_like(p, 0.5) for n, p in model.state_dict().items()}
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(bool((p == 0.5).all()) for p in model.parameters())
    blocks = [m for m in model.modules() if isinstance(m, ConvBlock)]
    assert len(blocks) > 20 and not any(m.fused for m in blocks)  # injected ops: the composition
    assert all(m.fused for m in PWCLite(kitti_base().model).modules() if isinstance(m, ConvBlock))
