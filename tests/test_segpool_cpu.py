"""The mask-feature branch's per-segment max pool and spread without a GPU: the
torch composition against the contract written as a plain per-segment loop
(forward and the G / (t + z) gradient), include/unsamflow_hip_segpool.h exported
and bound, argument rejection before any device work, and the model's switches
leaving the CPU path as it was."""
import re
import shutil
import subprocess

import pytest
import torch

import segpool_util as su
from conftest import REPO

HEADER = REPO / "include" / "unsamflow_hip_segpool.h"
SYMBOLS = ["usf_segpool_api_version", "usf_segpool_state_words", "usf_segpool_fwd_f32", "usf_segpool_bwd_f32"]


@pytest.fixture(scope="module")
def lib():
    from unsamflow_amd import _lib
    from unsamflow_amd.build import build_library

    build_library()
    return _lib.load()


def header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


# ------------------------------------------------------------ composition --
def _composition(proj, seg, gs, K=None):
    from unsamflow_amd.segpool import segment_max_spread_torch

    p = proj.clone().requires_grad_(True)
    out = segment_max_spread_torch(p, seg, K)
    (g,) = torch.autograd.grad(out, p, gs)
    return out.detach(), g


def test_the_issue_example():
    """seg = [[0,0,1,1],[2,2,1,1]], proj = [[.5,.5,-1,-2],[0,-3,-1,-4]], grad_spread = 1..8."""
    seg = torch.tensor([[0., 0, 1, 1], [2, 2, 1, 1]]).reshape(1, 1, 2, 4)
    proj = torch.tensor([[.5, .5, -1, -2], [0, -3, -1, -4]]).reshape(1, 1, 2, 4)
    gs = torch.arange(1., 9.).reshape(1, 1, 2, 4)
    out, g = _composition(proj, seg, gs)
    assert torch.equal(out, torch.tensor([[.5, .5, 0, 0], [0, 0, 0, 0]]).reshape(1, 1, 2, 4))
    want = torch.tensor([[1.5, 1.5, 0, 0], [11 / 7, 0, 0, 0]]).reshape(1, 1, 2, 4)
    assert torch.allclose(g, want, rtol=1e-6, atol=0)
    ref_out, ref_g = su.loop_reference(proj, seg, gs)
    assert torch.equal(ref_out, out)
    assert torch.allclose(ref_g, want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_composition_equals_the_per_segment_loop(quantised, dtype):
    gen = torch.Generator().manual_seed(11 + quantised)
    B, C, h, w, K = 2, 3, 6, 10, 7
    seg = su.block_segments(B, h, w, K, 2, gen)
    seg[1] = 3.0  # one id covers a whole sample: no zero joins the maximum there
    proj = su.values((B, C, h, w), gen, quantised).to(dtype)
    proj[1, 0] = -proj[1, 0].abs() - 0.25  # ... and all of its values are negative
    su.force_negative_segment(proj, seg, 0, 1)  # a partial segment below 0: pooled to 0, no gradient
    gs = torch.randn((B, C, h, w), generator=gen).to(dtype)
    out, g = _composition(proj, seg, gs)
    ref_out, ref_g = su.loop_reference(proj, seg, gs)
    assert torch.equal(out, ref_out)
    assert (out[1, 0] < 0).all()
    tol = 1e-5 if dtype == torch.float32 else 1e-13
    assert (g - ref_g).abs().max() <= tol * ref_g.abs().max()
    assert torch.equal(g == 0, ref_g == 0)
    if quantised:  # what the quantised inputs are there for
        assert su.input_features(proj, seg, K) == (True, True, True)


def test_num_segments_only_pads_the_one_hot():
    gen = torch.Generator().manual_seed(5)
    seg = su.block_segments(1, 4, 6, 3, 2, gen)
    proj = torch.randn((1, 2, 4, 6), generator=gen)
    gs = torch.randn((1, 2, 4, 6), generator=gen)
    a, ga = _composition(proj, seg, gs)
    b, gb = _composition(proj, seg, gs, K=9)
    assert torch.equal(a, b) and torch.equal(ga, gb)


def test_public_op_on_cpu_is_the_composition():
    from unsamflow_amd.segpool import segment_max_spread, segment_max_spread_torch

    gen = torch.Generator().manual_seed(6)
    seg = su.block_segments(2, 5, 7, 4, 3, gen)
    proj = torch.randn((2, 3, 5, 7), generator=gen)
    assert torch.equal(segment_max_spread(proj, seg), segment_max_spread_torch(proj, seg))
    assert torch.equal(segment_max_spread(proj, seg.long(), 4, fused=False), segment_max_spread_torch(proj, seg, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        segment_max_spread(proj, seg, 4, fused=True)


# ------------------------------------------------------------------ C ABI --
def test_header_declares_exactly_the_bound_symbols():
    from unsamflow_amd import _lib

    declared = sorted(set(re.findall(r"\b(usf_\w+)\s*\(", header_text())))
    assert declared == sorted(SYMBOLS) == sorted(_lib.SEGPOOL_SYMBOLS)
    others = set(_lib.EXPORTED_SYMBOLS) | set(_lib.CENSUS_SYMBOLS) | set(_lib.AR_SYMBOLS)
    assert not set(_lib.SEGPOOL_SYMBOLS) & others
    for name, (argtypes, _) in _lib.SEGPOOL_SYMBOLS.items():
        m = re.search(name + r"\s*\(([^)]*)\)", header_text())
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(argtypes), name
    text = HEADER.read_text()
    assert int(re.search(r"#define USF_SEGPOOL_MAX_K (\d+)", text).group(1)) == _lib.SEGPOOL_MAX_K >= 1024
    bit = int(re.search(r"#define USF_DEVERR_SEGPOOL_BAD_ID (\d+)", text).group(1))
    assert bit == _lib.DEVERR_SEGPOOL_BAD_ID and bit not in (1, 2) and bit & (bit - 1) == 0
    assert int(re.search(r"#define USF_SEGPOOL_API_VERSION (\d+)", text).group(1)) == _lib.SEGPOOL_API_VERSION


def test_library_exports_and_binds_the_entries(lib):
    from unsamflow_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.library_path())], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (usf_\w+)", out))
    for s in SYMBOLS:
        assert s in exported, s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.usf_segpool_api_version() == _lib.SEGPOOL_API_VERSION == 1
    assert lib.usf_abi_version() == _lib.ABI_VERSION == 8
    assert "#define USF_ABI_VERSION 8" in (REPO / "include" / "unsamflow_hip.h").read_text()


def test_build_id_covers_the_segpool_sources():
    from unsamflow_amd import build

    assert "segpool.hip" in build.SOURCES and HEADER.name in build.PUBLIC_HEADERS
    before = build.build_id()
    at = build.SOURCES.index("segpool.hip")
    build.SOURCES.remove("segpool.hip")
    try:
        assert build.build_id() != before
    finally:
        build.SOURCES.insert(at, "segpool.hip")
    assert build.build_id() == before


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc not available")
def test_segpool_kernels_do_not_spill():
    """The tables' fill, the table pass, both instantiations of the dense pass and the backward:
    no scratch, at most 64 VGPRs (8 waves/SIMD); their LDS is dynamic (K-sized)."""
    import sys

    sys.path.insert(0, str(REPO / "tools"))
    import kernel_resources

    res = kernel_resources.resources(REPO / "unsamflow_amd" / "csrc" / "segpool.hip")
    assert len(res) == 5, [r[0] for r in res]
    for name, vgpr, lds, scratch in res:
        assert scratch == 0, (name, scratch)
        assert vgpr <= 64 and lds == 0, (name, vgpr, lds)


def test_state_words(lib):
    # [B,C,K] maxima and [B,K] pixel counts
    assert lib.usf_segpool_state_words(2, 32, 40) == 2 * 32 * 40 + 2 * 40
    assert lib.usf_segpool_state_words(1, 1, 1024) == 2048
    assert lib.usf_segpool_state_words(1, 1, 1025) == 0
    assert lib.usf_segpool_state_words(1, 1, 0) == 0
    assert lib.usf_segpool_state_words(0, 4, 8) == 0


# dummy non-null pointers (never dereferenced: every call is rejected before a launch)
def _fwd(L, proj=4, seg=4, spread=4, state=4, B=1, C=2, H=3, W=4, K=5):
    return L.usf_segpool_fwd_f32(proj, seg, spread, state, B, C, H, W, K, None)


def _bwd(L, proj=4, seg=4, state=4, gs=4, gp=4, B=1, C=2, H=3, W=4, K=5):
    return L.usf_segpool_bwd_f32(proj, seg, state, gs, gp, B, C, H, W, K, None)


@pytest.mark.parametrize(
    "call,needle",
    [
        (lambda L: _fwd(L, K=0), "K=0 outside"),
        (lambda L: _fwd(L, K=-2), "K=-2 outside"),
        (lambda L: _fwd(L, K=1025), "K=1025 outside"),
        (lambda L: _fwd(L, proj=None), "null input"),
        (lambda L: _fwd(L, seg=None), "null input"),
        (lambda L: _fwd(L, spread=None), "null output"),
        (lambda L: _fwd(L, state=None), "null output"),
        (lambda L: _fwd(L, state=6), "4-byte aligned"),
        (lambda L: _fwd(L, H=0), "non-positive"),
        (lambda L: _fwd(L, W=0), "non-positive"),
        (lambda L: _fwd(L, B=0), "non-positive"),
        (lambda L: _fwd(L, C=0), "non-positive"),
        (lambda L: _fwd(L, B=65536), "B=65536"),
        (lambda L: _fwd(L, C=65536, H=1, W=1), "C=65536"),
        (lambda L: _fwd(L, H=16384, W=16384, C=32), "too large"),
        (lambda L: _bwd(L, K=0), "K=0 outside"),
        (lambda L: _bwd(L, K=1025), "K=1025 outside"),
        (lambda L: _bwd(L, proj=None), "null input"),
        (lambda L: _bwd(L, seg=None), "null input"),
        (lambda L: _bwd(L, state=None), "null input"),
        (lambda L: _bwd(L, gs=None), "null input"),
        (lambda L: _bwd(L, gp=None), "null output"),
        (lambda L: _bwd(L, H=0), "non-positive"),
        (lambda L: _bwd(L, W=0), "non-positive"),
        # the alignment contract (include/unsamflow_hip_segpool.h): 20 where 16 bytes are required, 18 where 4
        (lambda L: _fwd(L, proj=20, seg=16, spread=16, state=16), "proj must be 16-byte aligned"),
        (lambda L: _fwd(L, proj=16, seg=16, spread=24, state=16), "spread must be 16-byte aligned"),
        (lambda L: _fwd(L, proj=16, seg=16, spread=16, state=18), "state not 4-byte aligned"),
        (lambda L: _bwd(L, proj=16, seg=20, state=16, gs=16, gp=16), "seg must be 16-byte aligned"),
        (lambda L: _bwd(L, proj=16, seg=16, state=16, gs=16, gp=20), "grad_proj must be 16-byte aligned"),
        (lambda L: _bwd(L, proj=16, seg=16, state=18, gs=16, gp=16), "state not 4-byte aligned"),
    ],
)
def test_invalid_arguments_rejected_without_launch(lib, call, needle):
    assert call(lib) == -1
    msg = lib.usf_last_error_string().decode()
    assert needle in msg, msg


def test_ops_refuse_bad_tensors_before_the_library():
    from unsamflow_amd import ops

    proj, seg = torch.zeros(1, 2, 3, 4), torch.zeros(1, 1, 3, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.segpool_forward(proj, seg, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.segpool_backward(proj, seg, torch.zeros(12, dtype=torch.int32), proj, 4)


# ------------------------------------------------------------------- model --
def test_cpu_model_keeps_the_composition_under_every_switch(monkeypatch):
    """CPU tensors never take the fused pooling or the shared branch: the flows
    are the same bits whatever the switches say."""
    from oracle.torch_ref import OracleCorrelation, oracle_flow_warp
    from unsamflow_amd import config, pwclite
    from unsamflow_amd.harness import synthetic_pair

    cfg = config.sintel_mf()
    torch.manual_seed(0)
    model = pwclite.PWCLite(cfg.model, corr_module=OracleCorrelation(4), warp_fn=oracle_flow_warp)
    assert pwclite.FUSED_SEG_POOL and pwclite.SHARED_MASK_FEATURE
    img1, img2, seg1, seg2 = synthetic_pair(1, 128, 256, "cpu", with_seg=True)
    with torch.no_grad():
        on = model(img1, img2, seg1, seg2, with_bk=True)
        monkeypatch.setattr(pwclite, "FUSED_SEG_POOL", False)
        monkeypatch.setattr(pwclite, "SHARED_MASK_FEATURE", False)
        off = model(img1, img2, seg1, seg2, with_bk=True)
    for key in ("flows_12", "flows_21"):
        for a, b in zip(on[key], off[key]):
            assert torch.equal(a, b)
