"""Validation without a GPU: the torch composition of resize_flow +
evaluate_flow, the numpy drop-in and the fp64 restatement against the reference
capture (tests/golden/flow_eval.npz, made by tests/golden/make_golden_eval.py),
the generator's cap on invalidated pixels, include/unsamflow_hip_eval.h exported
and bound, argument rejection before any device work, FlowMetrics across two
gloo ranks, and the Validator's mode handling on a stand-in model.

Tolerances: EPE numbers and the resized flow atol = rtol = 1e-5 against the
capture (the warp / correlation contract; the reference's own fp32
numbers lie within 2.2e-7 relative of fp64 on these inputs); bad-pixel counts
exactly the recorded fp64 counts (tests/eval_util removed the only pixels that
could flip); Fl rates rtol 1e-5."""
import os
import re
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import eval_util
from conftest import REPO, load_golden

HEADER = REPO / "include" / "unsamflow_hip_eval.h"
SYMBOLS = ["usf_eval_api_version", "usf_flow_resize_f32", "usf_flow_eval_partials", "usf_flow_eval_f32"]
CASES = list(eval_util.CASES)
EPE_COLS, FL_COLS, TOL = eval_util.EPE_COLS, eval_util.FL_COLS, eval_util.TOL


@pytest.fixture(scope="module")
def lib():
    from unsamflow_amd import _lib
    from unsamflow_amd.build import build_library

    build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return load_golden("flow_eval.npz")


check_metrics, check_counts = eval_util.check_metrics, eval_util.check_counts


# ------------------------------------------------------------- the capture --
@pytest.mark.parametrize("name", CASES)
def test_capture_matches_the_case_table(golden, name):
    B, (h, w), sizes, seed = eval_util.CASES[name]
    assert tuple(golden[f"{name}_shape"]) == (B, h, w) and int(golden[f"{name}_seed"]) == seed
    assert np.array_equal(golden[f"{name}_sizes"], np.array(sizes))
    assert np.array_equal(golden[f"{name}_ret5"], golden[f"{name}_ret7"][:5])
    # a batch's return is the mean of its samples' (evaluate_flow's error / B)
    np.testing.assert_allclose(golden[f"{name}_ret7"], golden[f"{name}_sample7"].mean(axis=0), rtol=1e-6)


@pytest.mark.parametrize("name", CASES)
def test_generator_invalidates_at_most_two_per_mille(name):
    c = eval_util.case(name)
    assert c["valid_before"] > 0 and c["invalidated"] <= 0.002 * c["valid_before"]
    print(f"[eval] {name}: invalidated {c['invalidated']} of {c['valid_before']} valid pixels")
    for gt, mv in zip(c["gts"], c["moves"]):
        valid, noc = gt[..., 2], gt[..., 3]
        assert set(np.unique(valid)) <= {0.0, 1.0} and np.all(noc <= valid) and set(np.unique(mv)) <= {0.0, 1.0}
        if valid.size >= 5000:  # the shares (60 %, 75 % of valid, 30 %): 3 sigma at 5000 draws is 2 points
            assert 0.57 < valid.mean() < 0.63 and 0.72 < noc.sum() / valid.sum() < 0.78 and 0.27 < mv.mean() < 0.33


@pytest.mark.parametrize("name", CASES)
def test_fp64_restatement_matches_the_capture(golden, name):
    c = eval_util.case(name)
    m, bad = eval_util.evaluate_f64(c["pred"], c["gts"], c["moves"])
    check_metrics(m, golden, name)
    assert np.array_equal(bad, golden[f"{name}_bad"])
    assert np.array_equal(m[:, FL_COLS], golden[f"{name}_sample7"][:, FL_COLS])  # the rates: exactly
    m2, _ = eval_util.evaluate_f64(c["pred"], [g[..., :2] for g in c["gts"]])
    check_metrics(m2, golden, name, channels=2)


# ------------------------------------------------------------- composition --
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("move", [True, False])
def test_composition_matches_the_reference_capture(golden, name, move):
    from unsamflow_amd.evaluate import flow_errors

    c = eval_util.case(name)
    gt, mv = (torch.from_numpy(a) for a in eval_util.planar_batch(c))
    metrics, sums = flow_errors(torch.from_numpy(c["pred"]), gt, torch.from_numpy(c["sizes"]), mv if move else None)
    assert metrics.shape == (c["B"], 7) and sums.shape == (c["B"], 12) and metrics.dtype == torch.float32
    check_metrics(metrics.numpy(), golden, name, move=move)
    check_counts(sums.numpy(), golden, name)


@pytest.mark.parametrize("name", CASES)
def test_composition_two_channel_ground_truth(golden, name):
    from unsamflow_amd.evaluate import flow_errors

    c = eval_util.case(name)
    gt, _ = eval_util.planar_batch(c, channels=2)
    metrics, sums = flow_errors(torch.from_numpy(c["pred"]), torch.from_numpy(gt), torch.from_numpy(c["sizes"]))
    check_metrics(metrics.numpy(), golden, name, channels=2)
    # valid = noc = 1: both masks count every pixel of the window, nothing is occluded
    area = c["sizes"].prod(axis=1)
    assert np.array_equal(sums[:, 1].numpy(), area) and np.array_equal(sums[:, 3].numpy(), area)
    assert float(sums[:, 4:6].abs().max()) == 0.0 and torch.equal(metrics[:, 0], metrics[:, 1])


@pytest.mark.parametrize("name", CASES)
def test_evaluate_flow_drop_in(golden, name):
    """The reference's interface: lists of HWC numpy ground truths, an NHWC
    numpy prediction -> 7, 5 or 1 Python floats."""
    from unsamflow_amd.evaluate import evaluate_flow

    c = eval_util.case(name)
    pred = np.ascontiguousarray(c["pred"].transpose(0, 2, 3, 1))
    r7 = evaluate_flow(c["gts"], pred, c["moves"], device="cpu")
    r5 = evaluate_flow(c["gts"], pred, device="cpu")
    r1 = evaluate_flow([g[..., :2] for g in c["gts"]], pred, device="cpu")
    assert [len(r7), len(r5), len(r1)] == [7, 5, 1] and all(isinstance(v, float) for v in r7 + r5 + r1)
    np.testing.assert_allclose(r7, golden[f"{name}_ret7"], **TOL)
    np.testing.assert_allclose(r5, golden[f"{name}_ret5"], **TOL)
    np.testing.assert_allclose(r1, golden[f"{name}_ret1"], **TOL)


@pytest.mark.parametrize("name", eval_util.SMALL)
def test_resize_flow_composition(golden, name):
    from unsamflow_amd.evaluate import resize_flow

    c = eval_util.case(name)
    pred = torch.from_numpy(c["pred"])
    Hmax, Wmax = (int(v) for v in c["sizes"].max(axis=0))
    table = resize_flow(pred, (Hmax, Wmax), sizes=torch.from_numpy(c["sizes"]))
    for b, (H, W) in enumerate(c["sizes"]):
        want = golden[f"{name}_resized_{b}"]
        np.testing.assert_allclose(resize_flow(pred[b:b + 1], (H, W))[0].numpy(), want, **TOL)
        np.testing.assert_allclose(table[b, :, :H, :W].numpy(), want, **TOL)
        assert float(table[b, :, H:].abs().sum()) == 0.0 and float(table[b, :, :, W:].abs().sum()) == 0.0
        np.testing.assert_allclose(eval_util.resize_f64(c["pred"][b], int(H), int(W)), want, **TOL)


def test_empty_masks_and_bad_sizes_follow_the_documented_nan_cases():
    from unsamflow_amd.evaluate import flow_errors

    c = eval_util.case("ragged_small")
    gt, mv = (torch.from_numpy(a) for a in eval_util.planar_batch(c))
    pred = torch.from_numpy(c["pred"])
    ref, ref_sums = flow_errors(pred, gt, torch.from_numpy(c["sizes"]), mv)
    empty = gt.clone()
    empty[0, 3] = 0.0  # sample 0: no non-occluded pixel -> EPE_noc, Fl_noc 0/0; EPE_occ = EPE_all
    m, _ = flow_errors(pred, empty, torch.from_numpy(c["sizes"]), mv)
    assert torch.isnan(m[0, [1, 4]]).all() and not torch.isnan(m[0, [0, 2, 3, 5, 6]]).any()
    assert torch.equal(m[1], ref[1])
    for bad in ([1, 23], [12, 23], [11, 24], [11, 1], [-3, 5], [0, 0]):
        sizes = torch.tensor([bad, [9, 19]], dtype=torch.int32)
        m, s = flow_errors(pred, gt, sizes, mv)
        assert torch.isnan(m[0]).all() and float(s[0].abs().max()) == 0.0, bad
        assert torch.equal(m[1], ref[1]) and torch.equal(s[1], ref_sums[1])


# ------------------------------------------------------ library and header --
def header_text():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def test_header_declares_exactly_the_bound_symbols():
    from unsamflow_amd import _lib, build

    declared = sorted(set(re.findall(r"\b(usf_\w+)\s*\(", header_text())))
    assert declared == sorted(SYMBOLS) == sorted(_lib.EVAL_SYMBOLS)
    others = (set(_lib.EXPORTED_SYMBOLS) | set(_lib.CENSUS_SYMBOLS) | set(_lib.AR_SYMBOLS) | set(_lib.SEGPOOL_SYMBOLS)
              | set(_lib.HG_SYMBOLS) | set(_lib.CONVEPI_SYMBOLS) | set(_lib.FAKEOBJ_SYMBOLS))
    assert not set(_lib.EVAL_SYMBOLS) & others
    for name, (argtypes, _) in _lib.EVAL_SYMBOLS.items():
        m = re.search(name + r"\s*\(([^)]*)\)", header_text())
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(argtypes), name
    text = HEADER.read_text()
    bit = int(re.search(r"#define USF_DEVERR_EVAL_BAD_SIZE (\d+)", text).group(1))
    # the next free bit after USF_DEVERR_FAKEOBJ_BAD_SLOT
    assert bit == _lib.DEVERR_EVAL_BAD_SIZE == 2 * _lib.DEVERR_FAKEOBJ_BAD_SLOT == 32
    assert int(re.search(r"#define USF_EVAL_NACC (\d+)", text).group(1)) == _lib.EVAL_NACC == 12
    assert int(re.search(r"#define USF_EVAL_NMETRIC (\d+)", text).group(1)) == _lib.EVAL_NMETRIC == 7
    assert int(re.search(r"#define USF_EVAL_API_VERSION (\d+)", text).group(1)) == _lib.EVAL_API_VERSION == 1
    assert "eval.hip" in build.SOURCES and "resize_tap.h" in build.HEADERS and HEADER.name in build.PUBLIC_HEADERS
    # the main header and its version are untouched
    main = (REPO / "include" / "unsamflow_hip.h").read_text()
    assert "#define USF_ABI_VERSION 8" in main and "usf_flow_eval" not in main and "usf_eval" not in main


def test_library_exports_and_binds_the_entries(lib):
    from unsamflow_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.library_path())], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\bT (usf_\w+)", out))
    for s in SYMBOLS:
        assert s in exported, s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.usf_eval_api_version() == _lib.EVAL_API_VERSION == 1
    assert lib.usf_abi_version() == 8  # the main ABI is untouched
    # one row of 12 words per workgroup; a workgroup takes 256 threads x 2 groups of 4 elements
    # (Hmax Wmax % 4 == 0) or of 1 element
    assert lib.usf_flow_eval_partials(2, 70, 150) == 12 * 2 * 6      # 10500 / 2048 -> 6
    assert lib.usf_flow_eval_partials(2, 11, 23) == 12 * 2 * 1       # 253 / 512 -> 1
    assert lib.usf_flow_eval_partials(2, 375, 1242) == 12 * 2 * 910  # 465750 / 512 -> 910
    assert lib.usf_flow_eval_partials(0, 8, 8) == 0 and lib.usf_flow_eval_partials(1, -8, 8) == 0


@pytest.mark.skipif(shutil.which("/opt/rocm/bin/hipcc") is None, reason="hipcc not available")
def test_eval_kernels_do_not_spill():
    """Two resize and two evaluation instantiations (4 elements per group, or 1)
    and the finalisation: no scratch, at most 96 VGPRs (5 waves/SIMD of the 512
    per lane: streaming kernels that hide their plane loads by occupancy), LDS
    only for the reductions' slots (12 sums x 4 waves, fp64 in the finalisation)."""
    sys.path.insert(0, str(REPO / "tools"))
    import kernel_resources

    res = kernel_resources.resources(REPO / "unsamflow_amd" / "csrc" / "eval.hip")
    assert len(res) == 5 and sum("flow_eval_kernel" in r[0] for r in res) == 2, [r[0] for r in res]
    for name, vgpr, lds, scratch in res:
        print(f"[eval] {name}: {vgpr} VGPRs, {lds} B LDS, scratch {scratch}")
        assert scratch == 0, (name, scratch)
        assert vgpr <= 96 and lds <= 12 * 4 * 8, (name, vgpr, lds)


# dummy non-null pointers (never dereferenced: every call is rejected before a launch)
def _resize(L, pred=16, pbs=24, sizes=16, out=16, B=1, h=3, w=4, Hmax=5, Wmax=6):
    return L.usf_flow_resize_f32(pred, pbs, sizes, out, B, h, w, Hmax, Wmax, None)


def _eval(L, pred=16, pbs=24, gt=16, Cg=4, move=16, sizes=16, part=16, sums=16, metrics=16, B=1, h=3, w=4, Hmax=5,
          Wmax=6):
    return L.usf_flow_eval_f32(pred, pbs, gt, Cg, move, sizes, part, sums, metrics, B, h, w, Hmax, Wmax, None)


@pytest.mark.parametrize(
    "call,needle",
    [
        (lambda L: _resize(L, h=1), "every size >= 2"),
        (lambda L: _resize(L, w=1), "every size >= 2"),
        (lambda L: _resize(L, Hmax=1), "every size >= 2"),
        (lambda L: _resize(L, Wmax=0), "every size >= 2"),
        (lambda L: _resize(L, B=0), "B=0 outside"),
        (lambda L: _resize(L, B=65536), "B=65536 outside"),
        (lambda L: _resize(L, B=2, pbs=23), "< 2*h*w"),
        (lambda L: _resize(L, pred=None), "null input"),
        (lambda L: _resize(L, out=None), "null output"),
        (lambda L: _resize(L, pred=18), "pred must be 4-byte aligned"),
        (lambda L: _resize(L, sizes=18), "sizes must be 4-byte aligned"),
        (lambda L: _resize(L, out=20), "out must be 16-byte aligned"),
        (lambda L: _eval(L, h=1), "every size >= 2"),
        (lambda L: _eval(L, w=-4), "every size >= 2"),
        (lambda L: _eval(L, Hmax=1), "every size >= 2"),
        (lambda L: _eval(L, Wmax=1), "every size >= 2"),
        (lambda L: _eval(L, Cg=3), "Cg=3"),
        (lambda L: _eval(L, Cg=1), "Cg=1"),
        (lambda L: _eval(L, Cg=5), "Cg=5"),
        (lambda L: _eval(L, B=0), "B=0 outside"),
        (lambda L: _eval(L, B=-1), "B=-1 outside"),
        (lambda L: _eval(L, B=70000), "B=70000 outside"),
        (lambda L: _eval(L, B=2, pbs=23), "< 2*h*w"),
        (lambda L: _eval(L, pred=None), "null input"),
        (lambda L: _eval(L, gt=None), "null input"),
        (lambda L: _eval(L, part=None), "null output"),
        (lambda L: _eval(L, sums=None), "null output"),
        (lambda L: _eval(L, metrics=None), "null output"),
        (lambda L: _eval(L, pred=18), "pred must be 4-byte aligned"),
        (lambda L: _eval(L, sizes=22), "sizes must be 4-byte aligned"),
        (lambda L: _eval(L, gt=20), "gt must be 16-byte aligned"),
        (lambda L: _eval(L, move=24), "move must be 16-byte aligned"),
        (lambda L: _eval(L, part=20), "partials must be 16-byte aligned"),
        (lambda L: _eval(L, sums=24), "sums must be 16-byte aligned"),
        (lambda L: _eval(L, metrics=28), "metrics must be 16-byte aligned"),
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
        ops.flow_resize(z(1, 2, 4, 6), None, 8, 12)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.flow_eval(z(1, 2, 4, 6), z(1, 4, 8, 12))


# ------------------------------------------------------------- FlowMetrics --
def test_flow_metrics_is_the_mean_over_samples(golden):
    from unsamflow_amd.evaluate import FLOW_ERROR_NAMES, FlowMetrics

    assert FLOW_ERROR_NAMES["kitti"] == ("EPE_all", "EPE_noc", "EPE_occ", "Fl_all", "Fl_noc")
    assert FLOW_ERROR_NAMES["sintel"] == ("EPE_all", "EPE_noc", "EPE_occ")
    fm = FlowMetrics("kitti_move")
    per_sample = []
    for name in ("ragged_small", "identity"):
        c = eval_util.case(name)
        gt, mv = (torch.from_numpy(a) for a in eval_util.planar_batch(c))
        fm.update(torch.from_numpy(c["pred"]), gt, torch.from_numpy(c["sizes"]), mv)
        per_sample.append(golden[f"{name}_sample7"])
    assert isinstance(fm.total, torch.Tensor) and isinstance(fm.count, torch.Tensor) and float(fm.count) == 3
    out = fm.compute()
    assert tuple(out) == eval_util.NAMES
    np.testing.assert_allclose(list(out.values()), np.concatenate(per_sample).mean(axis=0), **TOL)
    fm.reset()
    assert all(np.isnan(v) for v in fm.compute().values())
    with pytest.raises(ValueError, match="leading"):
        FlowMetrics(("EPE_noc",))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _metrics_worker(rank, world, port, out_dir):
    sys.path.insert(0, str(REPO))
    sys.path.insert(0, str(REPO / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from unsamflow_amd.evaluate import FlowMetrics

    c = eval_util.case("multi_block")
    gt, mv = (torch.from_numpy(a) for a in eval_util.planar_batch(c))
    pred, sizes = torch.from_numpy(c["pred"]), torch.from_numpy(c["sizes"])
    half = slice(rank, rank + 1)  # this rank's half of the batch of two
    fm = FlowMetrics("kitti_move")
    fm.update(pred[half], gt[half], sizes[half], mv[half])
    local = fm.compute()
    fm.all_reduce()
    torch.save({"local": local, "reduced": fm.compute(), "count": float(fm.count)},
               os.path.join(out_dir, f"metrics{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_flow_metrics_all_reduce_two_ranks_gloo(tmp_path):
    """Two ranks with one half of a batch each, all-reduced, equal one rank
    over the whole batch."""
    from unsamflow_amd.evaluate import FlowMetrics

    world = 2
    mp.spawn(_metrics_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(tmp_path / "metrics0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "metrics1.pt", weights_only=True)
    c = eval_util.case("multi_block")
    gt, mv = (torch.from_numpy(a) for a in eval_util.planar_batch(c))
    whole = FlowMetrics("kitti_move")
    whole.update(torch.from_numpy(c["pred"]), gt, torch.from_numpy(c["sizes"]), mv)
    want = whole.compute()
    assert r0["count"] == r1["count"] == 2.0
    assert r0["reduced"] == r1["reduced"] and r0["local"] != r1["local"]
    for k, v in want.items():
        assert r0["reduced"][k] == pytest.approx(v, rel=1e-12), k


# --------------------------------------------------------------- Validator --
class _StandIn(torch.nn.Module):
    """Returns a fixed prediction in PWCLite's result layout and records the mode it ran in."""

    def __init__(self, pred):
        super().__init__()
        self.pred, self.modes = pred, []

    def forward(self, img1, img2, full_seg1=None, full_seg2=None, with_bk=True):
        assert with_bk is False and not torch.is_grad_enabled()
        self.modes.append(self.training)
        return {"flows_12": [self.pred, self.pred[:, :, ::2, ::2]]}


@pytest.mark.parametrize("kind", ["kitti", "sintel"])
def test_validator_feeds_the_first_flow_and_restores_the_mode(kind):
    from unsamflow_amd.evaluate import flow_errors
    from unsamflow_amd.harness import Validator

    c = eval_util.case("ragged_small")
    gt, _ = (torch.from_numpy(a) for a in eval_util.planar_batch(c, fill=0.0))
    pred, sizes = torch.from_numpy(c["pred"]), torch.from_numpy(c["sizes"])
    model = _StandIn(pred)
    model.train()
    v = Validator(model, metrics=kind)
    img = torch.zeros(c["B"], 3, 8, 16)
    if kind == "kitti":
        v.update(img, img, gt, sizes)
        want, _ = flow_errors(pred, gt, sizes)
        n = 5
    else:
        occ = 1 - gt[:, 3:4]
        v.update(img, img, gt[:, :2], sizes, occ=occ)
        want, _ = flow_errors(pred, torch.cat([gt[:, :2], torch.ones_like(occ), 1 - occ], 1), sizes)
        n = 3
    assert model.modes == [False] and model.training  # ran in eval mode, train mode restored
    out = v.compute()
    assert tuple(out) == eval_util.NAMES[:n]
    np.testing.assert_allclose(list(out.values()), want.double().mean(dim=0)[:n].numpy(), rtol=1e-12)
    model.eval()
    v.update(img, img, gt if kind == "kitti" else gt[:, :2], sizes, occ=None if kind == "kitti" else occ)
    assert not model.training  # an eval-mode model stays in eval mode


def test_synthetic_flow_gt():
    from unsamflow_amd.harness import synthetic_flow_gt

    sizes = [(37, 122), (36, 120), (37, 124)]
    gt, table = synthetic_flow_gt(3, sizes, "cpu", seed=5)
    again, _ = synthetic_flow_gt(3, sizes, "cpu", seed=5)
    assert gt.shape == (3, 4, 37, 124) and torch.equal(gt, again)
    assert table.dtype == torch.int32 and table.tolist() == [list(s) for s in sizes]
    for b, (h, w) in enumerate(sizes):
        valid, noc = gt[b, 2, :h, :w], gt[b, 3, :h, :w]
        assert 0.5 < float(valid.mean()) < 0.7 and bool((noc <= valid).all()) and 0.6 < float(noc.sum() / valid.sum()) < 0.9
        assert float(gt[b, :, h:].abs().sum()) == 0.0 and float(gt[b, :, :, w:].abs().sum()) == 0.0
