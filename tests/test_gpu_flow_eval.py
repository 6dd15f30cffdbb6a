"""Validation on the GPU (unsamflow_amd/csrc/eval.hip) against the reference
capture (tests/golden/flow_eval.npz): the fused resize + EPE / Fl kernels
through flow_errors and the evaluate_flow drop-in, the resize kernel,
determinism, bad sizes, a guard-band run of both C entry points, the Validator.

Tolerances as tests/test_flow_eval_cpu.py: EPE numbers and the resized flow
atol = rtol = 1e-5 against the capture, bad-pixel counts exactly the recorded
fp64 counts, Fl rates rtol 1e-5."""
import numpy as np
import pytest
import torch

import eval_util
from conftest import load_golden
from eval_util import check_counts, check_metrics
from guard_util import Arena

pytestmark = pytest.mark.gpu
CASES = list(eval_util.CASES)


@pytest.fixture(scope="module")
def golden():
    return load_golden("flow_eval.npz")


def device_case(name, dev, channels=4):
    """(pred, gt, sizes, move) of a case on the device; the padding holds NaN."""
    c = eval_util.case(name)
    gt, mv = eval_util.planar_batch(c, channels=channels)
    return (torch.from_numpy(c["pred"]).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(c["sizes"]).to(dev),
            torch.from_numpy(mv).to(dev))


# ------------------------------------------------------------- the metrics --
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("move", [True, False])
def test_flow_errors_match_the_reference_capture(hip_device, golden, name, move):
    from unsamflow_amd import ops
    from unsamflow_amd.evaluate import flow_errors

    pred, gt, sizes, mv = device_case(name, hip_device)
    metrics, sums = flow_errors(pred, gt, sizes, mv if move else None)
    assert metrics.shape == (pred.shape[0], 7) and sums.shape == (pred.shape[0], 12)
    assert metrics.device == pred.device and metrics.dtype == torch.float32
    check_metrics(metrics.cpu().numpy(), golden, name, move=move)
    check_counts(sums.cpu().numpy(), golden, name)
    if not move:
        assert float(sums[:, 6:10].abs().max()) == 0.0
    assert ops.device_errors(hip_device) == 0


@pytest.mark.parametrize("name", CASES)
def test_two_channel_ground_truth(hip_device, golden, name):
    from unsamflow_amd.evaluate import flow_errors

    pred, gt, sizes, _ = device_case(name, hip_device, channels=2)
    metrics, sums = flow_errors(pred, gt, sizes)
    check_metrics(metrics.cpu().numpy(), golden, name, channels=2)
    area = eval_util.case(name)["sizes"].prod(axis=1)
    s = sums.cpu().numpy()
    assert np.array_equal(s[:, 1], area) and np.array_equal(s[:, 3], area) and np.abs(s[:, 4:6]).max() == 0.0


@pytest.mark.parametrize("name", CASES)
def test_prediction_as_a_channel_slice(hip_device, golden, name):
    """pred = x[:, :2] of a [B,4,h,w] tensor (how the step keeps its flows) is used in place."""
    from unsamflow_amd.evaluate import flow_errors

    pred, gt, sizes, mv = device_case(name, hip_device)
    both = torch.cat([pred, torch.full_like(pred, float("nan"))], dim=1)
    want = flow_errors(pred, gt, sizes, mv)
    got = flow_errors(both[:, :2], gt, sizes, mv)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    check_metrics(got[0].cpu().numpy(), golden, name)
    # the upper half of the channels: a slice that starts inside the allocation
    got = flow_errors(torch.cat([torch.full_like(pred, float("nan")), pred], dim=1)[:, 2:], gt, sizes, mv)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("name", CASES)
def test_evaluate_flow_drop_in(hip_device, golden, name):
    from unsamflow_amd.evaluate import evaluate_flow

    c = eval_util.case(name)
    pred = np.ascontiguousarray(c["pred"].transpose(0, 2, 3, 1))
    r7 = evaluate_flow(c["gts"], pred, c["moves"], device=hip_device)
    r5 = evaluate_flow(c["gts"], pred)  # the default device: the ROCm device when one is present
    r1 = evaluate_flow([g[..., :2] for g in c["gts"]], pred, device=hip_device)
    assert [len(r7), len(r5), len(r1)] == [7, 5, 1] and all(isinstance(v, float) for v in r7 + r5 + r1)
    np.testing.assert_allclose(r7, golden[f"{name}_ret7"], **eval_util.TOL)
    np.testing.assert_allclose(r5, golden[f"{name}_ret5"], **eval_util.TOL)
    np.testing.assert_allclose(r1, golden[f"{name}_ret1"], **eval_util.TOL)
    assert r5 == r7[:5]


@pytest.mark.parametrize("name", CASES)
def test_two_runs_are_bit_identical(hip_device, name):
    from unsamflow_amd.evaluate import flow_errors

    pred, gt, sizes, mv = device_case(name, hip_device)
    a = flow_errors(pred, gt, sizes, mv)
    b = flow_errors(pred.clone(), gt.clone(), sizes.clone(), mv.clone())
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_null_size_table_means_the_whole_plane(hip_device, golden):
    from unsamflow_amd.evaluate import flow_errors

    pred, gt, sizes, mv = device_case("identity", hip_device)
    a, b = flow_errors(pred, gt, None, mv), flow_errors(pred, gt, sizes, mv)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    check_metrics(a[0].cpu().numpy(), golden, "identity")


# -------------------------------------------------------------- the resize --
@pytest.mark.parametrize("name", eval_util.SMALL)
def test_resize_flow_matches_the_stored_flows(hip_device, golden, name):
    from unsamflow_amd.evaluate import resize_flow

    c = eval_util.case(name)
    pred = torch.from_numpy(c["pred"]).to(hip_device)
    Hmax, Wmax = (int(v) for v in c["sizes"].max(axis=0))
    table = resize_flow(pred, (Hmax, Wmax), sizes=torch.from_numpy(c["sizes"])).cpu()
    for b, (H, W) in enumerate(c["sizes"]):
        want = golden[f"{name}_resized_{b}"]
        single = resize_flow(pred[b:b + 1], (int(H), int(W)))
        assert single.shape == (1, 2, H, W) and single.device == pred.device
        np.testing.assert_allclose(single[0].cpu().numpy(), want, **eval_util.TOL)
        np.testing.assert_allclose(table[b, :, :H, :W].numpy(), want, **eval_util.TOL)
        assert float(table[b, :, H:].abs().sum()) == 0.0 and float(table[b, :, :, W:].abs().sum()) == 0.0


@pytest.mark.parametrize("shape", [(70, 150), (375, 1242)])
def test_resize_flow_matches_the_composition(hip_device, shape):
    """Both group widths (Hmax Wmax % 4 == 0 and not) at sizes with many workgroups."""
    from unsamflow_amd.evaluate import resize_flow, resize_flow_torch

    name = "multi_block" if shape == (70, 150) else "kitti_like"
    pred = torch.from_numpy(eval_util.case(name)["pred"])
    got = resize_flow(pred.to(hip_device), shape).cpu()
    torch.testing.assert_close(got, resize_flow_torch(pred, shape), **eval_util.TOL)


# --------------------------------------------------------------- bad sizes --
def test_bad_size_skips_its_sample_and_raises_the_flag(hip_device):
    from unsamflow_amd import _lib, ops
    from unsamflow_amd.evaluate import flow_errors

    pred, gt, sizes, mv = device_case("ragged_small", hip_device)
    ops.device_errors(hip_device)
    want = flow_errors(pred, gt, sizes, mv)
    assert ops.device_errors(hip_device) == 0
    for bad in ([12, 23], [11, 24], [1, 23], [11, 0], [-5, 7], [2 ** 31 - 1, 2 ** 31 - 1]):
        table = sizes.clone()
        table[0] = torch.tensor(bad, dtype=torch.int32)
        metrics, sums = flow_errors(pred, gt, table, mv)
        assert bool(torch.isnan(metrics[0]).all()) and float(sums[0].abs().max()) == 0.0, bad
        assert torch.equal(metrics[1], want[0][1]) and torch.equal(sums[1], want[1][1]), bad
        assert ops.device_errors(hip_device, clear=False) == _lib.DEVERR_EVAL_BAD_SIZE
        assert ops.device_errors(hip_device) == _lib.DEVERR_EVAL_BAD_SIZE and ops.device_errors(hip_device) == 0
    # the resize leaves the skipped sample's planes untouched
    table = sizes.clone()
    table[1] = torch.tensor([9, 24], dtype=torch.int32)
    out = torch.full((2, 2, 11, 23), 1000.0, device=hip_device)
    ops.flow_resize(pred, table, 11, 23, out=out)
    assert float((out[1] - 1000.0).abs().max()) == 0.0 and float(out[0].abs().max()) < 100.0
    assert ops.device_errors(hip_device) == _lib.DEVERR_EVAL_BAD_SIZE and ops.device_errors(hip_device) == 0


# -------------------------------------------------------------- guard band --
def test_guard_band_run_of_both_entry_points(hip_device, golden):
    """Both C entry points at ragged_small with every buffer inside one
    poison-filled arena: no guard word damaged, every metric and sum written,
    the resize output's padding still poison; the prediction and the size table
    on 4-byte (not 16-byte) boundaries, as their contract allows."""
    from unsamflow_amd import _lib

    name = "ragged_small"
    c = eval_util.case(name)
    B, (h, w) = c["B"], c["hw"]
    Hmax, Wmax = (int(v) for v in c["sizes"].max(axis=0))
    gt_np, mv_np = eval_util.planar_batch(c)
    lib = _lib.load()
    a = Arena(hip_device)
    pred = a.place((B, 2, h, w), fill=c["pred"], name="pred", misalign=1)
    sizes = a.place((B, 2), dtype=torch.int32, fill=c["sizes"], name="sizes", misalign=3)
    gt = a.place((B, 4, Hmax, Wmax), fill=gt_np, name="gt")
    move = a.place((B, 1, Hmax, Wmax), fill=mv_np, name="move")
    npart = lib.usf_flow_eval_partials(B, Hmax, Wmax)
    partials = a.place((npart,), name="partials")
    sums = a.place((B, _lib.EVAL_NACC), name="sums")
    metrics = a.place((B, _lib.EVAL_NMETRIC), name="metrics")
    out = a.place((B, 2, Hmax, Wmax), name="out")
    assert pred.data_ptr() % 16 == 4 and sizes.data_ptr() % 16 == 12
    stream = _lib.stream_handle(hip_device)
    with torch.cuda.device(hip_device):
        rc = lib.usf_flow_eval_f32(pred.data_ptr(), 2 * h * w, gt.data_ptr(), 4, move.data_ptr(), sizes.data_ptr(),
                                   partials.data_ptr(), sums.data_ptr(), metrics.data_ptr(), B, h, w, Hmax, Wmax,
                                   stream)
        _lib.check(rc, "usf_flow_eval_f32")
        rc = lib.usf_flow_resize_f32(pred.data_ptr(), 2 * h * w, sizes.data_ptr(), out.data_ptr(), B, h, w, Hmax,
                                     Wmax, stream)
        _lib.check(rc, "usf_flow_resize_f32")
    torch.cuda.synchronize(hip_device)
    a.check()
    assert a.poisoned(metrics) == 0 and a.poisoned(sums) == 0 and a.poisoned(partials) == 0
    check_metrics(metrics.cpu().numpy(), golden, name)
    check_counts(sums.cpu().numpy(), golden, name)
    inside = 0
    for b, (H, W) in enumerate(c["sizes"]):
        H, W = int(H), int(W)
        assert a.poisoned(out[b, :, :H, :W]) == 0
        np.testing.assert_allclose(out[b, :, :H, :W].cpu().numpy(), golden[f"{name}_resized_{b}"], **eval_util.TOL)
        inside += 2 * H * W
    assert a.poisoned(out) == out.numel() - inside  # the padding still holds the pattern


# ------------------------------------------------------------- FlowMetrics --
def test_flow_metrics_update_does_not_synchronise(hip_device, golden):
    """Two updates under torch's sync debug mode (a device-to-host read or a
    stream sync would raise); compute() afterwards is the one sync and gives
    the mean over the three samples."""
    from unsamflow_amd.evaluate import FlowMetrics

    batches = [device_case(n, hip_device) for n in ("ragged_small", "identity")]
    fm = FlowMetrics("kitti_move")
    fm.update(*batches[0])  # warm-up: library load, allocator, the scratch's first use
    fm.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for pred, gt, sizes, mv in batches:
            fm.update(pred, gt, sizes, mv)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out = fm.compute()
    want = np.concatenate([golden["ragged_small_sample7"], golden["identity_sample7"]]).mean(axis=0)
    assert tuple(out) == eval_util.NAMES and fm.total.device == batches[0][0].device
    np.testing.assert_allclose(list(out.values()), want, **eval_util.TOL)


# --------------------------------------------------------------- Validator --
def test_validator_on_a_tiny_pwclite(hip_device):
    from oracle.hashrng import hash_init_
    from unsamflow_amd.config import AttrDict, kitti_base
    from unsamflow_amd.evaluate import flow_errors
    from unsamflow_amd.harness import Validator, synthetic_flow_gt, synthetic_pair
    from unsamflow_amd.pwclite import PWCLite

    model = PWCLite(AttrDict.wrap(dict(kitti_base().model))).to(hip_device)
    hash_init_(model, seed=1)
    model.train()
    img1, img2, _, _ = synthetic_pair(2, 64, 128, hip_device, seed=3)
    gt, sizes = synthetic_flow_gt(2, [(75, 150), (70, 141)], hip_device, seed=4)
    model.eval()
    with torch.no_grad():
        by_hand = model(img1, img2, with_bk=False)["flows_12"][0]
    model.train()
    want, _ = flow_errors(by_hand, gt, sizes)

    v = Validator(model, metrics="kitti")
    pred = v.update(img1, img2, gt, sizes)
    assert model.training and not pred.requires_grad and pred.shape == by_hand.shape
    out = v.compute()
    assert tuple(out) == eval_util.NAMES[:5] and all(np.isfinite(list(out.values())))
    # the validator's numbers are flow_errors' on the prediction it made ...
    mine, _ = flow_errors(pred, gt, sizes)
    np.testing.assert_allclose(list(out.values()), mine.double().mean(dim=0)[:5].cpu().numpy(), rtol=1e-12)
    # ... and that prediction is the one taken by hand (the same kernels on the same inputs)
    torch.testing.assert_close(pred, by_hand, atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(list(out.values())[:3], want.double().mean(dim=0)[:3].cpu().numpy(), rtol=1e-4)
