"""The homography smoothness kernels (csrc/hg.hip) on the device.

Selection is exact against numpy. The fit is this project's own RANSAC, so it is
tested by recovery: on a planted scene whose margins (0.03 px of noise and 5 px
of displacement against thr = 0.5) make the outcome a condition, the final
inlier set of every accepted segment is the planted one, and H acts as the fp64
numpy refit on the inliers of the winning hypothesis to 1e-3 px over the whole
image. The loss of given records is compared with the torch composition:

    forward   |gpu - fp64| <= 4 e_ref,  e_ref = max(|cpu_fp32 - fp64|, half an fp32 ulp of the loss)
              (the project's factor 4; the floor is the format's: the kernel's result is an fp32 number)
    backward  equal to -sign(diff_fp64) / (h w B) at every pixel with |diff_fp64| >= 1e-4 (at most 1 % of
              the refined pixels may fall below, asserted), exactly 0 outside the accepted segments

Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest
import torch

import hg_util as hu
from conftest import load_golden

pytestmark = pytest.mark.gpu

THR = 0.5


@pytest.fixture(scope="module")
def scene():
    return hu.planted_scene()


@pytest.fixture(scope="module")
def scene_records(hip_device, scene):
    """The planted scene fitted once on the device, with seed 0 -> records on the CPU."""
    from unsamflow_amd.homography import fit_homographies

    flow, seg, occ, K, _ = scene
    d = hip_device
    return fit_homographies(flow.to(d), seg.to(d), occ.to(d), THR, K).cpu()


def _f32_half_ulp(x):
    return 0.5 * float(np.spacing(np.float32(abs(x))))


# -------------------------------------------------------------- selection --
def _selection_case(shape):
    B, h, w = shape
    g = torch.Generator().manual_seed(100 + h)
    if shape == (2, 24, 40):
        _, seg, occ = hu.golden_inputs("b2_24x40")
        return seg, occ, 9
    K = 3 if shape == (1, 5, 7) else 12
    blk = 2 if h < 10 else 3
    ids = torch.randint(0, K, (B, 1, (h + blk - 1) // blk, (w + blk - 1) // blk), generator=g).float()
    seg = ids.repeat_interleave(blk, 2).repeat_interleave(blk, 3)[:, :, :h, :w].contiguous()
    if K == 12:
        seg[seg == 7] = 8.0   # an id present in no pixel
        seg[1] = 5.0          # a sample that is one segment
    occ = (torch.rand((B, 1, h, w), generator=g) < 0.45).float()
    return seg, occ, K


@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 24, 40), (2, 33, 47)])
def test_selection_is_exact(hip_device, shape):
    from unsamflow_amd.homography import fit_homographies

    B, h, w = shape
    seg, occ, K = _selection_case(shape)
    flow = torch.from_numpy(hu.hashrng.symmetric((B, 2, h, w), 77, 1.0))
    d = hip_device
    rec = fit_homographies(flow.to(d), seg.to(d), occ.to(d), THR, K, n_hyp=32).cpu().numpy()
    for b, (cnt, ids, st) in enumerate(hu.select_np(seg.numpy(), occ.numpy(), K)):
        assert rec[b, :, 0].tolist() == ids, (b, rec[b, :, 0].tolist(), ids)
        for s, k in enumerate(ids):
            if k < 0:
                assert rec[b, s, 1] == hu.EMPTY
                continue
            assert (rec[b, s, 2], rec[b, s, 3]) == (cnt[0, k], cnt[2, k]), (b, s, k)
            if st[s] >= 0:
                assert rec[b, s, 1] == st[s], (b, s, k, rec[b, s, 1], st[s])
            else:
                assert rec[b, s, 1] in (hu.ACCEPTED, hu.LOW_INLIER, hu.DEGENERATE), (b, s, k, rec[b, s, 1])
    if shape == (2, 33, 47):
        assert rec[1, 0, 0] in (1, 5) and (seg == 7).sum() == 0


# --------------------------------------------------------------- recovery --
def _check_recovery(scene, rec, label):
    from unsamflow_amd import homography as hg

    flow, seg, occ, K, planted = scene
    H = hg.records_H(rec).numpy()
    rec = rec.numpy()
    px = hu.all_pixels(64, 96)
    worst, seen = 0.0, set()
    for b in range(2):
        for s in range(6):
            k = int(rec[b, s, 0])
            want = planted[(b, k)]
            seen.add(want["kind"])
            p1, p2 = hu.slot_pairs(flow, seg, occ, b, k)
            assert rec[b, s, 3] == len(p1)
            if want["kind"] == "outliers":
                assert rec[b, s, 1] == hu.LOW_INLIER, (b, k, rec[b, s, 1])
                continue
            assert rec[b, s, 1] == hu.ACCEPTED, (b, k, rec[b, s, 1])
            assert rec[b, s, 4] == want["inliers"].sum(), (b, k, rec[b, s, 4])
            assert np.array_equal(hg.inliers_np(H[b, s], p1, p2, THR), want["inliers"]), (b, k)
            Hs, valid = hg.hypotheses_np(p1, p2, b, s, seed=label)
            j = int(rec[b, s, 14])
            assert 0 <= j < 256 and valid[j]
            inl0 = hg.inliers_np(Hs[j], p1, p2, THR)
            H_ref = hg.refit_homography_np(p1[inl0], p2[inl0])
            if want["kind"] == "block":
                # four points 1 px apart fix a homography whose denominator crosses zero inside the image
                # (tests/test_hg_cpu.py): its action is compared on the block's own pixels
                assert rec[b, s, 4] == 4
                at = p1.astype(np.float64)
            else:
                at = px
            err = float(np.abs(hu.apply_h(H[b, s], at) - hu.apply_h(H_ref, at)).max())
            print(f"[hg] seed {label} sample {b} id {k} ({want['kind']}): n_inl={rec[b, s, 4]} best_j={j} "
                  f"max|H p - H_ref p|={err:.3e} px")
            worst = max(worst, err)
    assert seen == {"plane", "outliers", "block"}
    print(f"[hg] seed {label}: max |H_gpu p - H_ref p| = {worst:.3e} px")
    assert worst <= 1e-3
    return worst


def test_recovery_of_planted_homographies(scene, scene_records):
    _check_recovery(scene, scene_records, 0)


def test_fit_is_deterministic_and_seed_independent_on_the_planted_scene(hip_device, scene, scene_records):
    from unsamflow_amd.homography import fit_homographies

    flow, seg, occ, K, _ = scene
    d = hip_device
    again = fit_homographies(flow.to(d), seg.to(d), occ.to(d), THR, K).cpu()
    assert torch.equal(again, scene_records)  # bit-identical records
    other = fit_homographies(flow.to(d), seg.to(d), occ.to(d), THR, K, seed=12345).cpu()
    assert not torch.equal(other[..., 14], scene_records[..., 14])  # another stream, other winners
    assert torch.equal(other[..., :5], scene_records[..., :5])      # the same statuses and inlier counts
    _check_recovery(scene, other, 12345)                            # and the same (planted) inlier sets


# ------------------------------------------------- loss with given records --
def _given_case(shape, seed):
    """flow4 [B,4,h,w] (the loss reads its [:, 2:] slice), seg with ids 0..4 and records: ids 1 and 3
    accepted, id 2 rejected for its inlier share, id 4 degenerate (both carry an H that must not be used)."""
    B, h, w = shape
    flow4 = torch.from_numpy(hu.hashrng.symmetric((B, 4, h, w), seed, 2.0))
    ys, xs = np.mgrid[0:h, 0:w]
    seg = np.stack([((xs * 5) // w + b + (ys >= h // 2)) % 5 for b in range(B)])[:, None].astype(np.float32)
    entries = {}
    for b in range(B):
        for s, (k, status) in enumerate([(1, hu.ACCEPTED), (2, hu.LOW_INLIER), (3, hu.ACCEPTED), (4, hu.DEGENERATE)]):
            entries[(b, s)] = (k, status, hu.random_homography(seed + 10 * b + s, w / 2.0, h / 2.0))
    return flow4, torch.from_numpy(seg), hu.make_records(B, entries)


def _expected(flow, seg, rec):
    """fp64 numpy: (diff [B,2,h,w], refined [B,h,w]) of the accepted slots."""
    from unsamflow_amd.homography import records_H

    B, _, h, w = flow.shape
    H = records_H(rec).numpy().astype(np.float64)
    f, s, r = flow.numpy().astype(np.float64), seg.numpy()[:, 0], rec.numpy()
    diff, refined = np.zeros((B, 2, h, w)), np.zeros((B, h, w), dtype=bool)
    ys, xs = np.mgrid[0:h, 0:w]
    for b in range(B):
        for slot in range(6):
            if r[b, slot, 1] != hu.ACCEPTED:
                continue
            m = s[b] == r[b, slot, 0]
            p1 = np.stack([xs[m], ys[m]], 1).astype(np.float64)
            # pts2 is formed in fp32, as the reference and the kernel form it
            p2 = (p1.astype(np.float32) + np.stack([flow.numpy()[b, 0][m], flow.numpy()[b, 1][m]], 1)).astype(np.float64)
            d = hu.apply_h(H[b, slot], p1) - p2
            diff[b, 0][m], diff[b, 1][m] = d[:, 0], d[:, 1]
            refined[b] |= m
    return diff, refined


def _check_loss(name, loss, grad, flow, seg, rec, l_ref32=None, g_ref32=None):
    from unsamflow_amd.homography import homography_loss_torch

    B, _, h, w = flow.shape
    l64 = float(homography_loss_torch(flow.double(), seg, rec))
    if l_ref32 is None:
        l_ref32 = float(homography_loss_torch(flow.float(), seg, rec))
    e_ref = max(abs(l_ref32 - l64), _f32_half_ulp(l64))
    err = abs(float(loss) - l64)
    diff, refined = _expected(flow, seg, rec)
    small = (np.abs(diff) < 1e-4) & refined[:, None]
    want = (-np.sign(diff) * np.float32(1.0 / (h * w * B))).astype(np.float32)
    g = grad.cpu().numpy()
    keep = ~small
    wrong = int((g[keep] != want[keep]).sum())
    print(f"[hg] {name}: loss gpu={float(loss):.9g} fp64={l64:.9g} err={err:.3e} e_ref={e_ref:.3e} "
          f"refined={int(refined.sum())} excluded={int(small.any(1).sum())} wrong={wrong}")
    assert small.any(1).sum() <= 0.01 * max(int(refined.sum()), 1)  # checked on the CPU: the inputs stay under the cap
    assert err <= 4.0 * e_ref, (name, err, e_ref)
    assert wrong == 0
    assert np.abs(g[~np.broadcast_to(refined[:, None], g.shape)]).max(initial=0.0) == 0.0  # exactly zero outside
    if g_ref32 is not None:
        assert np.array_equal(g[keep], g_ref32[keep])


@pytest.mark.parametrize("shape,seed", [((1, 5, 7), 810), ((2, 33, 47), 820), ((2, 64, 96), 830)])
def test_loss_of_given_records(hip_device, shape, seed):
    from unsamflow_amd.homography import homography_loss

    flow4, seg, rec = _given_case(shape, seed)
    d = hip_device
    f4 = flow4.to(d).requires_grad_(True)
    loss = homography_loss(f4[:, 2:], seg.to(d), rec.to(d))
    loss.backward()
    assert float(f4.grad[:, :2].abs().max()) == 0.0  # the other half of the [B,4,h,w] tensor is untouched
    _check_loss(str(shape), loss.detach(), f4.grad[:, 2:], flow4[:, 2:], seg, rec)
    # ids 0, 2 (rejected) and 4 (degenerate) get exactly zero gradient
    for k in (0, 2, 4):
        m = (seg == k).expand(-1, 2, -1, -1)
        assert float(f4.grad[:, 2:].cpu()[m].abs().max()) == 0.0
    assert float(loss) > 0


def test_golden_records_give_the_references_loss(hip_device):
    """The H the reference's own run recorded, fed as records: the reference's loss and gradient."""
    from unsamflow_amd.homography import homography_loss

    golden = load_golden("hg_smooth.npz")
    d = hip_device
    for name, (B, h, w, K, _) in hu.GOLDEN_CASES.items():
        flow, seg, occ = hu.golden_inputs(name)
        calls = iter(zip(golden[f"{name}_call_sample"], golden[f"{name}_call_npts"], golden[f"{name}_call_H"]))
        entries = {}
        for b, (cnt, ids, st) in enumerate(hu.select_np(seg.numpy(), occ.numpy(), K)):
            for s, k in enumerate(ids):
                if k < 0 or st[s] >= 0:
                    continue
                sample, npts, H = next(calls)  # the estimator calls come in slot order
                assert (sample, npts) == (b, cnt[2, k])
                share = (hu.transfer_error(H, *hu.slot_pairs(flow, seg, occ, b, k)) <= THR).mean()
                entries[(b, s)] = (k, hu.ACCEPTED if share >= 0.5 else hu.LOW_INLIER, H)
        assert next(calls, None) is None
        rec = hu.make_records(B, entries)
        f = flow.to(d).requires_grad_(True)
        loss = homography_loss(f, seg.to(d), rec.to(d))
        loss.backward()
        _check_loss(f"golden {name}", loss.detach(), f.grad, flow, seg, rec, float(golden[f"{name}_loss"]),
                    golden[f"{name}_grad"])


# ------------------------------------------------------------- end to end --
def _loss_inputs(B=2, h=64, w=96):
    g = torch.Generator().manual_seed(3)
    f12, s1, o1, K, _ = hu.planted_scene(4100)
    f21, s2, o2, _, _ = hu.planted_scene(4300)
    top = torch.cat([f12, f21], 1)
    flows = [top] + [torch.zeros(B, 4, h >> i, w >> i) for i in range(1, 5)]
    return flows, torch.rand(B, 3, h, w, generator=g), torch.rand(B, 3, h, w, generator=g), (s1, s2), (o1, o2), K


def _smooth_bound(name, l_fused, l_comp32, flows, segs, viss, thr):
    """l_sm of the fused path against the composition's, under the forward bound of the module docstring:
    the fp64 value is the composition's records' loss in fp64."""
    from unsamflow_amd.homography import fit_homographies_torch, homography_loss_torch

    top = flows[0].detach().cpu()
    l64 = 0.0
    for fl, sg, vis in zip((top[:, :2], top[:, 2:]), segs, viss):
        rec = fit_homographies_torch(fl, sg.cpu(), 1 - vis.cpu(), thr)
        l64 += float(homography_loss_torch(fl.double(), sg.cpu(), rec)) / 2.0
    e_ref = max(abs(l_comp32 - l64), _f32_half_ulp(l64))
    err = abs(l_fused - l64)
    print(f"[hg] {name}: l_sm fused={l_fused:.9g} composition={l_comp32:.9g} fp64={l64:.9g} err={err:.3e} "
          f"e_ref={e_ref:.3e}")
    assert err <= 4.0 * e_ref, (name, err, e_ref)


def test_unflowloss_fused_against_the_host_loop(hip_device):
    from unsamflow_amd.config import kitti_stage2_hg
    from unsamflow_amd.flow_loss import unFlowLoss
    from unsamflow_amd.homography import fit_homographies, fit_homographies_torch

    d = hip_device
    flows, im1, im2, segs, occs, K = _loss_inputs()
    flows = [f.to(d) for f in flows]
    segs, occs = [s.to(d) for s in segs], [o.to(d) for o in occs]
    occ_fn = lambda a, b: occs[0] if a.storage_offset() == 0 else occs[1]  # noqa: E731 (the scene's masks)
    out = {}
    for fused in (True, False):
        loss_fn = unFlowLoss(kitti_stage2_hg().loss, occ_bidir_fn=occ_fn, fused_homography=fused)
        flows[0] = flows[0].detach().requires_grad_(True)
        loss, _, l_sm, _, vis1, vis2 = loss_fn(flows, im1.to(d), im2.to(d), full_seg1=segs[0], full_seg2=segs[1])
        loss.sum().backward()
        assert torch.isfinite(flows[0].grad).all()
        out[fused] = float(l_sm.detach())
    assert out[True] > 0
    top = flows[0].detach()
    for fl, sg, oc in zip((top[:, :2], top[:, 2:]), segs, occs):
        a = fit_homographies(fl, sg, oc, THR, K).cpu()
        b = fit_homographies_torch(fl.cpu(), sg.cpu(), oc.cpu(), THR, K)
        assert torch.equal(a[..., :5], b[..., :5])  # ids, statuses, counts and inlier counts
    _smooth_bound("planted scene", out[True], out[False], flows, segs, (vis1, vis2), THR)


# ---------------------------------------------------------- graph capture --
def test_fit_and_loss_replay_from_a_graph(hip_device, scene):
    """Fit + loss forward + backward captured with num_segments given: no host sync anywhere on the path,
    and after the flow changes in place the replay equals the eager result bit for bit."""
    from unsamflow_amd import ops

    flow, seg, occ, K, _ = scene
    d = hip_device
    flow4 = torch.cat([flow, flow.flip(0)], 1).to(d)
    sg, oc = seg.to(d), occ.to(d)
    one = torch.ones(1, device=d)

    def fn():
        rec = ops.hg_fit(flow4[:, 2:], sg, oc, K, THR)
        return rec, ops.hg_loss_forward(flow4[:, 2:], sg, rec), ops.hg_loss_backward(flow4[:, 2:], sg, rec, one)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    first = [t.clone() for t in fn()]
    noise = torch.from_numpy(hu.hashrng.symmetric(tuple(flow4.shape), 991, 0.01)).to(d)
    flow4.add_(noise)
    graph.replay()
    torch.cuda.synchronize()
    eager = fn()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    assert not torch.equal(first[2], eager[2]) or not torch.equal(first[0], eager[0])  # the inputs did change
    assert float(eager[1]) > 0


# ---------------------------------------------------------------- bad ids --
def test_bad_ids_are_ignored_and_flagged(hip_device, scene):
    from unsamflow_amd import _lib, ops
    from unsamflow_amd.homography import fit_homographies, homography_loss

    flow, seg, occ, K, _ = scene
    d = hip_device
    bad = seg.clone()
    bad[0, 0, 0, 0:3] = torch.tensor([float(K), -1.0, 2.5])  # an id >= K, a negative id, a non-integer id (id 0 pixels)
    bad[1, 0, 5, 5] = 1e9                                    # inside segment 1 of sample 1
    ops.device_errors(d)
    rec = fit_homographies(flow.to(d), bad.to(d), occ.to(d), THR, K)
    assert ops.device_errors(d, clear=False) == _lib.DEVERR_HG_BAD_ID
    assert ops.device_errors(d) == _lib.DEVERR_HG_BAD_ID
    assert ops.device_errors(d) == 0
    rec = rec.cpu().numpy()
    for b, (cnt, ids, st) in enumerate(hu.select_np(bad.numpy(), occ.numpy(), K)):
        assert rec[b, :, 0].tolist() == ids
        assert rec[b, :, 2].tolist() == [cnt[0, k] for k in ids] and rec[b, :, 3].tolist() == [cnt[2, k] for k in ids]
    assert rec[1, :, 2][rec[1, :, 0] == 1] == 783  # the pixel with the bad id left its segment
    f = flow.to(d).requires_grad_(True)
    homography_loss(f, bad.to(d), torch.from_numpy(rec).to(d)).backward()
    assert float(f.grad[1, :, 5, 5].abs().max()) == 0.0 and float(f.grad[0, :, 0, 0:3].abs().max()) == 0.0
    assert ops.device_errors(d) == 0  # the loss kernels match ids, they index nothing with them


# -------------------------------------------------------------- one step --
def test_one_stage2_train_step(hip_device):
    """One whole step runs and l_sm equals the host loop's on the same flows. The flows of an untrained
    model fail the bidirectional check almost everywhere, so every slot is dropped for its reliable count
    and l_sm is 0 on both paths (printed). The comparison is therefore repeated on the same flows at 1/50
    of their size, which pass the check: segments are fitted and l_sm is not zero."""
    from unsamflow_amd.config import kitti_stage2_hg
    from unsamflow_amd.flow_loss import unFlowLoss
    from unsamflow_amd.harness import TrainStep, synthetic_pair

    d = hip_device
    cfg = kitti_stage2_hg()
    cfg.train.ot_size = [64, 128]  # the config's 192x640 crop of the third pass is larger than this image
    step = TrainStep(cfg, d)
    im1, im2, s1, s2 = synthetic_pair(1, 64, 128, d, with_seg=True, n_seg=8)
    loss = step(im1, im2, s1, s2)
    assert torch.isfinite(loss)
    with torch.no_grad():
        _, flows = step.forward_loss(im1, im2, s1, s2)
        _, _, l_sm, _, vis1, vis2 = step.loss_fn(flows, im1, im2, full_seg1=s1, full_seg2=s2)
        comp = unFlowLoss(kitti_stage2_hg().loss, fused_homography=False)
        _, _, l_comp, _, _, _ = comp(flows, im1, im2, full_seg1=s1, full_seg2=s2)
    assert torch.isfinite(l_sm)
    from unsamflow_amd.homography import fit_homographies

    for fl, sg, vis in zip((flows[0][:, :2], flows[0][:, 2:]), (s1, s2), (vis1, vis2)):
        a = fit_homographies(fl, sg, 1 - vis, cfg.loss.ransac_threshold)
        b = fit_homographies(fl, sg, 1 - vis, cfg.loss.ransac_threshold, fused=False)
        print(f"[hg] TrainStep statuses fused={a[0, :, 1].tolist()} host loop={b[0, :, 1].tolist()}")
        assert torch.equal(a[..., [0, 2, 3]], b[..., [0, 2, 3]].to(a.device))  # the selection: ids and counts
    _smooth_bound("TrainStep", float(l_sm), float(l_comp), flows, (s1, s2), (vis1, vis2), cfg.loss.ransac_threshold)
    # the same flows at 1/50 of their size pass the check, so segments are fitted and l_sm is not zero
    small = [f * 0.02 for f in flows]
    with torch.no_grad():
        _, _, l_sm, _, vis1, vis2 = step.loss_fn(small, im1, im2, full_seg1=s1, full_seg2=s2)
        _, _, l_comp, _, _, _ = comp(small, im1, im2, full_seg1=s1, full_seg2=s2)
    assert float(l_sm) > 0
    _smooth_bound("TrainStep, flows / 50", float(l_sm), float(l_comp), small, (s1, s2), (vis1, vis2),
                  cfg.loss.ransac_threshold)
