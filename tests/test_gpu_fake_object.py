"""The fused key-object augmentation (unsamflow_amd.fake_object,
csrc/fakeobj.hip) on the GPU against the torch composition of the same formulas
evaluated on the CPU in fp32 and again in fp64 on the same inputs.

Paste + crop: the project's 4x rule (tests/test_gpu_ar.py), per output tensor:
    e_ref = max|cpu_fp32 - fp64|,   max|gpu - fp64| <= max(4 e_ref, 2^-23 max|fp64|)
(the factor 4 covers another rounding of the same fp32 quantities; the floor is
one ulp, for tensors where the composition is exact). noc_ot must be bit-equal.

Push: the copies bit for bit; the motion against the fp64 masked mean under the
same rule with the CPU fp32 sum / sum as e_ref (the flow has one sign inside the
mask, so nothing cancels); two runs bit-equal.

Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest
import torch

import fakeobj_util
from oracle import hashrng

pytestmark = pytest.mark.gpu

TENSORS = ["imgs_ot", "flow_ot", "noc_ot"]
SHAPES = [(1, 2, 3), (2, 13, 21), (3, 33, 70), (2, 64, 96)]
# an interior window with odd y0, x0 and an odd width: (ch, cw), (y0, x0)
INTERIOR = {(1, 2, 3): ((1, 1), (1, 1)), (2, 13, 21): ((7, 9), (3, 5)), (3, 33, 70): ((20, 37), (5, 11)),
            (2, 64, 96): ((40, 71), (7, 13))}


def _setup(B, H, W, K):
    """Base tensors, K*B objects in slots 0..K*B-1 (every odd one mirrored) and their host tables."""
    n = K * B
    base = fakeobj_util.base(B, H, W, 700 + H + W)
    objs = fakeobj_util.objects(n, H, W, 800 + H + W)
    slots = torch.arange(n, dtype=torch.int32)
    params = fakeobj_util.plain_params(n, flips=range(1, n, 2))
    return base, objs, slots, params


@pytest.fixture(scope="module")
def paste_refs():
    """Per (shape, K): inputs and the full-size CPU fp32 / fp64 compositions (computed once, never modified)."""
    from unsamflow_amd import fake_object as fo

    refs = {}
    for B, H, W in SHAPES:
        for K in (1, 3):
            base, objs, slots, params = _setup(B, H, W, K)
            cache = fakeobj_util.filled_cache(*objs)
            o32 = fo.paste_and_crop(*base, cache, slots, params, (H, W), (0, 0))
            o64 = fo.paste_and_crop(*[t.double() for t in base], cache, slots, params, (H, W), (0, 0))
            refs[(B, H, W, K)] = (base, objs, slots, params, o32, o64)
    return refs


def _check(name, outs, o32, o64, win):
    for k, g, a, b in zip(TENSORS, outs, o32, o64):
        a, b = a[win], b[win]
        e_ref = float((a.double() - b).abs().max())
        err = float((g.cpu().double() - b).abs().max())
        floor = 2.0 ** -23 * float(b.abs().max())
        print(f"[fakeobj] {name} {k}: err={err:.3e} e_ref={e_ref:.3e} max|ref|={float(b.abs().max()):.3e}")
        assert tuple(g.shape) == tuple(b.shape) and g.is_contiguous()
        assert err <= max(4.0 * e_ref, floor), (name, k, err, e_ref)
        if k == "noc_ot":
            assert torch.equal(g.cpu(), a), name


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_paste_crop_matches_fp64_composition(hip_device, paste_refs, B, H, W, K):
    from unsamflow_amd import fake_object as fo

    base, objs, slots, params, o32, o64 = paste_refs[(B, H, W, K)]
    cache = fakeobj_util.filled_cache(*objs, device=hip_device)
    dev = [t.to(hip_device) for t in base]
    assert float((o32[0][:, :3] - base[0]).abs().max()) > 0.05  # something was pasted
    for (ch, cw), (y0, x0) in (((H, W), (0, 0)), INTERIOR[(B, H, W)]):
        assert (ch, cw) == (H, W) or (y0 % 2 == 1 and x0 % 2 == 1 and cw % 2 == 1)
        outs = fo.paste_and_crop(*dev, cache, slots, params, (ch, cw), (y0, x0))
        win = (slice(None), slice(None), slice(y0, y0 + ch), slice(x0, x0 + cw))
        _check(f"{(B, H, W)} K={K} crop={(ch, cw)}@{(y0, x0)}", outs, o32, o64, win)


def test_cases_cover_what_they_claim(paste_refs):
    """K = 3 at B = 2: flipped and unflipped objects, a fractional, an integer,
    a zero and an out-of-frame motion, a fractional mask, overlapping rounds."""
    base, (mask, src, motion), slots, params, o32, _ = paste_refs[(2, 13, 21, 3)]
    assert params[:, 2].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0, 1.0]
    assert motion[1].tolist() == [2.0, -1.0] and motion[2].tolist() == [0.0, 0.0] and float(motion[3, 0]) >= 21
    assert float(motion[0, 0]) % 1 != 0
    frac = mask[1][(mask[1] > 0) & (mask[1] < 1)]
    assert frac.numel() > 10
    assert float((mask[0] * mask[2] * mask[4]).sum()) > 0  # sample 0's three rounds overlap


def test_round_order_shows_on_the_gpu(hip_device, paste_refs):
    from unsamflow_amd import fake_object as fo

    B, H, W = 2, 13, 21
    base, objs, slots, params, _, _ = paste_refs[(B, H, W, 3)]
    cache_c, cache_g = fakeobj_util.filled_cache(*objs), fakeobj_util.filled_cache(*objs, device=hip_device)
    dev = [t.to(hip_device) for t in base]
    rev = torch.cat([slots[2 * B:], slots[B:2 * B], slots[:B]])
    prev = torch.cat([params[2 * B:], params[B:2 * B], params[:B]])
    a = fo.paste_and_crop(*dev, cache_g, slots, params, (H, W), (0, 0))
    b = fo.paste_and_crop(*dev, cache_g, rev, prev, (H, W), (0, 0))
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    o32 = fo.paste_and_crop(*base, cache_c, rev, prev, (H, W), (0, 0))
    o64 = fo.paste_and_crop(*[t.double() for t in base], cache_c, rev, prev, (H, W), (0, 0))
    _check("reversed rounds", b, o32, o64, (slice(None),) * 4)


def test_paste_takes_a_flow_channel_slice_in_place(hip_device, paste_refs):
    """flows_12[0] of the harness is a channel slice of the [B,4,H,W] flow: batch stride 4*H*W, no copy."""
    from unsamflow_amd import fake_object as fo

    B, H, W = 2, 13, 21
    base, objs, slots, params, _, _ = paste_refs[(B, H, W, 3)]
    cache = fakeobj_util.filled_cache(*objs, device=hip_device)
    img1, img2, flow, noc = (t.to(hip_device) for t in base)
    flow4 = torch.cat([flow, flow + 100.0], 1)
    a = fo.paste_and_crop(img1, img2, flow, noc, cache, slots, params, (7, 9), (3, 5))
    b = fo.paste_and_crop(img1, img2, flow4[:, :2], noc, cache, slots, params, (7, 9), (3, 5))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the pop's rescaling reaches the kernel: the same factors on the cached motion as the composition applies
    p2 = params.clone()
    p2[:, :2] *= torch.tensor([1.37, -0.93, 0.8, 1.49, -1.2, 1.0]).view(-1, 1)
    cache_c = fakeobj_util.filled_cache(*objs)
    g = fo.paste_and_crop(img1, img2, flow, noc, cache, slots, p2, (H, W), (0, 0))
    o32 = fo.paste_and_crop(*base, cache_c, slots, p2, (H, W), (0, 0))
    o64 = fo.paste_and_crop(*[t.double() for t in base], cache_c, slots, p2, (H, W), (0, 0))
    _check("rescaled motions", g, o32, o64, (slice(None),) * 4)


# -------------------------------------------------------------------- push --
def _push_inputs(B, H, W, seed):
    mask, img, _ = fakeobj_util.objects(B, H, W, seed)
    flow = torch.from_numpy(hashrng.normal((B, 2, H, W), seed + 2)).abs() * 5.0 + 0.5  # one sign: nothing cancels
    flow[:, 1] *= -1.0
    return mask, img, flow


@pytest.mark.parametrize("B,H,W", [(1, 2, 3), (3, 33, 70), (2, 64, 96)])
def test_push_copies_and_means(hip_device, B, H, W):
    from unsamflow_amd.fake_object import ObjectCache

    d = hip_device
    mask, img, flow = _push_inputs(B, H, W, 1200 + H)
    valid = torch.tensor([B == 1 or b != 0 for b in range(B)])  # sample 1's mask is fractional
    runs = []
    for _ in range(2):
        c = ObjectCache(5, d)
        c.push(mask.to(d), img.to(d), flow.to(d), valid)
        runs.append((c.obj_mask.cpu(), c.img.cpu(), c.motion.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))  # deterministic
    keep = [b for b in range(B) if valid[b]]
    cm, ci, cmo = runs[0]
    assert c.count == len(keep)
    for slot, b in enumerate(keep):
        assert torch.equal(cm[slot], mask[b]) and torch.equal(ci[slot], img[b])
        m64, f64 = mask[b].double(), flow[b].double()
        ref = (f64 * m64).sum(dim=[1, 2]) / m64.sum()
        cpu32 = (flow[b] * mask[b]).sum(dim=[1, 2]) / mask[b].sum()
        e_ref = float((cpu32.double() - ref).abs().max())
        err = float((cmo[slot].double() - ref).abs().max())
        print(f"[fakeobj] push {(B, H, W)} sample {b}: err={err:.3e} e_ref={e_ref:.3e} ref={ref.tolist()}")
        assert err <= max(4.0 * e_ref, 2.0 ** -23 * float(ref.abs().max())), (b, err, e_ref)
    assert float(cm[len(keep):].abs().max()) == 0.0 and float(cmo[len(keep):].abs().max()) == 0.0


def test_push_skips_leave_every_cache_byte_unchanged(hip_device):
    from unsamflow_amd import ops
    from unsamflow_amd.fake_object import ObjectCache

    d = hip_device
    B, H, W = 3, 33, 70
    mask, img, flow = _push_inputs(B, H, W, 1300)
    c = ObjectCache(4, d)
    c.push(mask.to(d), img.to(d), flow.to(d), torch.ones(B, dtype=torch.bool))
    snap = [t.clone() for t in (c.obj_mask, c.img, c.motion)]
    skip = torch.full((B,), -1, dtype=torch.int32, device=d)
    ops.fakeobj_push(img[:, :1].to(d).contiguous(), (img * 0.5).to(d), flow.to(d), skip, c.obj_mask, c.img, c.motion)
    assert all(torch.equal(a, b) for a, b in zip(snap, (c.obj_mask, c.img, c.motion)))
    # a flow passed as a channel slice of [B,4,H,W], one sample skipped: only slot 3 changes
    flow4 = torch.cat([flow + 100.0, flow], 1).to(d)
    one = torch.tensor([-1, 3, -1], dtype=torch.int32, device=d)
    ops.fakeobj_push(mask.to(d), (img * 0.5).to(d), flow4[:, 2:], one, c.obj_mask, c.img, c.motion)
    assert all(torch.equal(a[:3], b[:3]) for a, b in zip(snap, (c.obj_mask, c.img, c.motion)))
    assert torch.equal(c.img[3].cpu(), img[1] * 0.5) and torch.equal(c.motion[3], snap[2][1])
    with pytest.raises(ValueError, match="synchronise"):
        c.push(mask.to(d), img.to(d), flow.to(d))
    assert ops.device_errors(d) == 0


def test_a_corrupted_slot_table_is_skipped_and_flagged(hip_device):
    """Slots outside [0, cache_size): nothing is addressed with them. The cache
    sits between sentinel-filled guard regions of one allocation; the guards and
    the cache stay as they were, the flag is raised and cleared."""
    from unsamflow_amd import _lib, ops

    d = hip_device
    B, H, W, n, G = 3, 13, 21, 4, 2
    base = [t.to(d) for t in fakeobj_util.base(B, H, W, 1400)]
    mask, src, motion = fakeobj_util.objects(n, H, W, 1410)
    big = [torch.full((n + 2 * G, c, H, W), -777.0, device=d) for c in (1, 3)] + [torch.full((n + 2 * G, 2), -777.0,
                                                                                            device=d)]
    cm, ci, cmo = (t[G:G + n] for t in big)
    cm.copy_(mask)
    ci.copy_(src)
    cmo.copy_(motion)
    snap = [t.clone() for t in big]
    assert ops.device_errors(d) == 0

    good = torch.tensor([0, 1, 2], dtype=torch.int32)
    bad = torch.tensor([0, n, 2, -5, 1, 2 ** 30], dtype=torch.int32)  # sample 1 round 0, samples 0 and 2 round 1
    params = fakeobj_util.plain_params(6).to(d)
    ref1 = ops.fakeobj_paste_crop(*base, cm, ci, cmo, good.to(d), params[:3], (H, W), (0, 0))
    assert ops.device_errors(d) == 0
    out = ops.fakeobj_paste_crop(*base, cm, ci, cmo, bad.to(d), params, (H, W), (0, 0))
    assert ops.device_errors(d, clear=False) == _lib.DEVERR_FAKEOBJ_BAD_SLOT
    assert ops.device_errors(d) == _lib.DEVERR_FAKEOBJ_BAD_SLOT and ops.device_errors(d) == 0  # cleared
    # the bad rounds were skipped: sample 0 = round 0 only, sample 1 = round 1 only, sample 2 = round 0 only
    only1 = ops.fakeobj_paste_crop(*base, cm, ci, cmo, torch.tensor([1, 1, 1], dtype=torch.int32, device=d),
                                   params[:3], (H, W), (0, 0))
    for a, r0, r1 in zip(out, ref1, only1):
        assert torch.equal(a[0], r0[0]) and torch.equal(a[2], r0[2]) and torch.equal(a[1], r1[1])
    assert all(torch.equal(a, b) for a, b in zip(snap, big))

    pm, pi, pf = _push_inputs(B, H, W, 1420)
    slots = torch.tensor([n, -7, 1], dtype=torch.int32, device=d)
    ops.fakeobj_push(pm.to(d), pi.to(d), pf.to(d), slots, cm, ci, cmo)
    assert ops.device_errors(d) == _lib.DEVERR_FAKEOBJ_BAD_SLOT and ops.device_errors(d) == 0
    for a, b in zip(snap, big):  # only slot 1 of the cache changed
        keep = [j for j in range(n + 2 * G) if j != G + 1]
        assert torch.equal(a[keep], b[keep])
    assert torch.equal(ci[1].cpu(), pi[2]) and torch.equal(cm[1].cpu(), pm[2])


def test_pop_paste_and_push_do_not_synchronise(hip_device, paste_refs):
    """The branch's own work -- pop, the table copies, paste + crop, push -- under
    torch's sync debug mode: a device-to-host read or a stream sync would raise."""
    from unsamflow_amd import fake_object as fo

    d = hip_device
    B, H, W = 2, 64, 96
    base, objs, _, _, _, _ = paste_refs[(B, H, W, 3)]
    dev = [t.to(d) for t in base]
    cache = fakeobj_util.filled_cache(*objs, device=d)
    cache.generator = torch.Generator().manual_seed(4)
    pm, pi, _ = _push_inputs(B, H, W, 1600)
    pm, pi = pm.to(d), pi.to(d)
    fo.paste_and_crop(*dev, cache, *cache.pop(3 * B), (40, 71), (7, 13))  # warm-up: library load, allocator
    cache.push(pm, pi, dev[2], torch.tensor([True, False]))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        slots, params = cache.pop(3 * B)
        out = fo.paste_and_crop(*dev, cache, slots, params, (40, 71), (7, 13))
        cache.push(pm, pi, dev[2], torch.tensor([False, True]))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out[0].shape == (B, 6, 40, 71) and bool(torch.isfinite(out[0]).all())


def test_paste_and_push_graph_replay(hip_device, paste_refs):
    """Paste + crop followed by a push, captured on one stream with fixed
    offsets after an eager warm-up and replayed twice: equal outputs, equal to eager."""
    from unsamflow_amd import ops

    d = hip_device
    B, H, W = 2, 64, 96
    base, objs, slots, params, _, _ = paste_refs[(B, H, W, 3)]
    static = [t.to(d) for t in base]
    cache = fakeobj_util.filled_cache(*objs, device=d, cache_size=8)
    tables = (slots.to(d), params.to(d), torch.tensor([6, -1], dtype=torch.int32, device=d))
    pm, pi, _ = _push_inputs(B, H, W, 1500)
    pm, pi = pm.to(d), pi.to(d)

    def fn():
        out = ops.fakeobj_paste_crop(*static, cache.obj_mask, cache.img, cache.motion, tables[0], tables[1],
                                     (40, 71), (7, 13))
        ops.fakeobj_push(pm, pi, static[2], tables[2], cache.obj_mask, cache.img, cache.motion)
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    got = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        got.append([t.clone() for t in out] + [cache.motion.clone(), cache.img[6].clone()])
    ref = [t.clone() for t in fn()] + [cache.motion.clone(), cache.img[6].clone()]
    torch.cuda.synchronize()
    for a, b, c in zip(got[0], got[1], ref):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(cache.img[6], pi[0]) and float(cache.motion[6].abs().max()) > 0
    del graph


# -------------------------------------------------------------------- step --
def test_fused_step_matches_the_torch_composition(hip_device, monkeypatch):
    """TrainStep(kitti_aug()) at B=2, 128x192, ot_size 64x128, a cache of 4 (so
    key_obj_count = 2: a pop takes distinct objects) from one seed, run until the
    cache is full and one pasting step has happened, fused against
    fused_fake_object=False: loss and l_ot at rtol 1e-4; one paste + crop and one
    push launch in the pasting step, none in the composition run."""
    from unsamflow_amd import config, ops
    from unsamflow_amd.harness import TrainStep, synthetic_key_objects, synthetic_pair

    B, H, W = 2, 128, 192
    img1, img2, _, _ = synthetic_pair(B, H, W, hip_device)
    mask, valid = synthetic_key_objects(B, H, W, hip_device, seed=8, p_invalid=0.0)
    cfg = config.kitti_aug()
    cfg.train.ot_size = [64, 128]
    cfg.train.key_obj_count = 2
    counts = {"fakeobj_paste_crop": 0, "fakeobj_push": 0}
    for name in counts:
        orig = getattr(ops, name)

        def spy(*a, _n=name, _f=orig, **k):
            counts[_n] += 1
            return _f(*a, **k)

        monkeypatch.setattr(ops, name, spy)
    res = {}
    for fused in (True, False):
        step = TrainStep(cfg, hip_device, fused_fake_object=fused, obj_cache_size=4)
        with torch.no_grad():
            for p in step.module.parameters():
                p.mul_(0.02)
        for _ in range(2):
            step(img1, img2, key_obj_mask=mask, key_obj_valid=valid)
        assert step.obj_cache.count == 4
        for k in counts:
            counts[k] = 0
        loss = step(img1, img2, key_obj_mask=mask, key_obj_valid=valid)
        res[fused] = (float(loss), float(step.l_ot), dict(counts))
    print(f"[fakeobj] step fused={res[True][:2]} torch={res[False][:2]} rel diff="
          f"{[abs(a - b) / abs(b) for a, b in zip(res[True][:2], res[False][:2])]}")
    assert res[True][2] == {"fakeobj_paste_crop": 1, "fakeobj_push": 1}
    assert res[False][2] == {"fakeobj_paste_crop": 0, "fakeobj_push": 0}
    for a, b in zip(res[True][:2], res[False][:2]):
        assert b > 0 and np.isfinite(a)
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=0)
    assert ops.device_errors(hip_device) == 0
