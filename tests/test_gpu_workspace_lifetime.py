"""Lifetime of the persistent workspaces (ops.persistent_workspace) under HIP
graph replay. A captured graph records only the address of the workspace that
ops.warp_backward / ops.occ_backward / ops.occ_vis_pair used, so the tensor has
to outlive the cache entry: least-recently-used eviction, the failed-call drop
(ops._drop_workspace) and ops.clear_persistent_workspaces() must leave it
allocated at the same address while a graph can replay into it, a hold that is
released must free it again, and a use on a stream other than the allocation
stream must be known to the caching allocator.

Every test asserts that the workspace is alive and at its address BEFORE it
replays, so no replay ever writes into released memory. Replays run with
reloaded inputs (smooth, border-piling, contracting, smooth: the workspace's
parity, counts, dirty words and overflow entries carry over from one to the
next) and are checked like the eager sequences of test_gpu_persist.py:

* warp backward against the CPU oracle (oracle/warp.py, restating
  utils/warp_utils.py:97-106 + ATen's sampler), atol 1e-4 / rtol 1e-5 (SURVEY
  8(c));
* the occlusion masks (utils/warp_utils.py:120-126) against the per-call entry
  usf_occ_backward_f32, which zeroes its map on every call. A pixel may differ
  only where the splat sum lies within 1e-5 of the threshold (atomic summation
  order), and at most 0.1 % of the pixels may be excused in this way.

Shapes: the smallest that reach each form -- (2,16,40,64) the dense persistent
warp backward (512 < H*W <= 8192), (2,8,96,100) the list form (H*W > 8192),
(2,40,64) the occlusion maps.
"""
import functools
import gc
import weakref

import numpy as np
import pytest
import torch

from oracle import hashrng
from oracle.warp import warp_backward_np
from persist_util import cache_pressure, np_fields
from unsamflow_amd import _lib, ops

pytestmark = pytest.mark.gpu

CASES = {
    "warp_dense": ("warp_bwd", (2, 16, 40, 64)),
    "warp_list": ("warp_bwd", (2, 8, 96, 100)),
    "occ_bwd": ("occ_bwd", (2, 40, 64)),
    "occ_vis_pair": ("occ_vis_pair", (2, 40, 64)),
}
SEQUENCE = ("smooth", "pile", "contract", "smooth")
TH = 0.2
MAX_EXCUSED = 1e-3  # share of the pixels that may sit within 1e-5 of the threshold


@functools.lru_cache(maxsize=None)
def _warp_inputs(shape):
    return hashrng.uniform(shape, 900 + shape[1]), hashrng.normal(shape, 901 + shape[1])


@functools.lru_cache(maxsize=None)
def _fields(B, H, W):
    return np_fields(B, H, W)


@functools.lru_cache(maxsize=None)
def _warp_ref(shape, kind):
    x, g = _warp_inputs(shape)
    return warp_backward_np(x, _fields(shape[0], *shape[2:])[kind], g, "border")


class _Case:
    """One persistent op at one shape: static input buffers, the call, and the
    check of its outputs against the reference for the field in the buffer."""

    def __init__(self, name, dev):
        self.op, self.shape = CASES[name]
        self.dev = dev
        self.key = (dev.index, self.op, self.shape)
        B, H, W = self.shape[0], self.shape[-2], self.shape[-1]
        self.fields = _fields(B, H, W)
        if self.op == "warp_bwd":
            x, g = _warp_inputs(self.shape)
            self.x, self.g = torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev)
            self.flow = torch.zeros(B, 2, H, W, device=dev)
        else:
            self.flow = torch.zeros(B, 4 if self.op == "occ_vis_pair" else 2, H, W, device=dev)
        self.load("smooth")

    def load(self, kind):
        f = torch.from_numpy(self.fields[kind]).to(self.dev)
        # the pair's other half is the reversed field, so each mask must come from its own channels
        self.flow.copy_(torch.cat([f, -f], 1) if self.op == "occ_vis_pair" else f)

    def call(self):
        if self.op == "warp_bwd":
            return ops.warp_backward(self.x, self.flow, self.g, "border", True, True)
        if self.op == "occ_bwd":
            return (ops.occ_backward(self.flow, TH),)
        return (ops.occ_vis_pair(self.flow, TH),)

    def entry(self):
        return ops._PERSIST[self.key][0]

    def _occ_check(self, got, flow, what):
        lib = _lib.load()
        B, _, H, W = flow.shape
        flow = flow.contiguous()
        ref, m = torch.empty_like(got), torch.empty_like(got)
        _lib.check(lib.usf_occ_backward_f32(flow.data_ptr(), 2 * H * W, ref.data_ptr(), B, H, W, TH,
                                            _lib.stream_handle(self.dev)), "usf_occ_backward_f32")
        _lib.check(lib.usf_splat_map_f32(flow.data_ptr(), 2 * H * W, m.data_ptr(), B, H, W, 0,
                                         _lib.stream_handle(self.dev)), "usf_splat_map_f32")
        diff = got != ref
        n = int(diff.sum())
        print(f"{what}: {n} of {got.numel()} pixels differ from the per-call form, mask mean {float(ref.mean()):.3f}")
        assert bool(((m[diff].clamp(0, 1) - TH).abs() < 1e-5).all()), what
        assert n <= MAX_EXCUSED * got.numel(), (what, n)

    def check(self, out, kind, what):
        what = f"{self.op} {self.shape} {what} {kind}"
        torch.cuda.synchronize()
        if self.op == "warp_bwd":
            rx, rf = _warp_ref(self.shape, kind)
            np.testing.assert_allclose(out[0].cpu().numpy(), rx, atol=1e-4, rtol=1e-5, err_msg=what + " gx")
            np.testing.assert_allclose(out[1].cpu().numpy(), rf, atol=1e-4, rtol=1e-5, err_msg=what + " gflow")
        elif self.op == "occ_bwd":
            self._occ_check(out[0], self.flow, what)
        else:  # vis[0] from channels 2:4, vis[1] from channels 0:2
            self._occ_check(1.0 - out[0][0], self.flow[:, 2:], what + " vis0")
            self._occ_check(1.0 - out[0][1], self.flow[:, :2], what + " vis1")


@pytest.fixture
def fresh_cache(hip_device, monkeypatch):
    """An empty cache and the persistent form at every shape; afterwards the
    process-lifetime hold of the test's bare captures is released again (their
    graphs are gone by then)."""
    monkeypatch.setattr(ops, "WARP_PERSIST_MAX_PIXELS", None)
    ops.clear_persistent_workspaces()
    yield hip_device
    torch.cuda.synchronize()
    gc.collect()
    hold = getattr(ops, "_PROCESS_HOLD", None)
    if hold is not None:
        hold.release()
    ops.clear_persistent_workspaces()


def _warm_on_side_stream(case):
    side = torch.cuda.Stream(case.dev)
    side.wait_stream(torch.cuda.current_stream(case.dev))
    with torch.cuda.stream(side):
        case.call()
    torch.cuda.current_stream(case.dev).wait_stream(side)
    torch.cuda.synchronize()


def _capture(case, hold=None):
    graph = torch.cuda.CUDAGraph()
    if hold is None:
        with torch.cuda.graph(graph):
            out = case.call()
    else:
        with hold, torch.cuda.graph(graph):
            out = case.call()
    return graph, out


def _assert_alive(ref, ptr, what):
    ws = ref()
    assert ws is not None, f"{what}: the captured workspace was freed while its graph can still be replayed"
    assert ws.data_ptr() == ptr, what


@pytest.mark.parametrize("name", list(CASES))
def test_captured_workspace_survives_pressure_and_replays(fresh_cache, name):
    """A bare torch.cuda.graph(...) around a persistent op: after eviction
    pressure, the drop of its key, a clear and a collection, the workspace is
    still allocated at the captured address; replays with reloaded inputs match
    the reference, leave tensors allocated afterwards untouched, and an eager
    call of the shape still works."""
    case = _Case(name, fresh_cache)
    _warm_on_side_stream(case)
    ref, ptr, nbytes = weakref.ref(case.entry()), case.entry().data_ptr(), case.entry().numel()
    graph, out = _capture(case)
    cache_pressure(case.dev, case.key)
    assert case.key not in ops._PERSIST
    _assert_alive(ref, ptr, name)  # before any replay: nothing below writes into released memory
    # tensors that would receive the block had it been freed (zeros is a valid workspace state)
    bystanders = [torch.zeros(nbytes, device=case.dev, dtype=torch.uint8) for _ in range(4)]
    for i, kind in enumerate(SEQUENCE):
        case.load(kind)
        graph.replay()
        case.check(out, kind, f"replay {i}")
    torch.cuda.synchronize()
    for b in bystanders:
        assert int(torch.count_nonzero(b)) == 0
    eager = case.call()  # a fresh entry: the cache no longer knows the captured one
    case.check(eager, SEQUENCE[-1], "eager after replays")
    assert case.entry().data_ptr() != ptr
    _assert_alive(ref, ptr, name)
    del graph


@pytest.mark.parametrize("name", ["warp_dense", "occ_vis_pair"])
def test_released_hold_frees_the_workspace(fresh_cache, name):
    """A capture under an explicit hold keeps the workspace through the
    pressure; once the graph is gone and the hold released, the same pressure
    frees it."""
    case = _Case(name, fresh_cache)
    _warm_on_side_stream(case)
    ref, ptr = weakref.ref(case.entry()), case.entry().data_ptr()
    hold, n_process = ops.WorkspaceHold(), len(ops._PROCESS_HOLD)
    graph, out = _capture(case, hold)
    assert len(hold) == 1 and len(ops._PROCESS_HOLD) == n_process  # filed under the explicit hold only
    cache_pressure(case.dev, case.key)
    _assert_alive(ref, ptr, name)
    graph.replay()
    case.check(out, "smooth", "replay under hold")
    case.call()  # the cache's new entry, not held
    del graph, out
    hold.release()
    del hold
    gc.collect()
    assert ref() is None  # the hold had the last reference
    ref2 = weakref.ref(case.entry())
    cache_pressure(case.dev, case.key)
    assert ref2() is None


def test_device_time_us_keeps_no_workspace(fresh_cache):
    """kernel_timer.device_time_us builds and deletes a graph per timed site:
    afterwards nothing but the cache refers to the site's workspace, so a sweep
    over shapes stays within the cache's bound."""
    from unsamflow_amd.kernel_timer import device_time_us

    case = _Case("occ_bwd", fresh_cache)
    n_process = len(ops._PROCESS_HOLD)
    assert device_time_us(case.call, reps=2, iters=1) > 0
    assert len(ops._PROCESS_HOLD) == n_process
    ref = weakref.ref(case.entry())
    cache_pressure(case.dev)
    assert ref() is None


@pytest.mark.parametrize("name", list(CASES))
def test_failed_call_on_held_workspace_resets_it_in_place(fresh_cache, name):
    """The failed-call path (ops._drop_workspace) on a workspace that a graph
    holds: it leaves the cache but is not freed; it is zero-filled in stream
    order, which is the state a fresh entry starts from, so the graph's next
    replays are right, whatever the state the failed call left."""
    case = _Case(name, fresh_cache)
    _warm_on_side_stream(case)
    ref, ptr = weakref.ref(case.entry()), case.entry().data_ptr()
    hold = ops.WorkspaceHold()
    graph, out = _capture(case, hold)
    case.load("contract")
    case.call()  # leaves the parity word set (warp) before the drop
    case.entry()[:4].fill_(0x5a)  # and a header no call could continue from
    ops._drop_workspace(case.dev, case.op, case.shape)
    assert case.key not in ops._PERSIST
    _assert_alive(ref, ptr, name)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ref())) == 0
    for kind in ("pile", "smooth"):
        case.load(kind)
        graph.replay()
        case.check(out, kind, "replay after drop")
    _assert_alive(ref, ptr, name)
    del graph, out
    hold.release()


def test_use_off_the_allocation_stream_is_recorded(fresh_cache, monkeypatch):
    """A workspace created on a side stream: its uses there are not reported to
    the caching allocator, its use on the main stream is (Tensor.record_stream),
    and so is the stream on which a hold is released."""
    told = []
    record_stream = torch.Tensor.record_stream

    def spy(self, stream):
        told.append((self.data_ptr(), stream))
        return record_stream(self, stream)

    monkeypatch.setattr(torch.Tensor, "record_stream", spy)
    case = _Case("occ_bwd", fresh_cache)
    main = torch.cuda.current_stream(case.dev)
    side = torch.cuda.Stream(case.dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        case.call()
        case.call()
    assert told == []
    ptr = case.entry().data_ptr()
    out = case.call()  # on the main stream, ordered after the side stream's calls
    assert told == [(ptr, main)]
    case.check(out, "smooth", "main after side")
    with torch.cuda.stream(side):
        case.call()
    assert told == [(ptr, main)]  # back on the allocation stream
    torch.cuda.synchronize()
    # a graph captured from a workspace of the side stream, replayed and released on the main stream
    del told[:]
    case2 = _Case("occ_vis_pair", fresh_cache)
    _warm_on_side_stream(case2)
    ptr2 = case2.entry().data_ptr()
    hold = ops.WorkspaceHold()
    graph, out2 = _capture(case2, hold)
    graph.replay()
    case2.check(out2, "smooth", "replay on main")
    del graph
    hold.release()
    assert (ptr2, main) in told
