"""Tensor-level entry points to the HIP kernels (no autograd).

Each function validates its tensors, allocates the outputs with torch (the
caching allocator owns all memory; the library never allocates), and launches
on torch's current stream of the tensors' device. There is deliberately no
CPU path: CPU tensors raise ``RuntimeError``.
"""
from __future__ import annotations

import ctypes
import weakref

import torch

from collections import OrderedDict, namedtuple

from . import _lib
from . import kernel_timer as _kt

PAD_MODES = {"zeros": _lib.PAD_ZEROS, "border": _lib.PAD_BORDER}


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _require_device_f32(name: str, t: torch.Tensor) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(
            f"unsamflow_amd: {name} is on {t.device}; the HIP kernels need tensors on a ROCm "
            "device (there is no CPU path)"
        )
    if t.dtype != torch.float32:
        raise TypeError(f"unsamflow_amd: {name} must be float32, got {t.dtype}")


def _check_out(name: str, t: torch.Tensor, shape, device) -> None:
    if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 {tuple(shape)} tensor on {device}")
    if t.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned (it is written in place; pass a fresh allocation)")


def _dense16(t: torch.Tensor) -> torch.Tensor:
    """``t`` dense and on a 16-byte boundary: what the C ABI asks of every dense
    tensor parameter (include/unsamflow_hip*.h, "Alignment"). A contiguous tensor
    at such an address -- every fresh allocation -- is returned as is, no copy; a
    batch slice of an odd-sized tensor (contiguous, 4-byte aligned) is copied once."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _nchw(name: str, t: torch.Tensor) -> tuple[int, int, int, int]:
    if t.dim() != 4:
        raise ValueError(f"{name} must be 4-D NCHW, got shape {tuple(t.shape)}")
    return tuple(t.shape)  # type: ignore[return-value]


def corr_forward(x1: torch.Tensor, x2: torch.Tensor, max_displacement: int,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """Cost volume [B,(2d+1)^2,H,W] of x1 against x2 (correlation_native.py:13-23).

    ``out``: optional preallocated contiguous fp32 output of the right shape."""
    _require_device_f32("input1", x1)
    _require_device_f32("input2", x2)
    B, C, H, W = _nchw("input1", x1)
    if x2.shape != x1.shape:
        raise ValueError(f"input2 shape {tuple(x2.shape)} != input1 shape {tuple(x1.shape)}")
    if x2.device != x1.device:
        raise ValueError("input1 and input2 are on different devices")
    d = int(max_displacement)
    K = 2 * d + 1
    x1c, x2c = _dense16(x1), _dense16(x2)
    if out is None:
        out = torch.empty((B, K * K, H, W), device=x1.device, dtype=torch.float32)
    else:
        _check_out("output", out, (B, K * K, H, W), x1.device)
    lib = _lib.load()
    ws, nws = _corr_workspace(lib, B, C, H, W, d, x1.device)
    _args = (x1c.data_ptr(), x2c.data_ptr(), out.data_ptr(), K * K * H * W, 0, 0.0, None,
             ws.data_ptr() if nws else None, nws, B, C, H, W, d, _lib.stream_handle(x1.device),)
    with torch.cuda.device(x1.device), _kt.timed(
        "corr_fwd", (B, C, H, W), x1.device, _kt.corr_bytes(B, C, H, W, K * K), _kt.corr_flops(B, C, H, W, K * K)
    ):
        # the _ex entry with a dense output stride: same result as usf_corr_fwd_f32,
        # plus the channel-split workspace for the small levels
        rc = lib.usf_corr_fwd_ex_f32(*_args)
    _lib.check(rc, "usf_corr_fwd_ex_f32")
    return out


def _corr_workspace(lib, B, C, H, W, d, device):
    """Caller-provided scratch for the forward's channel split (torch's caching
    allocator; empty when the shape does not split)."""
    n = int(lib.usf_corr_fwd_workspace(B, C, H, W, d))
    if n <= 0:
        return None, 0
    return torch.empty(n, device=device, dtype=torch.float32), n


def corr_backward(
    x1: torch.Tensor,
    x2: torch.Tensor,
    grad_out: torch.Tensor,
    max_displacement: int,
    need_x1: bool = True,
    need_x2: bool = True,
    gx1_out: torch.Tensor | None = None,
    gx2_out: torch.Tensor | None = None,
) -> tuple[torch.Tensor | None, torch.Tensor | None]:
    """(grad_input1, grad_input2) of :func:`corr_forward`; deterministic.

    ``gx1_out`` / ``gx2_out``: optional preallocated contiguous outputs."""
    _require_device_f32("input1", x1)
    _require_device_f32("input2", x2)
    _require_device_f32("grad_output", grad_out)
    B, C, H, W = _nchw("input1", x1)
    d = int(max_displacement)
    K = 2 * d + 1
    if tuple(grad_out.shape) != (B, K * K, H, W):
        raise ValueError(f"grad_output shape {tuple(grad_out.shape)} != {(B, K * K, H, W)}")
    if not (need_x1 or need_x2):
        return None, None
    x1c, x2c, gc = _dense16(x1), _dense16(x2), _dense16(grad_out)
    g1 = g2 = None
    if need_x1:
        g1 = torch.empty_like(x1c) if gx1_out is None else gx1_out
        _check_out("grad_input1", g1, (B, C, H, W), x1.device)
    if need_x2:
        g2 = torch.empty_like(x2c) if gx2_out is None else gx2_out
        _check_out("grad_input2", g2, (B, C, H, W), x1.device)
    lib = _lib.load()
    _args = (x1c.data_ptr(), x2c.data_ptr(), gc.data_ptr(), _ptr(g1), _ptr(g2), B, C, H, W, d,
             _lib.stream_handle(x1.device),)
    with torch.cuda.device(x1.device), _kt.timed(
        "corr_bwd", (B, C, H, W, need_x1, need_x2), x1.device,
        _kt.corr_bytes(B, C, H, W, K * K, True, need_x1, need_x2),
        _kt.corr_flops(B, C, H, W, K * K, True, need_x1, need_x2),
    ):
        rc = lib.usf_corr_bwd_f32(*_args)
    _lib.check(rc, "usf_corr_bwd_f32")
    return g1, g2


def _flow_view(flow: torch.Tensor, B: int, H: int, W: int) -> tuple[torch.Tensor, int]:
    """Flow tensor whose per-sample [2,H,W] block is dense, plus its batch stride.

    A channel slice such as ``flow[:, :2]`` of a contiguous [B,4,H,W] tensor
    (flow_loss.py:130-131) qualifies as-is (batch stride 4*H*W): no copy.
    """
    if tuple(flow.shape) != (B, 2, H, W):
        raise ValueError(f"flow shape {tuple(flow.shape)} != {(B, 2, H, W)}")
    s = flow.stride()
    if s[1] == H * W and s[2] == W and s[3] == 1 and (B == 1 or s[0] >= 2 * H * W):
        return flow, s[0] if B > 1 else 2 * H * W
    flow = flow.contiguous()
    return flow, 2 * H * W


def warp_forward(x: torch.Tensor, flow: torch.Tensor, pad: str = "border") -> torch.Tensor:
    """Bilinear backward warp of x by flow (warp_utils.py:97-106)."""
    _require_device_f32("x", x)
    _require_device_f32("flow12", flow)
    B, C, H, W = _nchw("x", x)
    if pad not in PAD_MODES:
        raise NotImplementedError(f"flow_warp padding mode {pad!r} (supported: border, zeros)")
    if flow.device != x.device:
        raise ValueError("x and flow12 are on different devices")
    xc = _dense16(x)
    fv, fbs = _flow_view(flow, B, H, W)
    out = torch.empty_like(xc)
    lib = _lib.load()
    _args = (xc.data_ptr(), fv.data_ptr(), fbs, out.data_ptr(), B, C, H, W, PAD_MODES[pad],
             _lib.stream_handle(x.device),)
    with torch.cuda.device(x.device), _kt.timed("warp_fwd", (B, C, H, W, pad), x.device, _kt.warp_bytes(B, C, H, W)):
        rc = lib.usf_warp_fwd_f32(*_args)
    _lib.check(rc, "usf_warp_fwd_f32")
    return out


# Persistent workspaces of the *_persist_* entry points (include/unsamflow_hip.h,
# ABI 8): zeroed once when created, then left reusable by every call, so the
# per-call fill launch is gone. One per (device, op, shape). The state they
# carry (a parity word, count buffers, dirty words, an overflow buffer, the
# occlusion splat map) must see its calls in order, so each entry records the
# stream of its last eager use, and a call from another stream first makes its
# stream wait for that one (torch's wait_stream): two streams can never race a
# workspace. An entry also remembers the stream it was allocated on: a use on
# any other stream is reported to the caching allocator (Tensor.record_stream,
# once per stream), so that a later free cannot hand the block out on the
# allocation stream while the other stream's kernels may still run.
#
# The cache is bounded (least recently used out): each warp entry holds ~88 B
# per pixel plus one float per element of x (up to 8192 pixels; one int per
# pixel above), each occlusion entry 4 B per pixel (8 B for the pair), and a
# training run with a changing shape (a partial last batch, evaluation at
# another resolution) must not keep every shape's buffers alive.
#
# A HIP graph capture reuses the workspace its eager warm-up created (torch
# captures on its own stream; the capture records no fill, and replays are uses
# on the replaying stream). The graph holds only the raw address, so a use
# while the current stream is capturing also takes a strong reference to the
# tensor into a WorkspaceHold: the innermost ``with WorkspaceHold()`` block, or,
# for a bare torch.cuda.graph(...), a module-level hold that lives as long as
# the process (that costs the entry's size per captured shape, see above, until
# clear_persistent_workspaces(release_held=True)). Eviction, _drop_workspace and
# clear_persistent_workspaces() only detach a held workspace from the cache: it
# stays allocated at its address until every hold on it is released
# (GraphedTrainStep.release(), kernel_timer.device_time_us per timed site).
#
# A call that fails drops its entry (its state may be half-updated): the next
# call of that shape starts from a fresh zeroed buffer. If the entry is held,
# a graph still replays into it, so it is not freed: it is zero-filled in
# stream order (zeros is the state a fresh entry starts from; the kernels read
# their parity from the device header) and detached from the cache.
class _Entry(list):
    """``[workspace, stream of its last eager use]`` of one cache slot, plus the
    stream the workspace was allocated on and the other streams the allocator
    has been told about."""
    __slots__ = ("alloc_stream", "recorded")

    def __init__(self, ws, stream):
        super().__init__((ws, stream))
        self.alloc_stream = stream
        self.recorded = set()

    def used_on(self, stream) -> None:
        """Tell the allocator that the workspace is used on ``stream``."""
        if stream != self.alloc_stream and stream not in self.recorded:
            self[0].record_stream(stream)
            self.recorded.add(stream)


class WorkspaceHold:
    """Strong references to the persistent workspaces that HIP graphs recorded.

    ``with hold, torch.cuda.graph(g): ...`` files every workspace that a
    persistent op uses during the capture under ``hold``; keep the hold next to
    the graph and call :meth:`release` when the graph goes away (on the stream
    the graph was replayed on). Until then the workspaces stay allocated at the
    captured addresses, whatever happens to the cache."""

    def __init__(self):
        self._held: dict[int, _Entry] = {}
        _HOLDS.add(self)

    def __enter__(self):
        _HOLD_STACK.append(self)
        return self

    def __exit__(self, *exc):
        _HOLD_STACK.remove(self)
        return False

    def __len__(self):
        return len(self._held)

    def _add(self, ent: _Entry) -> None:
        self._held[id(ent)] = ent

    def holds(self, ent: _Entry) -> bool:
        return id(ent) in self._held

    def release(self) -> None:
        """Drop the references. The graphs that recorded these workspaces must
        not be replayed again. The replays issued so far are taken to be on the
        current stream: the allocator is told so, and a workspace freed here is
        not handed out before they finish."""
        for ent in self._held.values():
            if not torch.cuda.is_current_stream_capturing():
                ent.used_on(torch.cuda.current_stream(ent[0].device))
        self._held.clear()


_PERSIST: "OrderedDict[tuple, _Entry]" = OrderedDict()
PERSIST_MAX_ENTRIES = 32
_HOLDS: "weakref.WeakSet[WorkspaceHold]" = weakref.WeakSet()
_HOLD_STACK: "list[WorkspaceHold]" = []  # the open ``with WorkspaceHold()`` blocks, innermost last
_PROCESS_HOLD = WorkspaceHold()  # captures outside any such block


def _is_held(ent: _Entry) -> bool:
    return any(h.holds(ent) for h in _HOLDS)


def persistent_workspace(device: torch.device, op: str, shape: tuple, nbytes: int) -> torch.Tensor:
    """The zero-initialised persistent workspace of ``op`` at ``shape`` on
    ``device``, ordered after its previous use (created on first use with
    torch.zeros on the current stream, so the zeroing precedes the first call).

    A use on a stream other than the one it was allocated on is recorded with
    the caching allocator. A use while the current stream is capturing a HIP
    graph puts the tensor into the innermost open :class:`WorkspaceHold`, or
    into the process-lifetime hold: the graph's address stays valid after
    eviction, :func:`_drop_workspace` and :func:`clear_persistent_workspaces`."""
    key = (device.index, op, tuple(shape))
    cur = torch.cuda.current_stream(device)
    capturing = torch.cuda.is_current_stream_capturing()
    ent = _PERSIST.get(key)
    if ent is not None and ent[0].numel() >= nbytes:
        _PERSIST.move_to_end(key)
        if capturing:
            (_HOLD_STACK[-1] if _HOLD_STACK else _PROCESS_HOLD)._add(ent)
        else:
            if ent[1] != cur:
                cur.wait_stream(ent[1])  # the previous use on another stream comes first
                ent[1] = cur
                ent.used_on(cur)  # every use off the allocation stream follows a switch to it
        return ent[0]
    if capturing:
        # torch.zeros inside a capture is only recorded: the eager calls after it
        # would start from uninitialised state
        raise RuntimeError(
            f"unsamflow_amd: first use of the persistent {op} workspace for shape {tuple(shape)} inside a "
            "HIP graph capture; run the call once eagerly before capturing")
    ws = torch.zeros(nbytes, device=device, dtype=torch.uint8)
    _PERSIST[key] = _Entry(ws, cur)
    while len(_PERSIST) > PERSIST_MAX_ENTRIES:
        _PERSIST.popitem(last=False)
    return ws


def _drop_workspace(device: torch.device, op: str, shape: tuple) -> None:
    """Detach the entry of a failed call from the cache. Not held: it is freed.
    Held by a capture: it stays allocated and is put back to its initial state,
    zero-filled on the current stream after its last eager use (nothing ran if
    the failure happened inside a capture, so nothing is filled then)."""
    ent = _PERSIST.pop((device.index, op, tuple(shape)), None)
    if ent is None or not _is_held(ent) or torch.cuda.is_current_stream_capturing():
        return
    cur = torch.cuda.current_stream(device)
    if ent[1] != cur:
        cur.wait_stream(ent[1])
    ent[1] = cur
    ent.used_on(cur)
    ent[0].zero_()


def clear_persistent_workspaces(release_held: bool = False) -> None:
    """Empty the cache: every workspace that no capture holds is released, and
    the next call of each shape re-creates it. A workspace held for a HIP graph
    (:class:`WorkspaceHold`) only leaves the cache and stays allocated.

    ``release_held=True`` also releases every live hold, the process-lifetime
    one included. THIS INVALIDATES LIVE GRAPHS: a graph that recorded one of
    these workspaces must never be replayed afterwards (its replay would write
    into memory that may belong to another tensor)."""
    _PERSIST.clear()
    if release_held:
        for h in list(_HOLDS):
            h.release()


# The largest level (H*W pixels) that takes the persistent warp backward
# (usf_warp_bwd_persist_f32); larger ones take the four-launch per-call form
# (None: every level). The library picks the persistent layout by size: up to
# 8192 pixels two launches with a dense overflow buffer, above that three (the
# overflow listed and added by the overflow pass; no zero fill). Chosen by the
# in-step time of the training step (tools/instep_ab.py, same process,
# alternating, 6 rounds; profiles/ab_r06/warp_form_list.json): KITTI L4 (64x208)
# 55.4 us in the list form vs 59.0 four-launch; the dense form there was 68.8
# (profiles/ab_r06/warp_form_instep_r2.json).
WARP_PERSIST_MAX_PIXELS: int | None = None


def warp_backward(
    x: torch.Tensor,
    flow: torch.Tensor,
    grad_out: torch.Tensor,
    pad: str = "border",
    need_x: bool = True,
    need_flow: bool = True,
) -> tuple[torch.Tensor | None, torch.Tensor | None]:
    """(grad_x, grad_flow) of :func:`warp_forward`.

    grad_x is the library's binned gather in its persistent form
    (``usf_warp_bwd_persist_f32``: one launch with LDS binning up to 512 pixels,
    two launches up to 8192, three above with the overflow pass and no zero
    fill): every source pixel is filed under its
    north-west corner cell and each target cell sums its sources in a fixed
    order, so grad_x is deterministic unless a cell receives more than 4 source
    pixels (strongly compressive flow), whose excess is added with fp32
    atomics. Its workspace (``usf_warp_bwd_persist_workspace``: ~88 B per pixel,
    plus one float per element of x up to 8192 pixels, one int per pixel above)
    is kept per (device, shape), ordered across streams and, when the call is
    captured into a HIP graph, kept allocated for that graph
    (:func:`persistent_workspace`, :class:`WorkspaceHold`). grad_flow is
    deterministic."""
    _require_device_f32("x", x)
    _require_device_f32("flow12", flow)
    _require_device_f32("grad_output", grad_out)
    B, C, H, W = _nchw("x", x)
    if pad not in PAD_MODES:
        raise NotImplementedError(f"flow_warp padding mode {pad!r} (supported: border, zeros)")
    if tuple(grad_out.shape) != (B, C, H, W):
        raise ValueError(f"grad_output shape {tuple(grad_out.shape)} != {(B, C, H, W)}")
    if not (need_x or need_flow):
        return None, None
    xc = _dense16(x)
    fv, fbs = _flow_view(flow, B, H, W)
    gc = _dense16(grad_out)
    gx = torch.empty_like(xc) if need_x else None  # overwritten by the library
    gf = torch.empty((B, 2, H, W), device=x.device, dtype=torch.float32) if need_flow else None
    lib = _lib.load()
    # grad_x by the binned gather, persistent form (C <= 256), else the
    # four-launch form with a per-call workspace from torch's caching allocator
    # (the C ABI's limits of the persistent form: a 32-bit dirty mask of channel
    # groups, packed (y, x), both count buffers under 32-bit byte offsets)
    persist = need_x and C <= 256 and H < 32768 and W < 65536 and 8 * B * (H + 1) * (W + 1) < 2 ** 31
    if WARP_PERSIST_MAX_PIXELS is not None and H * W > WARP_PERSIST_MAX_PIXELS:
        persist = False
    with torch.cuda.device(x.device):
        if persist:
            nws = int(lib.usf_warp_bwd_persist_workspace(B, C, H, W))
            ws = persistent_workspace(x.device, "warp_bwd", (B, C, H, W), nws)
        else:
            nws = int(lib.usf_warp_bwd_workspace(B, H, W)) if need_x else 0
            ws = torch.empty(nws, device=x.device, dtype=torch.uint8) if nws > 0 else None
        fn = lib.usf_warp_bwd_persist_f32 if persist else lib.usf_warp_bwd_ex_f32
        _args = (xc.data_ptr(), fv.data_ptr(), fbs, gc.data_ptr(), _ptr(gx), _ptr(gf), _ptr(ws), nws, B, C, H, W,
                 PAD_MODES[pad], _lib.stream_handle(x.device),)
        with _kt.timed("warp_bwd", (B, C, H, W, pad, need_x, need_flow), x.device,
                       _kt.warp_bytes(B, C, H, W, True, need_x, need_flow)):
            rc = fn(*_args)
    if rc != 0 and persist:
        _drop_workspace(x.device, "warp_bwd", (B, C, H, W))
    _lib.check(rc, "usf_warp_bwd_persist_f32" if persist else "usf_warp_bwd_ex_f32")
    return gx, gf


def _flow_arg(flow: torch.Tensor, name: str) -> tuple[torch.Tensor, int, int, int, int]:
    _require_device_f32(name, flow)
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError(f"{name} must be [B,2,H,W], got {tuple(flow.shape)}")
    B, _, H, W = flow.shape
    fv, fbs = _flow_view(flow, B, H, W)
    return fv, fbs, B, H, W


def splat_map(flow: torch.Tensor, absolute: bool = False) -> torch.Tensor:
    """Forward bilinear splat of unit mass (warp_utils.py:26-94) -> [B,1,H,W].

    ``absolute``: ``flow`` holds target coordinates (get_corresponding_map's
    argument) instead of displacements from the pixel grid."""
    fv, fbs, B, H, W = _flow_arg(flow, "flow")
    out = torch.empty((B, 1, H, W), device=flow.device, dtype=torch.float32)
    lib = _lib.load()
    _args = (fv.data_ptr(), fbs, out.data_ptr(), B, H, W, int(bool(absolute)), _lib.stream_handle(flow.device),)
    with torch.cuda.device(flow.device), _kt.timed("splat", (B, 1, H, W, bool(absolute)), flow.device,
                                                     4 * B * H * W * 3):
        rc = lib.usf_splat_map_f32(*_args)
    _lib.check(rc, "usf_splat_map_f32")
    return out


def occ_backward(flow21: torch.Tensor, th: float = 0.2) -> torch.Tensor:
    """Occlusion mask get_occu_mask_backward (warp_utils.py:120-126) -> [B,1,H,W] float.

    The splat map is a persistent workspace per (device, B, H, W): ordered
    across streams, and held for the graph when the call is captured
    (:func:`persistent_workspace`, :class:`WorkspaceHold`)."""
    fv, fbs, B, H, W = _flow_arg(flow21, "flow21")
    out = torch.empty((B, 1, H, W), device=flow21.device, dtype=torch.float32)
    lib = _lib.load()
    with torch.cuda.device(flow21.device):
        # the splat map lives in a persistent zeroed buffer that the threshold pass
        # re-zeroes (usf_occ_backward_persist_f32: two launches, no fill)
        nmap = 4 * B * H * W
        ws = persistent_workspace(flow21.device, "occ_bwd", (B, H, W), nmap)
        _args = (fv.data_ptr(), fbs, out.data_ptr(), ws.data_ptr(), nmap, B, H, W, float(th),
                 _lib.stream_handle(flow21.device),)
        with _kt.timed("occ_bwd", (B, 1, H, W), flow21.device, 4 * B * H * W * 3):
            rc = lib.usf_occ_backward_persist_f32(*_args)
    if rc != 0:
        _drop_workspace(flow21.device, "occ_bwd", (B, H, W))
    _lib.check(rc, "usf_occ_backward_persist_f32")
    return out


def occ_vis_pair(flow4: torch.Tensor, th: float = 0.2) -> torch.Tensor:
    """Both visibility masks of a with_bk loss at once (flow_loss.py:101-103):
    ``vis[0] = 1 - get_occu_mask_backward(flow4[:, 2:], th)``, ``vis[1] = 1 -
    get_occu_mask_backward(flow4[:, :2], th)`` -> [2,B,1,H,W] (each half a
    contiguous [B,1,H,W]): one splat launch over both flow halves into a
    persistent interleaved map and one threshold pass (usf_occ_vis_pair_persist_f32)
    instead of two splats, two thresholds and two ``1 - occ`` passes. The map is
    a persistent workspace like :func:`occ_backward`'s: ordered across streams,
    and held for the graph when the call is captured (:class:`WorkspaceHold`)."""
    _require_device_f32("flow4", flow4)
    if flow4.dim() != 4 or flow4.shape[1] != 4:
        raise ValueError(f"flow4 must be [B,4,H,W], got {tuple(flow4.shape)}")
    f = flow4.contiguous()
    B, _, H, W = f.shape
    vis = torch.empty((2, B, 1, H, W), device=f.device, dtype=torch.float32)
    lib = _lib.load()
    with torch.cuda.device(f.device):
        nmap = 8 * B * H * W
        ws = persistent_workspace(f.device, "occ_vis_pair", (B, H, W), nmap)
        _args = (f.data_ptr(), 4 * H * W, vis.data_ptr(), ws.data_ptr(), nmap, B, H, W, float(th),
                 _lib.stream_handle(f.device),)
        with _kt.timed("occ_vis_pair", (B, 1, H, W), f.device, 4 * B * H * W * 6):
            rc = lib.usf_occ_vis_pair_persist_f32(*_args)
    if rc != 0:
        _drop_workspace(f.device, "occ_vis_pair", (B, H, W))
    _lib.check(rc, "usf_occ_vis_pair_persist_f32")
    return vis


def occ_bidirection(flow12: torch.Tensor, flow21: torch.Tensor, scale: float = 0.01, bias: float = 0.5
                    ) -> torch.Tensor:
    """Occlusion mask get_occu_mask_bidirection (warp_utils.py:109-117) -> [B,1,H,W] float, one kernel."""
    f1, bs1, B, H, W = _flow_arg(flow12, "flow12")
    f2, bs2, B2, H2, W2 = _flow_arg(flow21, "flow21")
    if (B2, H2, W2) != (B, H, W):
        raise ValueError(f"flow21 shape {tuple(flow21.shape)} != flow12 shape {tuple(flow12.shape)}")
    out = torch.empty((B, 1, H, W), device=flow12.device, dtype=torch.float32)
    lib = _lib.load()
    _args = (f1.data_ptr(), bs1, f2.data_ptr(), bs2, out.data_ptr(), B, H, W, float(scale), float(bias),
             _lib.stream_handle(flow12.device),)
    with torch.cuda.device(flow12.device), _kt.timed("occ_bidir", (B, 1, H, W), flow12.device,
                                                       4 * B * H * W * 5):
        rc = lib.usf_occ_bidirection_f32(*_args)
    _lib.check(rc, "usf_occ_bidirection_f32")
    return out


def _host_array(ctype, values):
    return (ctype * len(values))(*values)


# ---- the fused photometric losses: L1 + SSIM (photo.hip) and census (census.hip).
# Both families have the same six entries with the same arguments. A _LossKind
# holds what differs: the prefix of the usf_<prefix>_loss_* entries and of the
# <prefix>_* timer ops, the title of the messages, the floats of out per
# direction (the loss, then its coefficients), the planes of the gradient basis
# per direction, the entries' weight arguments, and the channel / shape rule
# (census: C = 3 and an interior pixel; else C <= 3). The _loss_* functions bind
# each entry once.
_LossKind = namedtuple("_LossKind", "prefix title nout planes weights census_rule")
_PHOTO = _LossKind("photo", "photometric", 3, 4, ("w_l1", "w_ssim"), False)
_CENSUS = _LossKind("census", "census", 2, 2, ("w_ternary",), True)


def _loss_call(kind, entry, op, key, device, nbytes, args):
    name = f"usf_{kind.prefix}_loss_{entry}"
    fn, stream = getattr(_lib.load(), name), _lib.stream_handle(device)
    with torch.cuda.device(device), _kt.timed(f"{kind.prefix}_{op}", key, device, nbytes):
        rc = fn(*args, stream)
    _lib.check(rc, name)


def _loss_tail(kind, pad, weights):
    """(pad_mode, *weights), the last arguments of a forward entry."""
    if pad not in PAD_MODES:
        raise NotImplementedError(f"flow_warp padding mode {pad!r} (supported: border, zeros)")
    if len(weights) != len(kind.weights):
        raise TypeError(f"the {kind.title} loss takes the weights {kind.weights}, got {len(weights)} values")
    return (PAD_MODES[pad],) + tuple(float(w) for w in weights)


def _loss_images(kind, src, tgt, mask):
    for n, t in (("src", src), ("tgt", tgt), ("mask", mask)):
        _require_device_f32(n, t)
    B, C, H, W = _nchw("src", src)
    if tuple(tgt.shape) != (B, C, H, W) or tuple(mask.shape) != (B, 1, H, W):
        raise ValueError(f"tgt {tuple(tgt.shape)} / mask {tuple(mask.shape)} do not match src {(B, C, H, W)}")
    if C > 3:
        raise NotImplementedError(f"fused photometric loss supports C <= 3 image channels, got {C}")
    if kind.census_rule and C != 3:
        raise NotImplementedError(f"fused census loss needs C = 3 image channels, got {C}")
    if kind.census_rule and (H < 3 or W < 3):
        raise ValueError(f"fused census loss needs H, W >= 3 (an interior pixel), got {(H, W)}")
    return _dense16(src), _dense16(tgt), _dense16(mask), B, C, H, W


def _loss_pair_args(kind, flow, im1, im2, mask1, mask2):
    a, b_, m1, B, C, H, W = _loss_images(kind, im1, im2, mask1)
    _require_device_f32("mask2", mask2)
    m2 = _dense16(mask2)
    _require_device_f32("flow", flow)
    if tuple(m2.shape) != (B, 1, H, W):
        raise ValueError(f"mask2 {tuple(m2.shape)} does not match {(B, 1, H, W)}")
    if tuple(flow.shape) != (B, 4, H, W):
        raise ValueError(f"flow must be [B,4,H,W] = {(B, 4, H, W)}, got {tuple(flow.shape)}")
    fv = flow if flow[0].is_contiguous() else flow.contiguous()
    return fv, a, b_, m1, m2, B, C, H, W, fv.stride(0) if B > 1 else 4 * H * W


def _loss_forward(kind, ndir, flow, a, b_, m1, m2, pad, weights, need_grad):
    """One scale. ndir = 1: rec = warp(a, flow [B,2,H,W]) against b_ under m1 (m2
    unused); ndir = 2: the with_bk pair of im1 = a, im2 = b_ and flow [B,4,H,W]."""
    tail = _loss_tail(kind, pad, weights)
    if ndir == 2:
        fv, a, b_, m1, m2, B, C, H, W, fbs = _loss_pair_args(kind, flow, a, b_, m1, m2)
        masks, entry, op = (m1.data_ptr(), m2.data_ptr()), "pair_fwd_f32", "pair"
    else:
        a, b_, m1, B, C, H, W = _loss_images(kind, a, b_, m1)
        _require_device_f32("flow", flow)
        fv, fbs = _flow_view(flow, B, H, W)
        masks, entry, op = (m1.data_ptr(),), "fwd_f32", "fwd"
    dev = a.device
    npart = ndir * getattr(_lib.load(), f"usf_{kind.prefix}_loss_partials")(B, H, W)
    partials = torch.empty(npart, device=dev, dtype=torch.float32)
    out = torch.empty(ndir * kind.nout, device=dev, dtype=torch.float32)
    basis = torch.empty((B, ndir * kind.planes, H, W), device=dev, dtype=torch.float32) if need_grad else None
    # algorithmic bytes (each input read once): both images (2C), per
    # direction its flow and mask; with the gradient the basis planes written once
    nbytes = 4 * B * H * W * (2 * C + 3 * ndir + (ndir * kind.planes if need_grad else 0))
    _loss_call(kind, entry, op + ("_grad" if need_grad else ""), (B, C, H, W, pad), dev, nbytes,
               (a.data_ptr(), b_.data_ptr()) + masks + (fv.data_ptr(), fbs, partials.data_ptr(), out.data_ptr(),
                                                        _ptr(basis), B, C, H, W) + tail)
    return out, basis


def _loss_pyramid_forward(kind, flows, im1s, im2s, masks1, masks2, pad, weights, need_grad):
    tail = _loss_tail(kind, pad, weights)
    n = len(flows)
    if not 1 <= n <= 4 or not (len(im1s) == len(im2s) == len(masks1) == len(masks2) == n):
        raise ValueError(f"1..4 scales with one flow, two images and two masks each (got {n})")
    args = [_loss_pair_args(kind, *x) for x in zip(flows, im1s, im2s, masks1, masks2)]
    B, C = args[0][5], args[0][6]
    if any(x[5] != B or x[6] != C for x in args):
        raise ValueError("every scale needs the same batch and channel count")
    dev = args[0][1].device
    Hs = _host_array(ctypes.c_int, [x[7] for x in args])
    Ws = _host_array(ctypes.c_int, [x[8] for x in args])
    npart = int(getattr(_lib.load(), f"usf_{kind.prefix}_loss_pyramid_partials")(n, Hs, Ws, B))
    partials = torch.empty(npart, device=dev, dtype=torch.float32)
    out = torch.empty((n, 2 * kind.nout), device=dev, dtype=torch.float32)
    bases = None
    if need_grad:
        bases = [torch.empty((B, 2 * kind.planes, x[7], x[8]), device=dev, dtype=torch.float32) for x in args]
    ptrs = lambda i: _host_array(ctypes.c_void_p, [x[i].data_ptr() for x in args])  # noqa: E731
    nbytes = sum(4 * B * x[7] * x[8] * (2 * C + 4 + 2 + (2 * kind.planes if need_grad else 0)) for x in args)
    key = (B, C) + tuple(v for x in args for v in (x[7], x[8])) + (pad,)
    _loss_call(kind, "pyramid_fwd_f32", "pyr_grad" if need_grad else "pyr", key, dev, nbytes,
               (n, ptrs(1), ptrs(2), ptrs(3), ptrs(4), ptrs(0), _host_array(ctypes.c_longlong, [x[9] for x in args]),
                Hs, Ws, partials.data_ptr(), npart, out.data_ptr(),
                _host_array(ctypes.c_void_p, [t.data_ptr() for t in bases]) if need_grad else None, B, C) + tail)
    return out, bases


def _loss_pyramid_backward(kind, bases, coef, grad_losses):
    n, K = len(bases), 2 * kind.planes
    for t in bases:
        _require_device_f32("basis", t)
        if t.dim() != 4 or t.shape[1] != K:
            raise ValueError(f"gradient basis must be [B,{K},H,W], got {tuple(t.shape)}")
    B = bases[0].shape[0]
    dev = bases[0].device
    gl = grad_losses.reshape(-1).to(torch.float32).contiguous()
    if gl.numel() != 2 * n or coef.numel() != 2 * kind.nout * n:
        raise ValueError(f"grad_losses / coef sizes {gl.numel()} / {coef.numel()} for {n} scales")
    bases = [_dense16(t) for t in bases]
    coef = coef.contiguous()
    gflows = [torch.empty((B, 4) + tuple(t.shape[2:]), device=dev, dtype=torch.float32) for t in bases]
    ptrs = lambda ts: _host_array(ctypes.c_void_p, [t.data_ptr() for t in ts])  # noqa: E731
    key = (B, 2) + tuple(v for t in bases for v in t.shape[2:])
    nbytes = sum(4 * B * t.shape[2] * t.shape[3] * (K + 4) for t in bases)
    _loss_call(kind, "pyramid_bwd_f32", "pyr_bwd", key, dev, nbytes,
               (n, ptrs(bases), coef.data_ptr(), gl.data_ptr(), ptrs(gflows),
                _host_array(ctypes.c_int, [t.shape[2] for t in bases]),
                _host_array(ctypes.c_int, [t.shape[3] for t in bases]), B))
    return gflows


def _loss_backward(kind, basis, coef, grad_loss):
    _require_device_f32("basis", basis)
    B, K, H, W = _nchw("basis", basis)
    P = kind.planes
    if K not in (P, 2 * P):
        raise ValueError(f"gradient basis must be [B,{P},H,W] or [B,{2 * P},H,W], got {tuple(basis.shape)}")
    ndir = K // P
    basis = _dense16(basis)
    coef = coef.contiguous()
    gl = grad_loss.reshape(-1).to(torch.float32).contiguous()
    if gl.numel() != ndir or coef.numel() != kind.nout * ndir:
        raise ValueError(f"grad_loss / coef have {gl.numel()} / {coef.numel()} elements for {ndir} direction(s)")
    gflow = torch.empty((B, 2 * ndir, H, W), device=basis.device, dtype=torch.float32)
    _loss_call(kind, "bwd_f32", "bwd", (B, ndir, H, W), basis.device, 4 * B * H * W * (P + 2) * ndir,
               (basis.data_ptr(), coef.data_ptr(), gl.data_ptr(), gflow.data_ptr(), B, H, W, ndir))
    return gflow


def photo_loss_forward(src, tgt, mask, flow, pad: str = "border", w_l1: float = 0.15, w_ssim: float = 0.85,
                       need_grad: bool = False):
    """Fused warp + occlusion-aware L1/SSIM photometric loss of one scale and
    direction (flow_loss.py:127-148, loss_blocks.py:53-72) -> (out, basis):
    ``out`` = tensor [3] on the device {loss, c_l1, c_ssim}; with ``need_grad``
    ``basis`` = [B,4,H,W], the per-pixel flow-gradient basis computed in the
    same pass (dL/dflow = c_l1 * basis[:, :2] + c_ssim * basis[:, 2:]), else None."""
    return _loss_forward(_PHOTO, 1, flow, src, tgt, mask, None, pad, (w_l1, w_ssim), need_grad)


def photo_loss_pair_forward(flow, im1, im2, mask1, mask2, pad: str = "border", w_l1: float = 0.15,
                            w_ssim: float = 0.85, need_grad: bool = False):
    """Both directions of a with_bk scale in one launch (flow_loss.py:130-131):
    direction 0 = loss(im1, warp(im2, flow[:, :2]), mask1), direction 1 =
    loss(im2, warp(im1, flow[:, 2:]), mask2) -> (out [6] = {loss, c_l1, c_ssim}
    per direction, basis [B,8,H,W] (= [B,2,4,H,W]) or None)."""
    return _loss_forward(_PHOTO, 2, flow, im1, im2, mask1, mask2, pad, (w_l1, w_ssim), need_grad)


def photo_loss_pyramid_forward(flows, im1s, im2s, masks1, masks2, pad: str = "border", w_l1: float = 0.15,
                               w_ssim: float = 0.85, need_grad: bool = False):
    """:func:`photo_loss_pair_forward` for up to 4 loss scales in one launch
    (usf_photo_loss_pyramid_fwd_f32; the largest scale first) -> (out
    [nscale, 6] = {loss, c_l1, c_ssim} per direction per scale, bases: a list
    of [B,8,H_k,W_k] or None)."""
    return _loss_pyramid_forward(_PHOTO, flows, im1s, im2s, masks1, masks2, pad, (w_l1, w_ssim), need_grad)


def photo_loss_pyramid_backward(bases, coef, grad_losses):
    """d(loss)/d(flow_k) * grad for every scale of :func:`photo_loss_pyramid_forward`
    in one launch: bases [B,8,H_k,W_k], coef = its out [nscale, 6], grad_losses
    [nscale, 2] -> list of [B,4,H_k,W_k] (deterministic)."""
    return _loss_pyramid_backward(_PHOTO, bases, coef, grad_losses)


def photo_loss_backward(basis, coef, grad_loss):
    """d(photo loss)/d(flow) * grad_loss from the forward's gradient basis
    ([B,4,H,W] one direction, [B,8,H,W] a pair) and coefficients ->
    [B,2,H,W] / [B,4,H,W] (deterministic)."""
    return _loss_backward(_PHOTO, basis, coef, grad_loss)


def census_loss_forward(src, tgt, mask, flow, pad: str = "border", w_ternary: float = 1.0,
                        need_grad: bool = False):
    """:func:`photo_loss_forward` of the ternary (census) term (loss_blocks.py:12-50)
    -> (out [2] = {loss, c_t}, basis [B,2,H,W] or None; dL/dflow = c_t * basis)."""
    return _loss_forward(_CENSUS, 1, flow, src, tgt, mask, None, pad, (w_ternary,), need_grad)


def census_loss_pair_forward(flow, im1, im2, mask1, mask2, pad: str = "border", w_ternary: float = 1.0,
                             need_grad: bool = False):
    """:func:`photo_loss_pair_forward` of the census term -> (out [4] = {loss, c_t}
    per direction, basis [B,4,H,W] (= [B,2,2,H,W]) or None)."""
    return _loss_forward(_CENSUS, 2, flow, im1, im2, mask1, mask2, pad, (w_ternary,), need_grad)


def census_loss_pyramid_forward(flows, im1s, im2s, masks1, masks2, pad: str = "border", w_ternary: float = 1.0,
                                need_grad: bool = False):
    """:func:`census_loss_pair_forward` for up to 4 loss scales in one launch -> (out
    [nscale, 4] = {loss, c_t} per direction per scale, bases: a list of [B,4,H_k,W_k] or None)."""
    return _loss_pyramid_forward(_CENSUS, flows, im1s, im2s, masks1, masks2, pad, (w_ternary,), need_grad)


def census_loss_pyramid_backward(bases, coef, grad_losses):
    """:func:`photo_loss_pyramid_backward` of the census term: bases [B,4,H_k,W_k], coef
    [nscale, 4], grad_losses [nscale, 2] -> list of [B,4,H_k,W_k] (deterministic)."""
    return _loss_pyramid_backward(_CENSUS, bases, coef, grad_losses)


def census_loss_backward(basis, coef, grad_loss):
    """:func:`photo_loss_backward` of the census term: basis [B,2,H,W] (one direction)
    or [B,4,H,W] (a pair) and coefficients -> the same shape (deterministic)."""
    return _loss_backward(_CENSUS, basis, coef, grad_loss)


def ar_transform(img1, img2, flow, mask, theta, noise1=None, noise2=None):
    """The stage-1 spatial transform of two frames, one flow and one mask in one
    launch (usf_ar_transform_f32; sp_transforms.py:260-290): img1, img2
    [B,3,H,W], flow [B,2,H,W] (a channel slice is used in place), mask
    [B,1,H,W], theta [2,B,6] on the device, noise1 / noise2 None or [B,3,H,W]
    already scaled -> (img1_t, img2_t, flow_t, mask_t)."""
    for n, t in (("img1", img1), ("img2", img2), ("flow", flow), ("mask", mask), ("theta", theta)):
        _require_device_f32(n, t)
    B, C, H, W = _nchw("img1", img1)
    if C != 3 or tuple(img2.shape) != (B, 3, H, W):
        raise ValueError(f"img1 / img2 must be [B,3,H,W], got {tuple(img1.shape)} / {tuple(img2.shape)}")
    if H < 2 or W < 2:
        raise ValueError(f"the spatial transform needs H, W >= 2, got {(H, W)}")
    if tuple(mask.shape) != (B, 1, H, W):
        raise ValueError(f"mask {tuple(mask.shape)} does not match {(B, 1, H, W)}")
    if tuple(theta.shape) != (2, B, 6):
        raise ValueError(f"theta must be [2,B,6] = {(2, B, 6)}, got {tuple(theta.shape)}")
    dev = img1.device
    noise = []
    for n, t in (("noise1", noise1), ("noise2", noise2)):
        if t is not None:
            _require_device_f32(n, t)
            if tuple(t.shape) != (B, 3, H, W):
                raise ValueError(f"{n} {tuple(t.shape)} does not match {(B, 3, H, W)}")
            t = _dense16(t)
        noise.append(t)
    if any(t.device != dev for t in (img2, flow, mask, theta) + tuple(t for t in noise if t is not None)):
        raise ValueError("the spatial transform's tensors are on different devices")
    a, b_, m, th = _dense16(img1), _dense16(img2), _dense16(mask), theta.contiguous()
    fv, fbs = _flow_view(flow, B, H, W)
    outs = (torch.empty_like(a), torch.empty_like(b_), torch.empty((B, 2, H, W), device=dev, dtype=torch.float32),
            torch.empty_like(m))
    lib = _lib.load()
    # algorithmic bytes: 9 planes in and out, plus the noise planes read
    nbytes = 4 * B * H * W * (18 + 3 * sum(t is not None for t in noise))
    _args = (a.data_ptr(), b_.data_ptr(), fv.data_ptr(), fbs, m.data_ptr(), th.data_ptr(), _ptr(noise[0]),
             _ptr(noise[1]), *[t.data_ptr() for t in outs], B, H, W, _lib.stream_handle(dev),)
    with torch.cuda.device(dev), _kt.timed("ar_transform", (B, H, W, noise[0] is not None), dev, nbytes):
        rc = lib.usf_ar_transform_f32(*_args)
    _lib.check(rc, "usf_ar_transform_f32")
    return outs


def _ar_strided(name: str, t: torch.Tensor, shape) -> tuple[torch.Tensor, tuple]:
    """(batch, channel, row) strides of a [B,K,H,W] view with unit column stride
    -- what usf_ar_loss_* can address in place (a crop or channel slice, an
    expanded mask). Any other layout is refused, never copied silently."""
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a tensor of shape {tuple(shape)}, got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    s = t.stride()
    if s[3] != 1:
        raise ValueError(f"{name} has column stride {s[3]}: the AR loss entries take batch, channel and row strides "
                         "with unit column stride (make it contiguous first)")
    return t, (s[0], s[1], s[2])


def _ar_loss_args(pred, target, noc, eps, q):
    B, K, H, W = _nchw("pred", pred)
    if K != 2:
        raise ValueError(f"pred must be [B,2,H,W], got {tuple(pred.shape)}")
    if not q > 0 or not eps >= 0:
        raise ValueError(f"the AR loss needs q > 0 and eps >= 0, got q={q} eps={eps}")
    target, ts = _ar_strided("target", target, (B, 2, H, W))
    noc, ns = _ar_strided("noc", noc, (B, 1, H, W))
    for n, t in (("pred", pred), ("target", target), ("noc", noc)):
        _require_device_f32(n, t)
    if target.device != pred.device or noc.device != pred.device:
        raise ValueError("pred, target and noc are on different devices")
    return pred.contiguous(), target, ts, noc, (ns[0], ns[2]), B, H, W


def ar_loss_forward(pred, target, noc, eps: float = 0.0, q: float = 1.0, denom=None):
    """``(((pred - target).abs() + eps) ** q * noc).mean() / (D + 1e-7)`` with D =
    ``noc.mean()`` or the device scalar ``denom`` (kitti_trainer_ar.py:169-172)
    -> out [2] on the device = {loss, c} (c: what the backward needs). target
    [B,2,H,W] and noc [B,1,H,W] may be strided views with unit column stride."""
    p, t, ts, n, ns, B, H, W = _ar_loss_args(pred, target, noc, eps, q)
    dev = p.device
    if denom is not None:
        _require_device_f32("denom", denom)
        if denom.numel() != 1 or denom.device != dev:
            raise ValueError("denom must be one float32 element on pred's device")
        denom = denom.reshape(1)
    lib = _lib.load()
    partials = torch.empty(lib.usf_ar_loss_partials(B, H, W), device=dev, dtype=torch.float32)
    out = torch.empty(2, device=dev, dtype=torch.float32)
    _args = (p.data_ptr(), t.data_ptr(), *ts, n.data_ptr(), *ns, _ptr(denom), partials.data_ptr(), out.data_ptr(),
             B, H, W, float(eps), float(q), _lib.stream_handle(dev),)
    # algorithmic bytes: pred and target (2 planes each) and noc read once
    with torch.cuda.device(dev), _kt.timed("ar_loss_fwd", (B, H, W, float(q)), dev, 4 * B * H * W * 5):
        rc = lib.usf_ar_loss_fwd_f32(*_args)
    _lib.check(rc, "usf_ar_loss_fwd_f32")
    return out


def ar_loss_backward(pred, target, noc, coef, grad_loss, eps: float = 0.0, q: float = 1.0):
    """d(AR loss)/d(pred) * grad_loss, recomputed from the forward's inputs in one
    dense pass (coef = :func:`ar_loss_forward`'s out) -> [B,2,H,W]; sign(0) = 0."""
    p, t, ts, n, ns, B, H, W = _ar_loss_args(pred, target, noc, eps, q)
    dev = p.device
    _require_device_f32("coef", coef)
    gl = grad_loss.reshape(-1).to(torch.float32).contiguous()
    if gl.numel() != 1 or coef.numel() != 2:
        raise ValueError(f"grad_loss / coef have {gl.numel()} / {coef.numel()} elements (1 / 2)")
    coef = coef.contiguous()
    gpred = torch.empty_like(p)
    lib = _lib.load()
    _args = (p.data_ptr(), t.data_ptr(), *ts, n.data_ptr(), *ns, coef.data_ptr(), gl.data_ptr(), gpred.data_ptr(),
             B, H, W, float(eps), float(q), _lib.stream_handle(dev),)
    with torch.cuda.device(dev), _kt.timed("ar_loss_bwd", (B, H, W, float(q)), dev, 4 * B * H * W * 7):
        rc = lib.usf_ar_loss_bwd_f32(*_args)
    _lib.check(rc, "usf_ar_loss_bwd_f32")
    return gpred


def _fakeobj_cache(cache_mask, cache_img, H, W):
    _require_device_f32("cache_mask", cache_mask)
    _require_device_f32("cache_img", cache_img)
    n = cache_mask.shape[0] if cache_mask.dim() == 4 else 0
    if n < 1 or tuple(cache_mask.shape) != (n, 1, H, W) or tuple(cache_img.shape) != (n, 3, H, W):
        raise ValueError(f"cache_mask / cache_img must be [N,1,{H},{W}] / [N,3,{H},{W}], got "
                         f"{tuple(cache_mask.shape)} / {tuple(cache_img.shape)}")
    if not cache_mask.is_contiguous() or not cache_img.is_contiguous():
        raise ValueError("the object cache must be contiguous (it is addressed in place)")
    return n


def _fakeobj_table(name, t, shape, dtype, device):
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device
            or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {dtype} {tuple(shape)} tensor on {device}")


def fakeobj_paste_crop(img1, img2, flow, noc, cache_mask, cache_img, cache_motion, slots, params, crop_sz, offsets):
    """K rounds of add_fake_object on objects read in place from the device
    cache, then the crop, in one launch (usf_fakeobj_paste_crop_f32). img1, img2
    [B,3,H,W], flow [B,2,H,W] (a channel slice is used in place), noc [B,1,H,W];
    slots [K*B] int32 and params [K*B,4] float32 (sx, sy, flip, 0: the factors
    on the slot's cached motion and the x mirror) on the device; crop_sz = (ch, cw), offsets = (y0, x0) -> (imgs_ot [B,6,ch,cw], flow_ot
    [B,2,ch,cw], noc_ot [B,1,ch,cw])."""
    for n, t in (("img1", img1), ("img2", img2), ("flow", flow), ("noc", noc), ("cache_motion", cache_motion)):
        _require_device_f32(n, t)
    B, C, H, W = _nchw("img1", img1)
    if C != 3 or tuple(img2.shape) != (B, 3, H, W):
        raise ValueError(f"img1 / img2 must be [B,3,H,W], got {tuple(img1.shape)} / {tuple(img2.shape)}")
    if H < 2 or W < 2:
        raise ValueError(f"the object insertion needs H, W >= 2, got {(H, W)}")
    if tuple(noc.shape) != (B, 1, H, W):
        raise ValueError(f"noc {tuple(noc.shape)} does not match {(B, 1, H, W)}")
    dev = img1.device
    size = _fakeobj_cache(cache_mask, cache_img, H, W)
    _fakeobj_table("cache_motion", cache_motion, (size, 2), torch.float32, dev)
    n = slots.numel() if isinstance(slots, torch.Tensor) else 0
    K = n // B
    if n != K * B or not 1 <= K <= _lib.FAKEOBJ_MAX_K:
        raise ValueError(f"slots must hold K*B entries with 1 <= K <= {_lib.FAKEOBJ_MAX_K}, got {n} for B={B}")
    _fakeobj_table("slots", slots, (n,), torch.int32, dev)
    _fakeobj_table("params", params, (n, 4), torch.float32, dev)
    (ch, cw), (y0, x0) = (int(v) for v in crop_sz), (int(v) for v in offsets)
    if y0 < 0 or x0 < 0 or ch < 1 or cw < 1 or y0 + ch > H or x0 + cw > W:
        raise ValueError(f"crop {(ch, cw)} at {(y0, x0)} lies outside the image {(H, W)}")
    if any(t.device != dev for t in (img2, flow, noc, cache_mask, cache_img)):
        raise ValueError("the object insertion's tensors are on different devices")
    a, b_, nc = _dense16(img1), _dense16(img2), _dense16(noc)
    fv, fbs = _flow_view(flow, B, H, W)
    outs = (torch.empty((B, 6, ch, cw), device=dev, dtype=torch.float32),
            torch.empty((B, 2, ch, cw), device=dev, dtype=torch.float32),
            torch.empty((B, 1, ch, cw), device=dev, dtype=torch.float32))
    lib = _lib.load()
    # algorithmic bytes: 9 base planes in and out; per object 4 floats at the pixel and 4 at the shifted position
    nbytes = 4 * B * ch * cw * (18 + 8 * K)
    _args = (a.data_ptr(), b_.data_ptr(), fv.data_ptr(), fbs, nc.data_ptr(), cache_mask.data_ptr(),
             cache_img.data_ptr(), cache_motion.data_ptr(), slots.data_ptr(), params.data_ptr(),
             *[t.data_ptr() for t in outs], B, H, W, K, size, y0, x0, ch, cw, _lib.stream_handle(dev),)
    with torch.cuda.device(dev), _kt.timed("fakeobj_paste_crop", (B, H, W, K, ch, cw), dev, nbytes):
        rc = lib.usf_fakeobj_paste_crop_f32(*_args)
    _lib.check(rc, "usf_fakeobj_paste_crop_f32")
    return outs


def fakeobj_push(obj_mask, img, flow, slots, cache_mask, cache_img, cache_motion):
    """Copy every sample b with slots[b] >= 0 into its cache slot and write its
    masked mean flow into cache_motion (usf_fakeobj_push_f32; deterministic).
    obj_mask [B,1,H,W], img [B,3,H,W], flow [B,2,H,W] (a channel slice is used in
    place), slots [B] int32 on the device (-1: skip the sample); the cache
    tensors are written in place."""
    for n, t in (("obj_mask", obj_mask), ("img", img), ("flow", flow), ("cache_motion", cache_motion)):
        _require_device_f32(n, t)
    B, C, H, W = _nchw("img", img)
    if C != 3 or tuple(obj_mask.shape) != (B, 1, H, W):
        raise ValueError(f"obj_mask / img must be [B,1,H,W] / [B,3,H,W], got {tuple(obj_mask.shape)} / "
                         f"{tuple(img.shape)}")
    if H < 2 or W < 2:
        raise ValueError(f"the object cache needs H, W >= 2, got {(H, W)}")
    dev = img.device
    size = _fakeobj_cache(cache_mask, cache_img, H, W)
    _fakeobj_table("cache_motion", cache_motion, (size, 2), torch.float32, dev)
    _fakeobj_table("slots", slots, (B,), torch.int32, dev)
    if any(t.device != dev for t in (obj_mask, flow, cache_mask, cache_img)):
        raise ValueError("the object cache's tensors are on different devices")
    m, im = _dense16(obj_mask), _dense16(img)
    fv, fbs = _flow_view(flow, B, H, W)
    lib = _lib.load()
    partials = torch.empty(lib.usf_fakeobj_push_partials(B, H, W), device=dev, dtype=torch.float32)
    # algorithmic bytes: mask and frame read and written once, the flow read once
    nbytes = 4 * B * H * W * (4 + 2 + 4)
    _args = (m.data_ptr(), im.data_ptr(), fv.data_ptr(), fbs, slots.data_ptr(), cache_mask.data_ptr(),
             cache_img.data_ptr(), cache_motion.data_ptr(), partials.data_ptr(), B, H, W, size,
             _lib.stream_handle(dev),)
    with torch.cuda.device(dev), _kt.timed("fakeobj_push", (B, H, W), dev, nbytes):
        rc = lib.usf_fakeobj_push_f32(*_args)
    _lib.check(rc, "usf_fakeobj_push_f32")


def _eval_args(pred, sizes, Hmax, Wmax):
    """Checks shared by the two evaluation entries -> (prediction view, its batch
    stride, B, h, w, size table or None)."""
    _require_device_f32("pred", pred)
    B, C, h, w = _nchw("pred", pred)
    if C != 2 or h < 2 or w < 2 or Hmax < 2 or Wmax < 2:
        raise ValueError(f"pred must be [B,2,h,w] with h, w >= 2 and the target at least 2x2, got {tuple(pred.shape)} "
                         f"-> {(Hmax, Wmax)}")
    if sizes is not None:
        _fakeobj_table("sizes", sizes, (B, 2), torch.int32, pred.device)
    pv, pbs = _flow_view(pred, B, h, w)
    return pv, pbs, B, h, w, sizes


def flow_resize(pred, sizes, Hmax: int, Wmax: int, out=None):
    """resize_flow (utils/flow_utils.py:62-71) to a size of its own per sample
    (usf_flow_resize_f32). pred [B,2,h,w] (a channel slice is used in place);
    sizes [B,2] int32 (H_b, W_b) on the device, or None: every sample is
    (Hmax, Wmax). -> out [B,2,Hmax,Wmax]: sample b's window [0,H_b) x [0,W_b) is
    written, the rest keeps what ``out`` held (zeros when allocated here)."""
    Hmax, Wmax = int(Hmax), int(Wmax)
    pv, pbs, B, h, w, sizes = _eval_args(pred, sizes, Hmax, Wmax)
    dev = pred.device
    if out is None:
        alloc = torch.empty if sizes is None else torch.zeros
        out = alloc((B, 2, Hmax, Wmax), device=dev, dtype=torch.float32)
    else:
        _check_out("out", out, (B, 2, Hmax, Wmax), dev)
    lib = _lib.load()
    _args = (pv.data_ptr(), pbs, _ptr(sizes), out.data_ptr(), B, h, w, Hmax, Wmax, _lib.stream_handle(dev),)
    # algorithmic bytes: the prediction read once, the output written once
    with torch.cuda.device(dev), _kt.timed("flow_resize", (B, h, w, Hmax, Wmax), dev,
                                           4 * B * 2 * (h * w + Hmax * Wmax)):
        rc = lib.usf_flow_resize_f32(*_args)
    _lib.check(rc, "usf_flow_resize_f32")
    return out


def flow_eval(pred, gt, sizes=None, move=None):
    """The error sums and metrics of evaluate_flow (flow_utils.py:117-201) for a
    batch of ragged ground truths (usf_flow_eval_f32; deterministic). pred
    [B,2,h,w] (a channel slice is used in place); gt [B,Cg,Hmax,Wmax] planar,
    Cg = 2 or 4 (u, v, valid, noc); sizes [B,2] int32 on the device or None;
    move [B,1,Hmax,Wmax] or None -> (metrics [B,7], sums [B,12])."""
    _require_device_f32("gt", gt)
    Bg, Cg, Hmax, Wmax = _nchw("gt", gt)
    pv, pbs, B, h, w, sizes = _eval_args(pred, sizes, Hmax, Wmax)
    dev = pred.device
    if Bg != B or Cg not in (2, 4) or gt.device != dev:
        raise ValueError(f"gt must be [{B},2 or 4,H,W] on {dev}, got {tuple(gt.shape)} on {gt.device}")
    g = _dense16(gt)
    m = None
    if move is not None:
        _require_device_f32("move", move)
        if tuple(move.shape) != (B, 1, Hmax, Wmax) or move.device != dev:
            raise ValueError(f"move {tuple(move.shape)} does not match {(B, 1, Hmax, Wmax)} on {dev}")
        m = _dense16(move)
    lib = _lib.load()
    # scratch of one row per workgroup: no initialisation needed, one per shape and device
    with torch.cuda.device(dev):
        partials = persistent_workspace(dev, "flow_eval", (B, Hmax, Wmax),
                                        4 * lib.usf_flow_eval_partials(B, Hmax, Wmax))
    metrics = torch.empty((B, _lib.EVAL_NMETRIC), device=dev, dtype=torch.float32)
    sums = torch.empty((B, _lib.EVAL_NACC), device=dev, dtype=torch.float32)
    _args = (pv.data_ptr(), pbs, g.data_ptr(), Cg, _ptr(m), _ptr(sizes), partials.data_ptr(), sums.data_ptr(),
             metrics.data_ptr(), B, h, w, Hmax, Wmax, _lib.stream_handle(dev),)
    # algorithmic bytes: every ground-truth plane and the move mask read once, the prediction once
    nbytes = 4 * B * ((Cg + (m is not None)) * Hmax * Wmax + 2 * h * w)
    with torch.cuda.device(dev), _kt.timed("flow_eval", (B, Cg, h, w, Hmax, Wmax, m is not None), dev, nbytes):
        rc = lib.usf_flow_eval_f32(*_args)
    _lib.check(rc, "usf_flow_eval_f32")
    return metrics, sums


def _segpool_args(proj, seg, num_segments):
    _require_device_f32("proj", proj)
    _require_device_f32("seg", seg)
    B, C, H, W = _nchw("proj", proj)
    if tuple(seg.shape) != (B, 1, H, W):
        raise ValueError(f"seg must be [B,1,h,w] = {(B, 1, H, W)}, got {tuple(seg.shape)}")
    if seg.device != proj.device:
        raise ValueError("proj and seg are on different devices")
    K = int(num_segments)
    if not 1 <= K <= _lib.SEGPOOL_MAX_K:
        raise ValueError(f"num_segments={K} outside [1, {_lib.SEGPOOL_MAX_K}] (USF_SEGPOOL_MAX_K)")
    return _dense16(proj), _dense16(seg), B, C, H, W, K


def segpool_forward(proj, seg, num_segments: int):
    """Per-segment max pool and spread (pwclite.py:317-357): ``spread[b,c,p] =
    pooled[b,c,seg[b,p]]`` with ``pooled = amax(one_hot(seg) * proj[..., None],
    dim=(2, 3))``. proj [B,C,h,w]; seg [B,1,h,w] fp32 integer ids in
    [0, num_segments) -> (spread [B,C,h,w], state), the int32 tables (maxima,
    pixel counts) :func:`segpool_backward` reads."""
    p, s, B, C, H, W, K = _segpool_args(proj, seg, num_segments)
    dev = p.device
    lib = _lib.load()
    state = torch.empty(lib.usf_segpool_state_words(B, C, K), device=dev, dtype=torch.int32)
    spread = torch.empty_like(p)
    _args = (p.data_ptr(), s.data_ptr(), spread.data_ptr(), state.data_ptr(), B, C, H, W, K,
             _lib.stream_handle(dev),)
    # algorithmic bytes: proj and seg read once, spread written
    with torch.cuda.device(dev), _kt.timed("segpool_fwd", (B, C, H, W, K), dev, B * H * W * (8 * C + 4)):
        rc = lib.usf_segpool_fwd_f32(*_args)
    _lib.check(rc, "usf_segpool_fwd_f32")
    return spread, state


def segpool_backward(proj, seg, state, grad_spread, num_segments: int):
    """d(spread)/d(proj) applied to ``grad_spread`` -> [B,C,h,w]: a segment's
    summed gradient shared evenly among the positions equal to its pooled value
    (the one-hot product's zeros outside the segment included)."""
    p, s, B, C, H, W, K = _segpool_args(proj, seg, num_segments)
    dev = p.device
    _require_device_f32("grad_spread", grad_spread)
    if tuple(grad_spread.shape) != (B, C, H, W) or grad_spread.device != dev:
        raise ValueError(f"grad_spread {tuple(grad_spread.shape)} does not match proj {(B, C, H, W)}")
    lib = _lib.load()
    if (state.dtype != torch.int32 or state.device != dev or not state.is_contiguous()
            or state.numel() != lib.usf_segpool_state_words(B, C, K)):
        raise ValueError("state is not the forward's table buffer for this shape")
    g = _dense16(grad_spread)
    gproj = torch.empty_like(p)
    _args = (p.data_ptr(), s.data_ptr(), state.data_ptr(), g.data_ptr(), gproj.data_ptr(), B, C, H, W, K,
             _lib.stream_handle(dev),)
    # algorithmic bytes: proj, grad_spread and seg read once, grad_proj written
    with torch.cuda.device(dev), _kt.timed("segpool_bwd", (B, C, H, W, K), dev, B * H * W * (12 * C + 8)):
        rc = lib.usf_segpool_bwd_f32(*_args)
    _lib.check(rc, "usf_segpool_bwd_f32")
    return gproj


def _hg_args(flow, seg):
    fv, fbs, B, H, W = _flow_arg(flow, "flow")
    _require_device_f32("full_seg", seg)
    if tuple(seg.shape) != (B, 1, H, W) or seg.device != fv.device:
        raise ValueError(f"full_seg must be [B,1,h,w] = {(B, 1, H, W)} on {fv.device}, got {tuple(seg.shape)}")
    return fv, fbs, _dense16(seg), B, H, W


def _hg_records(records, B, dev):
    if (not isinstance(records, torch.Tensor) or records.dtype != torch.int32 or records.device != dev
            or tuple(records.shape) != (B, _lib.HG_SLOTS, _lib.HG_RECORD_WORDS) or not records.is_contiguous()):
        raise ValueError(f"records must be the contiguous int32 [{B},{_lib.HG_SLOTS},{_lib.HG_RECORD_WORDS}] "
                         f"tensor of hg_fit on {dev}")
    return records


def hg_fit(flow, seg, occ, num_segments: int, thr: float, n_hyp: int = _lib.HG_DEFAULT_HYP, seed: int = 0):
    """Select the six segments per sample and fit their homographies by RANSAC
    (include/unsamflow_hip_hg.h; loss_blocks.py:125-178). flow [B,2,h,w] (a
    channel slice of a [B,4,h,w] tensor is read in place); seg, occ [B,1,h,w]
    fp32 -> records, int32 [B, 6, 16] (id, status, n_seg, n_rel, n_inl, H as
    float bits, best_j, list offset). No host sync."""
    fv, fbs, s, B, H, W = _hg_args(flow, seg)
    dev = fv.device
    _require_device_f32("occ_mask", occ)
    if tuple(occ.shape) != (B, 1, H, W) or occ.device != dev:
        raise ValueError(f"occ_mask must be [B,1,h,w] = {(B, 1, H, W)} on {dev}, got {tuple(occ.shape)}")
    o = _dense16(occ)
    K, n_hyp = int(num_segments), int(n_hyp)
    if not 1 <= K <= _lib.HG_MAX_K:
        raise ValueError(f"num_segments={K} outside [1, {_lib.HG_MAX_K}] (USF_HG_MAX_K)")
    lib = _lib.load()
    nbytes = lib.usf_hg_workspace_bytes(B, H, W, K, n_hyp)
    if nbytes <= 0:
        raise ValueError(f"hg_fit: bad arguments B={B} H={H} W={W} K={K} n_hyp={n_hyp}")
    ws = torch.empty(nbytes // 8, device=dev, dtype=torch.int64)
    records = torch.empty((B, _lib.HG_SLOTS, _lib.HG_RECORD_WORDS), device=dev, dtype=torch.int32)
    _args = (fv.data_ptr(), fbs, s.data_ptr(), o.data_ptr(), K, float(thr), n_hyp, int(seed) & (2 ** 64 - 1),
             records.data_ptr(), ws.data_ptr(), nbytes, B, H, W, _lib.stream_handle(dev),)
    # algorithmic bytes: seg and occ read for the statistics and the lists, flow for the pairs
    with torch.cuda.device(dev), _kt.timed("hg_fit", (B, H, W, K, n_hyp), dev, B * H * W * 24):
        rc = lib.usf_hg_fit_f32(*_args)
    _lib.check(rc, "usf_hg_fit_f32")
    return records


def hg_loss_forward(flow, seg, records):
    """The homography smoothness loss of given records -> a 0-d tensor: the L1
    distance of ``p + flow`` to ``dehom(H p)`` over the accepted slots' segments
    / (h * w * B) (loss_blocks.py:179-200)."""
    fv, fbs, s, B, H, W = _hg_args(flow, seg)
    dev = fv.device
    _hg_records(records, B, dev)
    lib = _lib.load()
    partials = torch.empty(lib.usf_hg_loss_partials(B, H, W), device=dev, dtype=torch.float64)
    out = torch.empty(1, device=dev, dtype=torch.float32)
    _args = (fv.data_ptr(), fbs, s.data_ptr(), records.data_ptr(), partials.data_ptr(), out.data_ptr(), B, H, W,
             _lib.stream_handle(dev),)
    with torch.cuda.device(dev), _kt.timed("hg_loss_fwd", (B, H, W), dev, B * H * W * 12):
        rc = lib.usf_hg_loss_fwd_f32(*_args)
    _lib.check(rc, "usf_hg_loss_fwd_f32")
    return out[0]


def hg_loss_backward(flow, seg, records, grad_loss):
    """d(hg_loss_forward)/d(flow) applied to the 0-d ``grad_loss`` -> [B,2,h,w]:
    ``-sign(diff) * grad_loss / (h * w * B)`` on the accepted slots' segments."""
    fv, fbs, s, B, H, W = _hg_args(flow, seg)
    dev = fv.device
    _hg_records(records, B, dev)
    _require_device_f32("grad_loss", grad_loss)
    if grad_loss.numel() != 1 or grad_loss.device != dev:
        raise ValueError("grad_loss must be one float32 on the flow's device")
    g = grad_loss.contiguous()
    gflow = torch.empty((B, 2, H, W), device=dev, dtype=torch.float32)
    _args = (fv.data_ptr(), fbs, s.data_ptr(), records.data_ptr(), g.data_ptr(), gflow.data_ptr(), B, H, W,
             _lib.stream_handle(dev),)
    with torch.cuda.device(dev), _kt.timed("hg_loss_bwd", (B, H, W), dev, B * H * W * 20):
        rc = _lib.load().usf_hg_loss_bwd_f32(*_args)
    _lib.check(rc, "usf_hg_loss_bwd_f32")
    return gflow


def device_errors(device, clear: bool = True) -> int:
    """The USF_DEVERR_* flags kernels raised on ``device``'s current stream since
    the last clear (usf_device_errors; synchronises the stream)."""
    with torch.cuda.device(device):
        v = _lib.load().usf_device_errors(_lib.stream_handle(torch.device(device)), 1 if clear else 0)
    if v < 0:
        _lib.check(v, "usf_device_errors")
    return v


def _plane_slice_stride(name: str, t: torch.Tensor, shape) -> int:
    """Batch stride of a [B,K,H,W] channel slice whose per-sample planes are dense."""
    B, K, H, W = shape
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} shape {tuple(t.shape)} != {tuple(shape)}")
    s = t.stride()
    if s[1] != H * W or s[2] != W or s[3] != 1 or (B > 1 and s[0] < K * H * W):
        raise ValueError(f"{name} must be a channel slice of an NCHW-contiguous tensor (strides {s})")
    return s[0] if B > 1 else K * H * W


def corr_act_mask(B: int, H: int, W: int, max_displacement: int, device, C: int | None = None
                  ) -> torch.Tensor | None:
    """An empty LeakyReLU sign mask for :func:`corr_forward_ex` (int64 words,
    [B,2d+1,H,ceil(W/4)]), at every level: the unsplit forward writes it in its
    epilogue, the channel-split forward of the small levels in its reduce.
    ``C`` is accepted for call-site compatibility (the mask no longer depends
    on it)."""
    lib = _lib.load()
    n = int(lib.usf_corr_act_mask_words(B, H, W, int(max_displacement)))
    if n == 0:
        return None
    return torch.empty((B, 2 * int(max_displacement) + 1, H, (W + 3) // 4), device=device, dtype=torch.int64)


def corr_forward_ex(x1: torch.Tensor, x2: torch.Tensor, max_displacement: int, out: torch.Tensor,
                    leaky_slope: float | None = None, act_mask: torch.Tensor | None = None) -> torch.Tensor:
    """:func:`corr_forward` into ``out``, a [B,(2d+1)^2,H,W] channel slice of a
    larger NCHW buffer (the flow estimator's concat input), with the decoder's
    LeakyReLU applied in the kernel epilogue when ``leaky_slope`` is given; with
    ``act_mask`` (:func:`corr_act_mask`) the epilogue also writes the output's
    sign bits for :func:`corr_backward_ex`."""
    _require_device_f32("input1", x1)
    _require_device_f32("input2", x2)
    _require_device_f32("output", out)
    B, C, H, W = _nchw("input1", x1)
    if x2.shape != x1.shape:
        raise ValueError(f"input2 shape {tuple(x2.shape)} != input1 shape {tuple(x1.shape)}")
    d = int(max_displacement)
    K = 2 * d + 1
    obs = _plane_slice_stride("output", out, (B, K * K, H, W))
    if out.data_ptr() % (16 if H * W % 4 == 0 else 4):
        raise ValueError("output must be a channel slice of a 16-byte aligned NCHW buffer")
    x1c, x2c = _dense16(x1), _dense16(x2)
    lib = _lib.load()
    act = 0 if leaky_slope is None else 1
    if act_mask is not None:
        if act == 0 or act_mask.dtype != torch.int64 or not act_mask.is_contiguous() \
                or act_mask.numel() != int(lib.usf_corr_act_mask_words(B, H, W, d)):
            raise ValueError("act_mask: a contiguous int64 corr_act_mask() tensor with leaky_slope set")
    ws, nws = _corr_workspace(lib, B, C, H, W, d, x1.device)
    # the decoder's site (LeakyReLU epilogue into the concat slice, + the sign mask)
    # is its own timing site, so its device time is measured on the same call
    op = "corr_fwd_leaky" if act else "corr_fwd"
    nbytes = _kt.corr_bytes(B, C, H, W, K * K) + (8 * act_mask.numel() if act_mask is not None else 0)
    _args = (x1c.data_ptr(), x2c.data_ptr(), out.data_ptr(), obs, act, float(leaky_slope or 0.0), _ptr(act_mask),
             ws.data_ptr() if nws else None, nws, B, C, H, W, d, _lib.stream_handle(x1.device),)
    with torch.cuda.device(x1.device), _kt.timed(
        op, (B, C, H, W), x1.device, nbytes, _kt.corr_flops(B, C, H, W, K * K)
    ):
        rc = lib.usf_corr_fwd_ex_f32(*_args)
    _lib.check(rc, "usf_corr_fwd_ex_f32")
    return out


def corr_backward_ex(x1: torch.Tensor, x2: torch.Tensor, grad_out: torch.Tensor, max_displacement: int,
                     need_x1: bool = True, need_x2: bool = True, act_out: torch.Tensor | None = None,
                     leaky_slope: float = 0.1, act_mask: torch.Tensor | None = None,
                     ) -> tuple[torch.Tensor | None, torch.Tensor | None]:
    """:func:`corr_backward` reading ``grad_out`` as a channel slice of the concat
    gradient; with ``act_out`` (the forward's activated slice) the LeakyReLU
    derivative is applied first (one dense pass into a scratch); with
    ``act_mask`` (the forward's sign mask) it is applied inside the backward
    kernel's gradient loads instead, and ``act_out`` is not read."""
    _require_device_f32("input1", x1)
    _require_device_f32("input2", x2)
    _require_device_f32("grad_output", grad_out)
    B, C, H, W = _nchw("input1", x1)
    d = int(max_displacement)
    K = 2 * d + 1
    gbs = _plane_slice_stride("grad_output", grad_out, (B, K * K, H, W))
    scratch = None
    lib = _lib.load()
    if act_mask is not None:
        if act_mask.dtype != torch.int64 or not act_mask.is_contiguous() \
                or act_mask.numel() != int(lib.usf_corr_act_mask_words(B, H, W, d)):
            raise ValueError("act_mask: the forward's contiguous int64 corr_act_mask() tensor")
        act_out = None
    elif act_out is not None:
        _require_device_f32("act_out", act_out)
        if _plane_slice_stride("act_out", act_out, (B, K * K, H, W)) != gbs:
            raise ValueError("act_out and grad_output must share the batch stride")
        n = int(lib.usf_corr_bwd_ex_scratch(B, C, H, W, d))
        if n:
            scratch = torch.empty(n, device=x1.device, dtype=torch.float32)
    if not (need_x1 or need_x2):
        return None, None
    x1c, x2c = _dense16(x1), _dense16(x2)
    g1 = torch.empty_like(x1c) if need_x1 else None
    g2 = torch.empty_like(x2c) if need_x2 else None
    # with the LeakyReLU derivative the site also reads the activated output
    # once (what leaky_relu_backward needs): a distinct site, its bytes included
    # (with the sign mask instead: its words are the derivative's input)
    op = "corr_bwd" if act_out is None and act_mask is None else "corr_bwd_leaky"
    nbytes = _kt.corr_bytes(B, C, H, W, K * K, True, need_x1, need_x2)
    if act_out is not None:
        nbytes += 4 * B * H * W * K * K
    elif act_mask is not None:
        nbytes += 8 * act_mask.numel()
    _args = (x1c.data_ptr(), x2c.data_ptr(), grad_out.data_ptr(), gbs, _ptr(act_out), _ptr(act_mask),
             float(leaky_slope), _ptr(scratch), _ptr(g1), _ptr(g2), B, C, H, W, d, _lib.stream_handle(x1.device),)
    with torch.cuda.device(x1.device), _kt.timed(
        op, (B, C, H, W, need_x1, need_x2), x1.device, nbytes,
        _kt.corr_flops(B, C, H, W, K * K, True, need_x1, need_x2),
    ):
        rc = lib.usf_corr_bwd_ex_f32(*_args)
    _lib.check(rc, "usf_corr_bwd_ex_f32")
    return g1, g2


def flow_upsample(flow: torch.Tensor, factor: int) -> torch.Tensor:
    """F.interpolate(flow * factor, scale_factor=factor, mode="bilinear", align_corners=True)."""
    _require_device_f32("flow", flow)
    B, C, H, W = _nchw("flow", flow)
    k = int(factor)
    fc = _dense16(flow)
    out = torch.empty((B, C, H * k, W * k), device=flow.device, dtype=torch.float32)
    lib = _lib.load()
    _args = (fc.data_ptr(), out.data_ptr(), B, C, H, W, k, _lib.stream_handle(flow.device),)
    with torch.cuda.device(flow.device), _kt.timed("upsample", (B, C, H, W, k), flow.device,
                                                     4 * B * C * H * W * (1 + k * k)):
        rc = lib.usf_flow_upsample_f32(*_args)
    _lib.check(rc, "usf_flow_upsample_f32")
    return out


def warp_forward_up(x: torch.Tensor, coarse_flow: torch.Tensor, pad: str = "border") -> tuple[torch.Tensor, torch.Tensor]:
    """(up, out): up = F.interpolate(coarse_flow * 2, scale_factor=2, bilinear,
    align_corners=True) and out = flow_warp(x, up) (pwclite.py:299-302) in ONE
    launch (``usf_warp_fwd_up_f32``); the same numbers as :func:`flow_upsample`
    followed by :func:`warp_forward`."""
    _require_device_f32("x", x)
    _require_device_f32("coarse_flow", coarse_flow)
    B, C, H, W = _nchw("x", x)
    if pad not in PAD_MODES:
        raise NotImplementedError(f"flow_warp padding mode {pad!r} (supported: border, zeros)")
    if tuple(coarse_flow.shape) != (B, 2, H // 2, W // 2) or H % 2 or W % 2:
        raise ValueError(f"coarse flow shape {tuple(coarse_flow.shape)} is not [B,2,H/2,W/2] of x {(B, C, H, W)}")
    xc, fc = _dense16(x), _dense16(coarse_flow)
    up = torch.empty((B, 2, H, W), device=x.device, dtype=torch.float32)
    out = torch.empty_like(xc)
    lib = _lib.load()
    _args = (xc.data_ptr(), fc.data_ptr(), up.data_ptr(), out.data_ptr(), B, C, H, W, PAD_MODES[pad],
             _lib.stream_handle(x.device),)
    with torch.cuda.device(x.device), _kt.timed("warp_fwd_up", (B, C, H, W, pad), x.device,
                                                  _kt.warp_bytes(B, C, H, W) + 4 * B * 2 * (H // 2) * (W // 2)):
        rc = lib.usf_warp_fwd_up_f32(*_args)
    _lib.check(rc, "usf_warp_fwd_up_f32")
    return up, out


def flow_upsample_backward(grad_out: torch.Tensor, factor: int, grad_out2: torch.Tensor | None = None) -> torch.Tensor:
    """Backward of :func:`flow_upsample` for grad_out (+ grad_out2, summed per
    element inside the kernel: ``usf_flow_upsample_bwd_sum_f32``)."""
    _require_device_f32("grad_out", grad_out)
    B, C, Ho, Wo = _nchw("grad_out", grad_out)
    k = int(factor)
    if Ho % k or Wo % k:
        raise ValueError(f"grad_out spatial size {(Ho, Wo)} is not a multiple of {k}")
    H, W = Ho // k, Wo // k
    gc = _dense16(grad_out)
    gx = torch.empty((B, C, H, W), device=grad_out.device, dtype=torch.float32)
    lib = _lib.load()
    if grad_out2 is not None:
        _require_device_f32("grad_out2", grad_out2)
        if grad_out2.shape != grad_out.shape:
            raise ValueError(f"grad_out2 shape {tuple(grad_out2.shape)} != {tuple(grad_out.shape)}")
        g2 = _dense16(grad_out2)
        _args = (gc.data_ptr(), g2.data_ptr(), gx.data_ptr(), B, C, H, W, k, _lib.stream_handle(grad_out.device),)
        with torch.cuda.device(grad_out.device), _kt.timed("upsample_bwd", (B, C, H, W, k), grad_out.device,
                                                             4 * B * C * H * W * (1 + 2 * k * k)):
            rc = lib.usf_flow_upsample_bwd_sum_f32(*_args)
        _lib.check(rc, "usf_flow_upsample_bwd_sum_f32")
        return gx
    _args = (gc.data_ptr(), gx.data_ptr(), B, C, H, W, k, _lib.stream_handle(grad_out.device),)
    with torch.cuda.device(grad_out.device), _kt.timed("upsample_bwd", (B, C, H, W, k), grad_out.device,
                                                         4 * B * C * H * W * (1 + k * k)):
        rc = lib.usf_flow_upsample_bwd_f32(*_args)
    _lib.check(rc, "usf_flow_upsample_bwd_f32")
    return gx


def convex_upsample(flow: torch.Tensor, mask: torch.Tensor, factor: int = 4,
                    mask_scale: float = 0.25) -> torch.Tensor:
    """UpFlowNetwork.upsample_flow(flow, mask_scale * mask) (pwclite.py:148-166):
    flow [B,2,H,W], mask [B,9*f*f,H,W] (the convs' raw output) -> [B,2,fH,fW]."""
    _require_device_f32("flow", flow)
    _require_device_f32("mask", mask)
    B, C, H, W = _nchw("flow", flow)
    f = int(factor)
    if C != 2 or tuple(mask.shape) != (B, 9 * f * f, H, W):
        raise ValueError(f"convex_upsample: flow {tuple(flow.shape)} / mask {tuple(mask.shape)} (want [B,2,H,W] / "
                         f"[B,{9 * f * f},H,W])")
    fc, mc = _dense16(flow), _dense16(mask)
    out = torch.empty((B, 2, f * H, f * W), device=flow.device, dtype=torch.float32)
    lib = _lib.load()
    nbytes = 4 * B * H * W * (2 + 11 * f * f)
    _args = (fc.data_ptr(), mc.data_ptr(), out.data_ptr(), B, H, W, f, float(mask_scale),
             _lib.stream_handle(flow.device),)
    with torch.cuda.device(flow.device), _kt.timed("convex_up", (B, H, W, f), flow.device, nbytes):
        rc = lib.usf_convex_upsample_f32(*_args)
    _lib.check(rc, "usf_convex_upsample_f32")
    return out


def convex_upsample_backward(flow: torch.Tensor, mask: torch.Tensor, grad_out: torch.Tensor, factor: int = 4,
                             mask_scale: float = 0.25, need_flow: bool = True, need_mask: bool = True):
    """(grad_flow, grad_mask) of convex_upsample; grad_mask is w.r.t. the raw mask."""
    _require_device_f32("grad_out", grad_out)
    B, _, H, W = _nchw("flow", flow)
    f = int(factor)
    if tuple(grad_out.shape) != (B, 2, f * H, f * W):
        raise ValueError(f"convex_upsample_backward: grad_out {tuple(grad_out.shape)}")
    if not (need_flow or need_mask):
        return None, None
    fc, mc, gc = _dense16(flow), _dense16(mask), _dense16(grad_out)
    gf = torch.empty((B, 2, H, W), device=flow.device, dtype=torch.float32) if need_flow else None
    gm = torch.empty_like(mc) if need_mask else None
    lib = _lib.load()
    scratch = None
    if need_flow:
        scratch = torch.empty(int(lib.usf_convex_upsample_bwd_scratch(B, H, W)), device=flow.device,
                              dtype=torch.float32)
    nbytes = 4 * B * H * W * (2 + 9 * f * f + 2 * f * f + (2 if need_flow else 0) + (9 * f * f if need_mask else 0))
    _args = (fc.data_ptr(), mc.data_ptr(), gc.data_ptr(), _ptr(gf), _ptr(gm), _ptr(scratch), B, H, W, f,
             float(mask_scale), _lib.stream_handle(flow.device),)
    with torch.cuda.device(flow.device), _kt.timed("convex_up_bwd", (B, H, W, f), flow.device, nbytes):
        rc = lib.usf_convex_upsample_bwd_f32(*_args)
    _lib.check(rc, "usf_convex_upsample_bwd_f32")
    return gf, gm


def _level_sizes(flows):
    import ctypes

    return (_host_array(ctypes.c_int, [f.shape[2] for f in flows]),
            _host_array(ctypes.c_int, [f.shape[3] for f in flows]))


def convex_upsample_pyramid(flows, masks, factor: int = 4, mask_scale: float = 0.25):
    """:func:`convex_upsample` of every decoder level in one launch
    (usf_convex_upsample_pyramid_f32): flows [B,2,H_l,W_l], masks
    [B,9f^2,H_l,W_l] -> list of [B,2,fH_l,fW_l]; the same numbers as the
    per-level calls."""
    import ctypes

    n = len(flows)
    fl = [_dense16(f) for f in flows]
    mk = [_dense16(m) for m in masks]
    for f, m in zip(fl, mk):
        _require_device_f32("flow", f)
        _require_device_f32("mask", m)
    B, f_ = fl[0].shape[0], int(factor)
    outs = [torch.empty((B, 2, f_ * f.shape[2], f_ * f.shape[3]), device=f.device, dtype=torch.float32) for f in fl]
    Hs, Ws = _level_sizes(fl)
    lib = _lib.load()
    dev = fl[0].device
    key = (B,) + tuple(v for f in fl for v in f.shape[2:]) + (f_,)
    nbytes = sum(4 * B * f.shape[2] * f.shape[3] * (2 + 11 * f_ * f_) for f in fl)
    ptrs = lambda ts: _host_array(ctypes.c_void_p, [t.data_ptr() for t in ts])  # noqa: E731
    _args = (n, ptrs(fl), ptrs(mk), ptrs(outs), Hs, Ws, B, f_, float(mask_scale), _lib.stream_handle(dev),)
    with torch.cuda.device(dev), _kt.timed("convex_pyr", key, dev, nbytes):
        rc = lib.usf_convex_upsample_pyramid_f32(*_args)
    _lib.check(rc, "usf_convex_upsample_pyramid_f32")
    return outs


def convex_upsample_pyramid_backward(flows, masks, grad_outs, factor: int = 4, mask_scale: float = 0.25,
                                     need_flow: bool = True, need_mask: bool = True):
    """(grad_flows, grad_masks) lists of :func:`convex_upsample_pyramid` (None where not needed)."""
    import ctypes

    n = len(flows)
    fl = [_dense16(f) for f in flows]
    mk = [_dense16(m) for m in masks]
    go = [_dense16(g) for g in grad_outs]
    B, f_ = fl[0].shape[0], int(factor)
    if not (need_flow or need_mask):
        return None, None
    dev = fl[0].device
    gfs = [torch.empty((B, 2) + tuple(f.shape[2:]), device=dev, dtype=torch.float32) for f in fl] if need_flow else None
    gms = [torch.empty_like(m) for m in mk] if need_mask else None
    Hs, Ws = _level_sizes(fl)
    lib = _lib.load()
    nscr = int(lib.usf_convex_upsample_pyramid_bwd_scratch(n, Hs, Ws, B)) if need_flow else 0
    scratch = torch.empty(max(nscr, 1), device=dev, dtype=torch.float32)
    ptrs = lambda ts: _host_array(ctypes.c_void_p, [t.data_ptr() for t in ts])  # noqa: E731
    key = (B,) + tuple(v for f in fl for v in f.shape[2:]) + (f_,)
    ff = f_ * f_
    nbytes = sum(4 * B * f.shape[2] * f.shape[3] * (2 + 9 * ff + 2 * ff + (2 if need_flow else 0)
                                                    + (9 * ff if need_mask else 0)) for f in fl)
    _args = (n, ptrs(fl), ptrs(mk), ptrs(go), ptrs(gfs) if need_flow else None, ptrs(gms) if need_mask else None,
             scratch.data_ptr(), nscr, Hs, Ws, B, f_, float(mask_scale), _lib.stream_handle(dev),)
    with torch.cuda.device(dev), _kt.timed("convex_pyr_bwd", key, dev, nbytes):
        rc = lib.usf_convex_upsample_pyramid_bwd_f32(*_args)
    _lib.check(rc, "usf_convex_upsample_pyramid_bwd_f32")
    return gfs, gms


def area_pyramid(x: torch.Tensor):
    """The loss's image pyramid: ``[F.interpolate(x, (H >> s, W >> s), mode="area")
    for s in 1, 2, 3]`` (flow_loss.py:128-129), one read of x, bit-exact with
    torch's CPU kernel. x: [B,C,H,W] fp32 on the device, H and W multiples of 8."""
    _require_device_f32("x", x)
    B, C, H, W = _nchw("x", x)
    if H % 8 or W % 8:
        raise ValueError(f"area_pyramid needs H, W multiples of 8, got {H}x{W}")
    xc = _dense16(x)
    outs = [torch.empty((B, C, H >> s, W >> s), device=x.device, dtype=torch.float32) for s in (1, 2, 3)]
    lib = _lib.load()
    nbytes = 4 * B * C * H * W * (1 + 1 / 4 + 1 / 16 + 1 / 64)
    _args = (xc.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), B, C, H, W,
             _lib.stream_handle(x.device),)
    with torch.cuda.device(x.device), _kt.timed("area_pyramid", (B, C, H, W), x.device, int(nbytes)):
        rc = lib.usf_area_pyramid_f32(*_args)
    _lib.check(rc, "usf_area_pyramid_f32")
    return outs


def _conv_epi_args(y, bias, slope):
    _require_device_f32("y", y)
    _require_device_f32("bias", bias)
    B, C, H, W = _nchw("y", y)
    if not y.is_contiguous():
        raise ValueError(f"y must be dense NCHW (strides {y.stride()})")
    if y.data_ptr() % 16:
        raise ValueError("y must be 16-byte aligned (it is updated in place)")
    if tuple(bias.shape) != (C,) or bias.device != y.device:
        raise ValueError(f"bias must be [{C}] on {y.device}, got {tuple(bias.shape)} on {bias.device}")
    slope = float(slope)
    if not slope > 0.0:
        raise ValueError(f"slope={slope} must be > 0 (1 = no activation)")
    return B, C, H, W, slope


def conv_epilogue_forward(raw: torch.Tensor, bias: torch.Tensor, slope: float = 1.0) -> torch.Tensor:
    """In place on ``raw`` [B,C,H,W] (a bias-free convolution's output):
    ``raw = leaky_relu(raw + bias[c], slope)``, bit-identical to ``add_`` then
    ``leaky_relu_``; ``slope == 1`` is the bias add alone. Returns ``raw``."""
    B, C, H, W, slope = _conv_epi_args(raw, bias, slope)
    if raw.numel() == 0:
        return raw
    dev = raw.device
    lib = _lib.load()
    _args = (raw.data_ptr(), bias.contiguous().data_ptr(), B, C, H, W, slope, _lib.stream_handle(dev),)
    # algorithmic bytes: raw read and written, bias read
    with torch.cuda.device(dev), _kt.timed("conv_epi_fwd", (B, C, H, W, slope != 1.0), dev,
                                           8 * B * C * H * W + 4 * C):
        rc = lib.usf_convepi_fwd_f32(*_args)
    _lib.check(rc, "usf_convepi_fwd_f32")
    return raw


def conv_epilogue_backward(grad_out: torch.Tensor, y: torch.Tensor | None, slope: float,
                           need_bias: bool = True) -> tuple[torch.Tensor, torch.Tensor | None]:
    """The backward of :func:`conv_epilogue_forward` -> ``(grad_in, grad_bias)``.

    With an activation (``slope != 1``; ``y`` is the forward's result)
    ``grad_in = leaky_relu_backward(grad_out, y, slope)`` (bit-identical), dense;
    without one ``y`` is None and ``grad_in`` is ``grad_out`` itself.
    ``grad_bias[c]`` is the sum of ``grad_in`` over (b, h, w), from the same pass
    and deterministic; ``need_bias=False`` returns None and requests no workspace.
    ``grad_out`` may be a channel slice of an NCHW-contiguous tensor (a concat's
    gradient): it is read in place, no dense copy."""
    _require_device_f32("grad_out", grad_out)
    B, C, H, W = _nchw("grad_out", grad_out)
    slope = float(slope)
    if not slope > 0.0:
        raise ValueError(f"slope={slope} must be > 0 (1 = no activation)")
    act = slope != 1.0
    dev = grad_out.device
    if act:
        if y is None:
            raise ValueError("y (the forward's result) is needed with an activation")
        _require_device_f32("y", y)
        if tuple(y.shape) != (B, C, H, W) or y.device != dev or not y.is_contiguous():
            raise ValueError(f"y must be a dense {(B, C, H, W)} tensor on {dev}")
        y = _dense16(y)
    elif y is not None:
        raise ValueError("y must be None without an activation (slope == 1)")
    if not act and not need_bias:
        return grad_out, None
    if grad_out.numel() == 0:
        return (torch.empty_like(y) if act else grad_out), (grad_out.new_zeros(C) if need_bias else None)
    try:
        gbs = _plane_slice_stride("grad_out", grad_out, (B, C, H, W))
        g = grad_out
    except ValueError:  # any other layout: one dense copy, as the convolution would make
        g = grad_out.contiguous()
        gbs = C * H * W
    lib = _lib.load()
    gin = torch.empty((B, C, H, W), device=dev, dtype=torch.float32) if act else None
    gbias = ws = None
    nws = 0
    if need_bias:
        nws = int(lib.usf_convepi_bwd_workspace(B, C, H, W))
        if nws < 0:
            raise ValueError(f"conv_epilogue_backward: shape {(B, C, H, W)} is too large for the bias-gradient split")
        gbias = torch.empty(C, device=dev, dtype=torch.float32)
        if nws:
            ws = torch.empty(nws, device=dev, dtype=torch.float32)
    _args = (g.data_ptr(), gbs, _ptr(y), _ptr(gin), _ptr(gbias), _ptr(ws), nws, B, C, H, W, slope,
             _lib.stream_handle(dev),)
    # algorithmic bytes: grad_out (and y) read, grad_in written with an activation; grad_bias written
    with torch.cuda.device(dev), _kt.timed("conv_epi_bwd", (B, C, H, W, act), dev,
                                           (12 if act else 4) * B * C * H * W + 4 * C):
        rc = lib.usf_convepi_bwd_f32(*_args)
    _lib.check(rc, "usf_convepi_bwd_f32")
    return (gin if act else grad_out), gbias
