"""The buffer contract of the C ABI (include/unsamflow_hip*.h), entry point by
entry point: a kernel writes nothing outside its outputs, writes every output
element, changes no input, needs no initial state in its scratch beyond what
the header asks for, and computes the same numbers wherever its buffers lie.

Every case calls a C entry point directly (``_lib.load()``), so every pointer,
caller scratch and workspaces included, is the test's own. It runs twice on the
same ``oracle.hashrng`` inputs:

* the plain run: every buffer its own torch allocation, outputs and scratch zero;
* the guarded run: every buffer in one ``guard_util.Arena``, a single
  allocation filled with a NaN pattern, each buffer on a 16-byte boundary with
  its guard starting at the very next word. Inputs hold their data, outputs
  and "need not be initialised" scratch hold the pattern, "ZERO when first
  passed" workspaces hold zeros.

and asserts: both calls return 0 and raise no device error flag; every guard
word is intact; every input is unchanged bit for bit; no output element still
holds the pattern; the guarded outputs equal the plain ones -- bit for bit,
except the documented atomic-order outputs (warp grad_x, the splat map, the
0/1 occlusion masks next to the threshold), which take the tolerance of their
existing parity tests; the plain outputs equal the ``ops`` wrapper's on the
same inputs (the parity tests pin the wrappers to the oracle), or the oracle
where an entry has no wrapper. The persistent forms run twice in the arena:
the second call equals the first, and the occlusion maps read zero after each.

The parameters the headers declare 4-byte aligned (slices: the flows, the
correlation's concat slices, the conv epilogue's gradient, the AR loss's
views, the small coefficient tables) get one guarded case each with the
buffer shifted one word off the 16-byte boundary. No 16-byte parameter is ever
passed misaligned; ``test_ops_realign_*`` checks that ``ops`` never forwards one.

Out of scope: a benign over-READ whose lanes are discarded leaves no trace in
memory and cannot be seen by this method.
"""
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import torch

import ar_util
import fakeobj_util
from guard_util import Arena, Plain
from oracle import hashrng
from persist_util import np_fields
from unsamflow_amd import _lib, ops

pytestmark = pytest.mark.gpu

F32, I32, I64, F64, U8 = torch.float32, torch.int32, torch.int64, torch.float64, torch.uint8
BORDER, ZEROS = _lib.PAD_BORDER, _lib.PAD_ZEROS


class Run:
    """The buffers of one call, placed by a Plain or an Arena allocator."""

    def __init__(self, alloc, mis=()):
        self.alloc = alloc
        self.mis = set(mis) if alloc.guarded else set()  # buffers shifted one word off the 16-byte boundary
        self.inputs, self.outputs = [], {}

    def _place(self, name, shape, dtype, fill, keep=None):
        return self.alloc.place(shape, dtype, fill, name=name, misalign=1 if name in self.mis else 0, keep=keep)

    def inp(self, name, data, parent=None, keep=None):
        """An input holding ``data`` (ndarray or CPU tensor); with ``parent`` /
        ``keep`` a slice of a larger placed buffer."""
        t = torch.from_numpy(np.ascontiguousarray(data)) if isinstance(data, np.ndarray) else data.contiguous()
        v = self._place(name, parent or t.shape, t.dtype, t, keep)
        self.inputs.append((name, v, v.clone()))
        return v

    def out(self, name, shape, dtype=F32, parent=None, keep=None):
        v = self._place(name, parent or shape, dtype, None, keep)
        self.outputs[name] = v
        return v

    def inout(self, name, data):
        """A documented in-place buffer: holds data, compared as an output."""
        t = torch.from_numpy(np.ascontiguousarray(data)) if isinstance(data, np.ndarray) else data.contiguous()
        v = self._place(name, t.shape, t.dtype, t)
        self.outputs[name] = v
        return v

    def scratch(self, name, n, dtype=F32, zero=False):
        """Caller scratch of n elements (None for n <= 0): poison, or zeros for
        the workspaces the header wants ZERO when first passed."""
        if n <= 0:
            return None
        return self._place(name, (int(n),), dtype, "zero" if zero else None)


def ptr(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    t = t.contiguous()
    return t.view(I32) if t.element_size() == 4 else t.view(torch.int64) if t.element_size() == 8 else t


def exact(name, a, b):
    assert torch.equal(_bits(a), _bits(b)), f"{name}: {int((_bits(a) != _bits(b)).sum())} elements differ"


def close(atol, rtol):
    def cmp(name, a, b):
        torch.testing.assert_close(a, b, atol=atol, rtol=rtol, msg=lambda m: f"{name}: {m}")
    return cmp


def occ_equal(cmap, th=0.2, eps=1e-5):
    """0/1 masks equal except where the reference splat map lies within eps of the
    threshold (the allowance of test_occ_vis_pair_vs_oracle_full_size)."""
    def cmp(name, a, b):
        bad = (a != b).cpu().numpy().reshape(cmap.shape)
        assert not np.any(bad & (np.abs(np.clip(cmap, 0, 1) - th) > eps)), f"{name}: {int(bad.sum())} differ"
    return cmp


# tolerances of the existing parity tests (tests/test_gpu_parity.py, tests/test_gpu_persist.py)
CORR_VS_ORACLE = close(1e-5, 1e-5)
WARP_GX_VS_ORACLE = close(1e-4, 1e-5)  # fp32 atomics; also the scatter form's run-to-run bound
WARP_GX_OVERFLOW = close(1e-5, 1e-5)  # binned gather, cells beyond 4 pixels (test_gpu_persist.py)
SPLAT = close(2e-6, 1e-6)

Result = namedtuple("Result", "rc cmp ref ref_cmp post", defaults=({}, None, {}, None))


def _dev(a, dev):
    return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(dev)


def _flow(shape, seed, scale=2.0):
    return hashrng.symmetric(shape, seed, scale)


def _splat_ref(flow):
    """The reference splat map of a [B,2,H,W] displacement field (CPU, numpy [B,1,H,W])."""
    from oracle.torch_ref import oracle_corresponding_map

    B, _, H, W = flow.shape
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    grid = torch.stack([xs, ys], 0).float().expand(B, 2, H, W)
    return oracle_corresponding_map(grid + torch.from_numpy(np.ascontiguousarray(flow))).numpy().reshape(B, 1, H, W)


# ------------------------------------------------------------ correlation --
def corr_fwd(r, lib, st, shape, d):
    from oracle.corr import corr_forward_np

    B, C, H, W = shape
    K2 = (2 * d + 1) ** 2
    a1, a2 = hashrng.normal(shape, 11), hashrng.normal(shape, 12)
    x1, x2 = r.inp("x1", a1), r.inp("x2", a2)
    out = r.out("out", (B, K2, H, W))
    rc = lib.usf_corr_fwd_f32(ptr(x1), ptr(x2), ptr(out), B, C, H, W, d, st)
    return Result(rc, ref=lambda: {"out": corr_forward_np(a1, a2, d)}, ref_cmp={"out": CORR_VS_ORACLE})


def corr_fwd_ex(r, lib, st, shape, d, split=False):
    """LeakyReLU epilogue into a concat slice, the sign mask, the split workspace where the shape has one."""
    B, C, H, W = shape
    if split:  # the smallest channel count at which this level splits (host query)
        C = next(c for c in range(8, 2049, 8) if lib.usf_corr_fwd_workspace(B, c, H, W, d) > 0)
        shape = (B, C, H, W)
    nws = int(lib.usf_corr_fwd_workspace(B, C, H, W, d))
    assert (nws > 0) == split, (shape, d, nws)
    K2 = (2 * d + 1) ** 2
    CT, c0 = K2 + 3, 2  # the concat buffer and the slice's first channel
    x1, x2 = r.inp("x1", hashrng.normal(shape, 13)), r.inp("x2", hashrng.normal(shape, 14))
    out = r.out("out", (B, K2, H, W), parent=(B, CT, H, W), keep=(slice(None), slice(c0, c0 + K2)))
    nm = int(lib.usf_corr_act_mask_words(B, H, W, d))
    mask = r.out("act_mask", (nm,), I64)
    ws = r.scratch("workspace", nws)
    rc = lib.usf_corr_fwd_ex_f32(ptr(x1), ptr(x2), ptr(out), CT * H * W, 1, 0.1, ptr(mask), ptr(ws), nws, B, C, H, W, d,
                                 st)

    def ref():
        cat = torch.zeros((B, CT, H, W), device=x1.device)
        m = ops.corr_act_mask(B, H, W, d, x1.device)
        ops.corr_forward_ex(x1, x2, d, cat[:, c0:c0 + K2], leaky_slope=0.1, act_mask=m)
        return {"out": cat[:, c0:c0 + K2], "act_mask": m.view(-1)}
    return Result(rc, ref=ref)


def corr_bwd(r, lib, st, shape, d):
    B, C, H, W = shape
    K2 = (2 * d + 1) ** 2
    x1, x2 = r.inp("x1", hashrng.normal(shape, 15)), r.inp("x2", hashrng.normal(shape, 16))
    g = r.inp("gout", hashrng.normal((B, K2, H, W), 17))
    gx1, gx2 = r.out("gx1", shape), r.out("gx2", shape)
    rc = lib.usf_corr_bwd_f32(ptr(x1), ptr(x2), ptr(g), ptr(gx1), ptr(gx2), B, C, H, W, d, st)
    return Result(rc, ref=lambda: dict(zip(("gx1", "gx2"), ops.corr_backward(x1, x2, g, d))))


def corr_bwd_ex(r, lib, st, shape, d, mode):
    """The gradient read from a slice of the concat gradient; mode "act_out": the
    derivative pass into scratch, "mask": the sign-mask form. The concat holds
    K2 + 3 channels, so its batch stride is a multiple of 4 at both shapes."""
    B, C, H, W = shape
    K2 = (2 * d + 1) ** 2
    CT, c0 = K2 + 3, 1
    assert (CT * H * W) % 4 == 0
    keep = (slice(None), slice(c0, c0 + K2))
    x1, x2 = r.inp("x1", hashrng.normal(shape, 18)), r.inp("x2", hashrng.normal(shape, 19))
    g = r.inp("gout", hashrng.normal((B, K2, H, W), 20), parent=(B, CT, H, W), keep=keep)
    act = mask = scratch = None
    if mode == "act_out":
        act = r.inp("act_out", hashrng.normal((B, K2, H, W), 21), parent=(B, CT, H, W), keep=keep)
        scratch = r.scratch("scratch", int(lib.usf_corr_bwd_ex_scratch(B, C, H, W, d)))
    else:
        nm = int(lib.usf_corr_act_mask_words(B, H, W, d))
        bits = (hashrng.uniform((nm,), 22).astype(np.float64) * 2.0 ** 62).astype(np.int64)
        mask = r.inp("act_mask", bits)
    gx1, gx2 = r.out("gx1", shape), r.out("gx2", shape)
    rc = lib.usf_corr_bwd_ex_f32(ptr(x1), ptr(x2), ptr(g), CT * H * W, ptr(act), ptr(mask), 0.1, ptr(scratch), ptr(gx1),
                                 ptr(gx2), B, C, H, W, d, st)
    return Result(rc, ref=lambda: dict(zip(("gx1", "gx2"), ops.corr_backward_ex(
        x1, x2, g, d, act_out=act, leaky_slope=0.1, act_mask=mask))))


# ------------------------------------------------------------------- warp --
def warp_fwd(r, lib, st, shape, pad):
    B, C, H, W = shape
    x = r.inp("x", hashrng.normal(shape, 30))
    flow = r.inp("flow", _flow((B, 2, H, W), 31))
    out = r.out("out", shape)
    rc = lib.usf_warp_fwd_f32(ptr(x), ptr(flow), 2 * H * W, ptr(out), B, C, H, W, pad, st)
    return Result(rc, ref=lambda: {"out": ops.warp_forward(x, flow, "border" if pad == BORDER else "zeros")})


def warp_fwd_up(r, lib, st, shape, pad):
    B, C, H, W = shape
    x = r.inp("x", hashrng.normal(shape, 32))
    coarse = r.inp("coarse_flow", _flow((B, 2, H // 2, W // 2), 33, 1.0))
    up, out = r.out("up_flow", (B, 2, H, W)), r.out("out", shape)
    rc = lib.usf_warp_fwd_up_f32(ptr(x), ptr(coarse), ptr(up), ptr(out), B, C, H, W, pad, st)
    return Result(rc, ref=lambda: dict(zip(("up_flow", "out"), ops.warp_forward_up(
        x, coarse, "border" if pad == BORDER else "zeros"))))


def warp_bwd(r, lib, st, shape, pad, form, field="gentle"):
    """form: "scatter" (usf_warp_bwd_f32), "ex" (per-call workspace, poison),
    "persist" (zeroed workspace, two calls). field "gentle": a smooth +-0.5 px
    flow whose slope stays below 0.1, so no cell receives more than 2 x 2 source
    pixels and the binned gather is bit-identical; "pile": every pixel of a strip
    sent to one border column, so cells overflow (the overflow buffer / list)."""
    from oracle.warp import warp_backward_np

    B, C, H, W = shape
    ax, ag = hashrng.uniform(shape, 34), hashrng.normal(shape, 35)
    af = np_fields(B, H, W)["pile"] if field == "pile" else 0.25 * np_fields(B, H, W)["smooth"]
    x, flow, g = r.inp("x", ax), r.inp("flow", af), r.inp("gout", ag)
    gx, gf = r.out("gx", shape), r.out("gflow", (B, 2, H, W))
    pname = "border" if pad == BORDER else "zeros"
    oracle = lambda: dict(zip(("gx", "gflow"), warp_backward_np(ax, af, ag, pname)))  # noqa: E731
    vs_oracle = {"gx": WARP_GX_VS_ORACLE, "gflow": WARP_GX_VS_ORACLE}
    if form == "scatter":
        rc = lib.usf_warp_bwd_f32(ptr(x), ptr(flow), 2 * H * W, ptr(g), ptr(gx), ptr(gf), B, C, H, W, pad, st)
        return Result(rc, cmp={"gx": WARP_GX_VS_ORACLE}, ref=oracle, ref_cmp=vs_oracle)
    # cells beyond 4 pixels are summed by fp32 atomics: only then grad_x is not bit-identical
    gx_cmp = {k: WARP_GX_OVERFLOW for k in ("gx", "gx#2")} if field == "pile" else {}
    if form == "ex":
        n = int(lib.usf_warp_bwd_workspace(B, H, W))
        ws = r.scratch("workspace", n, U8)
        rc = lib.usf_warp_bwd_ex_f32(ptr(x), ptr(flow), 2 * H * W, ptr(g), ptr(gx), ptr(gf), ptr(ws), n, B, C, H, W, pad,
                                     st)
        return Result(rc, cmp=gx_cmp, ref=oracle, ref_cmp=vs_oracle)
    n = int(lib.usf_warp_bwd_persist_workspace(B, C, H, W))
    ws = r.scratch("workspace", n, U8, zero=True)
    gx2, gf2 = r.out("gx#2", shape), r.out("gflow#2", (B, 2, H, W))
    rc = [lib.usf_warp_bwd_persist_f32(ptr(x), ptr(flow), 2 * H * W, ptr(g), ptr(a), ptr(b), ptr(ws), n, B, C, H, W, pad,
                                       st) for a, b in ((gx, gf), (gx2, gf2))]

    def post():  # the second call on the same workspace repeats the first
        gx_cmp.get("gx", exact)("gx#2 vs gx", gx2, gx)
        exact("gflow#2 vs gflow", gf2, gf)

    def ref():
        ops.clear_persistent_workspaces()
        a, b = ops.warp_backward(x, flow, g, pname)
        return {"gx": a, "gflow": b, "gx#2": a, "gflow#2": b}
    return Result(rc, cmp=gx_cmp, ref=ref, ref_cmp=gx_cmp, post=post)


# -------------------------------------------------------------- occlusion --
def splat_map(r, lib, st, bhw, absolute):
    B, H, W = bhw
    af = _flow((B, 2, H, W), 40)
    if absolute:
        ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
        af = (af + np.stack([xs, ys])[None]).astype(np.float32)
    flow = r.inp("flow", af)
    m = r.out("map", (B, 1, H, W))
    rc = lib.usf_splat_map_f32(ptr(flow), 2 * H * W, ptr(m), B, H, W, int(absolute), st)
    return Result(rc, cmp={"map": SPLAT}, ref=lambda: {"map": ops.splat_map(flow, absolute)}, ref_cmp={"map": SPLAT})


def occ_backward(r, lib, st, bhw, persist):
    from oracle.torch_ref import oracle_occu_mask_backward

    B, H, W = bhw
    af = _flow((B, 2, H, W), 41)
    near = occ_equal(_splat_ref(af))
    flow = r.inp("flow21", af)
    occ = r.out("occ", (B, 1, H, W))
    if not persist:
        rc = lib.usf_occ_backward_f32(ptr(flow), 2 * H * W, ptr(occ), B, H, W, 0.2, st)
        return Result(rc, cmp={"occ": near}, ref=lambda: {"occ": oracle_occu_mask_backward(torch.from_numpy(af), 0.2)},
                      ref_cmp={"occ": near})
    occ2 = r.out("occ#2", (B, 1, H, W))
    m = r.scratch("map", B * H * W, zero=True)
    rc, zero = [], []
    for o in (occ, occ2):
        rc.append(lib.usf_occ_backward_persist_f32(ptr(flow), 2 * H * W, ptr(o), ptr(m), 4 * B * H * W, B, H, W, 0.2, st))
        zero.append(int(torch.count_nonzero(m)))  # the header: the threshold pass zeroes the map again

    def post():
        assert zero == [0, 0], f"map not re-zeroed: {zero} nonzero words after call 1 / 2"
        near("occ#2 vs occ", occ2, occ)

    def ref():
        o = ops.occ_backward(flow, 0.2)
        return {"occ": o, "occ#2": o}
    return Result(rc, cmp={"occ": near, "occ#2": near}, ref=ref, ref_cmp={"occ": near, "occ#2": near}, post=post)


def occ_vis_pair(r, lib, st, bhw):
    B, H, W = bhw
    af = _flow((B, 4, H, W), 42)
    # vis[0] comes from flow4[:, 2:], vis[1] from flow4[:, :2]
    near = occ_equal(np.stack([_splat_ref(af[:, 2:]), _splat_ref(af[:, :2])]))
    flow = r.inp("flow4", af)
    vis, vis2 = r.out("vis", (2, B, 1, H, W)), r.out("vis#2", (2, B, 1, H, W))
    m = r.scratch("map", 2 * B * H * W, zero=True)
    rc, zero = [], []
    for v in (vis, vis2):
        rc.append(lib.usf_occ_vis_pair_persist_f32(ptr(flow), 4 * H * W, ptr(v), ptr(m), 8 * B * H * W, B, H, W, 0.2, st))
        zero.append(int(torch.count_nonzero(m)))

    def post():
        assert zero == [0, 0], f"map not re-zeroed: {zero} nonzero words after call 1 / 2"
        near("vis#2 vs vis", vis2, vis)

    def ref():
        v = ops.occ_vis_pair(flow, 0.2)
        return {"vis": v, "vis#2": v}
    return Result(rc, cmp={"vis": near, "vis#2": near}, ref=ref, ref_cmp={"vis": near, "vis#2": near}, post=post)


def occ_bidirection(r, lib, st, bhw):
    B, H, W = bhw
    f12, f21 = r.inp("flow12", _flow((B, 2, H, W), 43)), r.inp("flow21", _flow((B, 2, H, W), 44))
    occ = r.out("occ", (B, 1, H, W))
    rc = lib.usf_occ_bidirection_f32(ptr(f12), 2 * H * W, ptr(f21), 2 * H * W, ptr(occ), B, H, W, 0.01, 0.5, st)
    return Result(rc, ref=lambda: {"occ": ops.occ_bidirection(f12, f21)})


# ------------------------------------------- photometric and census losses --
LOSS = {"photo": (3, 4, (0.15, 0.85)), "census": (2, 2, (1.0,))}  # floats of out and basis planes per direction, weights


def _loss_inputs(r, B, C, H, W, seed, tag=""):
    im1, im2 = r.inp("im1" + tag, hashrng.uniform((B, C, H, W), seed)), r.inp("im2" + tag, hashrng.uniform((B, C, H, W), seed + 1))
    m1, m2 = r.inp("mask1" + tag, hashrng.uniform((B, 1, H, W), seed + 2)), r.inp("mask2" + tag, hashrng.uniform((B, 1, H, W), seed + 3))
    return im1, im2, m1, m2, r.inp("flow" + tag, _flow((B, 4, H, W), seed + 4, 1.5))


def loss_fwd(r, lib, st, kind, shape):
    B, C, H, W = shape
    nout, planes, w = LOSS[kind]
    src, tgt = r.inp("src", hashrng.uniform(shape, 50)), r.inp("tgt", hashrng.uniform(shape, 51))
    mask, flow = r.inp("mask", hashrng.uniform((B, 1, H, W), 52)), r.inp("flow", _flow((B, 2, H, W), 53, 1.5))
    part = r.scratch("partials", getattr(lib, f"usf_{kind}_loss_partials")(B, H, W))
    out, basis = r.out("out", (nout,)), r.out("grad_basis", (B, planes, H, W))
    rc = getattr(lib, f"usf_{kind}_loss_fwd_f32")(ptr(src), ptr(tgt), ptr(mask), ptr(flow), 2 * H * W, ptr(part), ptr(out),
                                                  ptr(basis), B, C, H, W, BORDER, *w, st)
    return Result(rc, ref=lambda: dict(zip(("out", "grad_basis"), getattr(ops, f"{kind}_loss_forward")(
        src, tgt, mask, flow, "border", *w, need_grad=True))))


def loss_pair_fwd(r, lib, st, kind, shape):
    B, C, H, W = shape
    nout, planes, w = LOSS[kind]
    im1, im2, m1, m2, flow = _loss_inputs(r, B, C, H, W, 54)
    part = r.scratch("partials", 2 * getattr(lib, f"usf_{kind}_loss_partials")(B, H, W))
    out, basis = r.out("out", (2 * nout,)), r.out("grad_basis", (B, 2 * planes, H, W))
    rc = getattr(lib, f"usf_{kind}_loss_pair_fwd_f32")(ptr(im1), ptr(im2), ptr(m1), ptr(m2), ptr(flow), 4 * H * W,
                                                       ptr(part), ptr(out), ptr(basis), B, C, H, W, BORDER, *w, st)
    return Result(rc, ref=lambda: dict(zip(("out", "grad_basis"), getattr(ops, f"{kind}_loss_pair_forward")(
        flow, im1, im2, m1, m2, "border", *w, need_grad=True))))


def loss_bwd(r, lib, st, kind, bhw, ndir):
    B, H, W = bhw
    nout, planes, _ = LOSS[kind]
    basis = r.inp("grad_basis", hashrng.normal((B, ndir * planes, H, W), 59))
    coef, gl = r.inp("coef", hashrng.uniform((ndir * nout,), 60)), r.inp("grad_loss", hashrng.normal((ndir,), 61))
    gflow = r.out("grad_flow", (B, 2 * ndir, H, W))
    rc = getattr(lib, f"usf_{kind}_loss_bwd_f32")(ptr(basis), ptr(coef), ptr(gl), ptr(gflow), B, H, W, ndir, st)
    return Result(rc, ref=lambda: {"grad_flow": getattr(ops, f"{kind}_loss_backward")(basis, coef, gl)})


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _ints(vs, ctype=ctypes.c_int):
    return (ctype * len(vs))(*vs)


def loss_pyr_fwd(r, lib, st, kind, B, C, sizes):
    nout, planes, w = LOSS[kind]
    n = len(sizes)
    sc = [_loss_inputs(r, B, C, H, W, 62 + 10 * k, f"[{k}]") for k, (H, W) in enumerate(sizes)]
    Hs, Ws = _ints([s[0] for s in sizes]), _ints([s[1] for s in sizes])
    npart = int(getattr(lib, f"usf_{kind}_loss_pyramid_partials")(n, Hs, Ws, B))
    part = r.scratch("partials", npart)
    out = r.out("out", (n, 2 * nout))
    bases = [r.out(f"grad_basis[{k}]", (B, 2 * planes, H, W)) for k, (H, W) in enumerate(sizes)]
    rc = getattr(lib, f"usf_{kind}_loss_pyramid_fwd_f32")(
        n, *[_ptrs([s[i] for s in sc]) for i in range(5)], _ints([4 * H * W for H, W in sizes], ctypes.c_longlong), Hs, Ws,
        ptr(part), npart, ptr(out), _ptrs(bases), B, C, BORDER, *w, st)

    def ref():
        o, bs = getattr(ops, f"{kind}_loss_pyramid_forward")([s[4] for s in sc], *[[s[i] for s in sc] for i in range(4)],
                                                             "border", *w, need_grad=True)
        return {"out": o, **{f"grad_basis[{k}]": b for k, b in enumerate(bs)}}
    return Result(rc, ref=ref)


def loss_pyr_bwd(r, lib, st, kind, B, sizes):
    nout, planes, _ = LOSS[kind]
    n = len(sizes)
    bases = [r.inp(f"grad_basis[{k}]", hashrng.normal((B, 2 * planes, H, W), 90 + k)) for k, (H, W) in enumerate(sizes)]
    coef, gl = r.inp("coef", hashrng.uniform((n, 2 * nout), 95)), r.inp("grad_loss", hashrng.normal((n, 2), 96))
    gflows = [r.out(f"grad_flow[{k}]", (B, 4, H, W)) for k, (H, W) in enumerate(sizes)]
    rc = getattr(lib, f"usf_{kind}_loss_pyramid_bwd_f32")(n, _ptrs(bases), ptr(coef), ptr(gl), _ptrs(gflows),
                                                          _ints([s[0] for s in sizes]), _ints([s[1] for s in sizes]), B,
                                                          st)
    return Result(rc, ref=lambda: {f"grad_flow[{k}]": t for k, t in enumerate(
        getattr(ops, f"{kind}_loss_pyramid_backward")(bases, coef, gl))})


# ------------------------------------------------- upsampling and pyramid --
def flow_upsample(r, lib, st, shape, f, form):
    B, C, H, W = shape
    big = (B, C, H * f, W * f)
    if form == "fwd":
        flow, out = r.inp("flow", hashrng.normal(shape, 100)), r.out("out", big)
        rc = lib.usf_flow_upsample_f32(ptr(flow), ptr(out), B, C, H, W, f, st)
        return Result(rc, ref=lambda: {"out": ops.flow_upsample(flow, f)})
    ga, gf = r.inp("grad_a", hashrng.normal(big, 101)), r.out("grad_flow", shape)
    if form == "bwd":
        rc = lib.usf_flow_upsample_bwd_f32(ptr(ga), ptr(gf), B, C, H, W, f, st)
        return Result(rc, ref=lambda: {"grad_flow": ops.flow_upsample_backward(ga, f)})
    gb = r.inp("grad_b", hashrng.normal(big, 102))
    rc = lib.usf_flow_upsample_bwd_sum_f32(ptr(ga), ptr(gb), ptr(gf), B, C, H, W, f, st)
    return Result(rc, ref=lambda: {"grad_flow": ops.flow_upsample_backward(ga, f, gb)})


def convex(r, lib, st, bhw, f, bwd):
    B, H, W = bhw
    flow, mask = r.inp("flow", hashrng.normal((B, 2, H, W), 110)), r.inp("mask", hashrng.normal((B, 9 * f * f, H, W), 111))
    if not bwd:
        out = r.out("out", (B, 2, f * H, f * W))
        rc = lib.usf_convex_upsample_f32(ptr(flow), ptr(mask), ptr(out), B, H, W, f, 0.25, st)
        return Result(rc, ref=lambda: {"out": ops.convex_upsample(flow, mask, f, 0.25)})
    go = r.inp("grad_out", hashrng.normal((B, 2, f * H, f * W), 112))
    gf, gm = r.out("grad_flow", (B, 2, H, W)), r.out("grad_mask", (B, 9 * f * f, H, W))
    scratch = r.scratch("scratch", int(lib.usf_convex_upsample_bwd_scratch(B, H, W)))
    rc = lib.usf_convex_upsample_bwd_f32(ptr(flow), ptr(mask), ptr(go), ptr(gf), ptr(gm), ptr(scratch), B, H, W, f, 0.25, st)
    return Result(rc, ref=lambda: dict(zip(("grad_flow", "grad_mask"), ops.convex_upsample_backward(flow, mask, go, f, 0.25))))


def convex_pyr(r, lib, st, B, sizes, bwd):
    n, f = len(sizes), 4
    flows = [r.inp(f"flow[{k}]", hashrng.normal((B, 2, H, W), 120 + k)) for k, (H, W) in enumerate(sizes)]
    masks = [r.inp(f"mask[{k}]", hashrng.normal((B, 144, H, W), 125 + k)) for k, (H, W) in enumerate(sizes)]
    Hs, Ws = _ints([s[0] for s in sizes]), _ints([s[1] for s in sizes])
    if not bwd:
        outs = [r.out(f"out[{k}]", (B, 2, f * H, f * W)) for k, (H, W) in enumerate(sizes)]
        rc = lib.usf_convex_upsample_pyramid_f32(n, _ptrs(flows), _ptrs(masks), _ptrs(outs), Hs, Ws, B, f, 0.25, st)
        return Result(rc, ref=lambda: {f"out[{k}]": t for k, t in enumerate(ops.convex_upsample_pyramid(flows, masks, f, 0.25))})
    gos = [r.inp(f"grad_out[{k}]", hashrng.normal((B, 2, f * H, f * W), 130 + k)) for k, (H, W) in enumerate(sizes)]
    gfs = [r.out(f"grad_flow[{k}]", (B, 2, H, W)) for k, (H, W) in enumerate(sizes)]
    gms = [r.out(f"grad_mask[{k}]", (B, 144, H, W)) for k, (H, W) in enumerate(sizes)]
    ns = int(lib.usf_convex_upsample_pyramid_bwd_scratch(n, Hs, Ws, B))
    scratch = r.scratch("scratch", ns)
    rc = lib.usf_convex_upsample_pyramid_bwd_f32(n, _ptrs(flows), _ptrs(masks), _ptrs(gos), _ptrs(gfs), _ptrs(gms),
                                                 ptr(scratch), ns, Hs, Ws, B, f, 0.25, st)

    def ref():
        a, b = ops.convex_upsample_pyramid_backward(flows, masks, gos, f, 0.25)
        return {**{f"grad_flow[{k}]": t for k, t in enumerate(a)}, **{f"grad_mask[{k}]": t for k, t in enumerate(b)}}
    return Result(rc, ref=ref)


def area_pyramid(r, lib, st, shape):
    B, C, H, W = shape
    x = r.inp("x", hashrng.uniform(shape, 140))
    outs = [r.out(f"out{s}", (B, C, H >> s, W >> s)) for s in (1, 2, 3)]
    rc = lib.usf_area_pyramid_f32(ptr(x), *[ptr(o) for o in outs], B, C, H, W, st)
    return Result(rc, ref=lambda: {f"out{s}": t for s, t in zip((1, 2, 3), ops.area_pyramid(x))})


def stream_copy(r, lib, st, n):
    a = hashrng.normal((n,), 141)
    src, dst = r.inp("src", a), r.out("dst", (n,))
    return Result(lib.usf_stream_copy_f32(ptr(src), ptr(dst), n, st), ref=lambda: {"dst": a})


# ----------------------------------------------------------- augmentation --
def ar_transform(r, lib, st, bhw, noise):
    B, H, W = bhw
    a1, a2, af, am = ar_util.inputs(B, H, W, 150)
    img1, img2, flow, mask = r.inp("img1", a1), r.inp("img2", a2), r.inp("flow", af), r.inp("mask", am)
    theta = r.inp("theta", ar_util.explicit_thetas(B))
    n1 = r.inp("noise1", hashrng.symmetric((B, 3, H, W), 151, 0.05)) if noise else None
    n2 = r.inp("noise2", hashrng.symmetric((B, 3, H, W), 152, 0.05)) if noise else None
    names = ("img1_t", "img2_t", "flow_t", "mask_t")
    outs = [r.out(nm, s) for nm, s in zip(names, ((B, 3, H, W), (B, 3, H, W), (B, 2, H, W), (B, 1, H, W)))]
    rc = lib.usf_ar_transform_f32(ptr(img1), ptr(img2), ptr(flow), 2 * H * W, ptr(mask), ptr(theta), ptr(n1), ptr(n2),
                                  *[ptr(o) for o in outs], B, H, W, st)
    return Result(rc, ref=lambda: dict(zip(names, ops.ar_transform(img1, img2, flow, mask, theta, n1, n2))))


def ar_loss(r, lib, st, bhw, bwd):
    """target and noc are crop views of larger tensors (batch, channel and row strides)."""
    B, H, W = bhw
    PH, PW = H + 2, W + 3
    crop = (slice(None), slice(None), slice(1, 1 + H), slice(2, 2 + W))
    pred = r.inp("pred", _flow((B, 2, H, W), 160))
    target = r.inp("target", _flow((B, 2, H, W), 161), parent=(B, 2, PH, PW), keep=crop)
    noc = r.inp("noc", (hashrng.uniform((B, 1, H, W), 162) > 0.3).astype(np.float32), parent=(B, 1, PH, PW), keep=crop)
    ts, ns = (2 * PH * PW, PH * PW, PW), (PH * PW, PW)
    eps, q = 0.01, 0.4
    if not bwd:
        part = r.scratch("partials", lib.usf_ar_loss_partials(B, H, W))
        out = r.out("out", (2,))
        rc = lib.usf_ar_loss_fwd_f32(ptr(pred), ptr(target), *ts, ptr(noc), *ns, None, ptr(part), ptr(out), B, H, W, eps, q,
                                     st)
        return Result(rc, ref=lambda: {"out": ops.ar_loss_forward(pred, target, noc, eps, q)})
    coef, gl = r.inp("coef", np.array([0.7, 0.003], np.float32)), r.inp("grad_loss", np.array([1.3], np.float32))
    gp = r.out("grad_pred", (B, 2, H, W))
    rc = lib.usf_ar_loss_bwd_f32(ptr(pred), ptr(target), *ts, ptr(noc), *ns, ptr(coef), ptr(gl), ptr(gp), B, H, W, eps, q,
                                 st)
    return Result(rc, ref=lambda: {"grad_pred": ops.ar_loss_backward(pred, target, noc, coef, gl, eps, q)})


def fakeobj_paste(r, lib, st, bhw, crop):
    B, H, W = bhw
    K, size = 2, 5
    a1, a2, af, an = fakeobj_util.base(B, H, W, 170)
    om, oi, mo = fakeobj_util.objects(size, H, W, 171)
    img1, img2, flow, noc = r.inp("img1", a1), r.inp("img2", a2), r.inp("flow", af), r.inp("noc", an)
    cm, ci, cmo = r.inp("cache_mask", om), r.inp("cache_img", oi), r.inp("cache_motion", mo)
    slot = r.inp("slot", torch.tensor([(3 * j + 1) % size for j in range(K * B)], dtype=I32))
    param = r.inp("param", fakeobj_util.plain_params(K * B, flips=[1]))
    y0, x0, ch, cw = crop
    names = ("imgs_ot", "flow_ot", "noc_ot")
    outs = [r.out(nm, (B, c, ch, cw)) for nm, c in zip(names, (6, 2, 1))]
    rc = lib.usf_fakeobj_paste_crop_f32(ptr(img1), ptr(img2), ptr(flow), 2 * H * W, ptr(noc), ptr(cm), ptr(ci), ptr(cmo),
                                        ptr(slot), ptr(param), *[ptr(o) for o in outs], B, H, W, K, size, y0, x0, ch, cw,
                                        st)
    return Result(rc, ref=lambda: dict(zip(names, ops.fakeobj_paste_crop(img1, img2, flow, noc, cm, ci, cmo, slot, param,
                                                                         (ch, cw), (y0, x0)))))


def fakeobj_push(r, lib, st, bhw):
    """The cache tensors are in-place: sample 0 goes to slot 3, sample 1 is skipped (-1)."""
    B, H, W = bhw
    size = 5
    _, a2, af, _ = fakeobj_util.base(B, H, W, 172)
    om, oi, mo = fakeobj_util.objects(size, H, W, 173)
    mask, img, flow = r.inp("obj_mask", om[:B].clone()), r.inp("img", a2), r.inp("flow", af)
    slot = r.inp("slot", torch.tensor([3] + [-1] * (B - 1), dtype=I32))
    old = (torch.from_numpy(hashrng.uniform((size, 1, H, W), 174)), torch.from_numpy(hashrng.uniform((size, 3, H, W), 175)),
           torch.from_numpy(hashrng.normal((size, 2), 176)))
    cm, ci, cmo = r.inout("cache_mask", old[0]), r.inout("cache_img", old[1]), r.inout("cache_motion", old[2])
    part = r.scratch("partials", lib.usf_fakeobj_push_partials(B, H, W))
    rc = lib.usf_fakeobj_push_f32(ptr(mask), ptr(img), ptr(flow), 2 * H * W, ptr(slot), ptr(cm), ptr(ci), ptr(cmo),
                                  ptr(part), B, H, W, size, st)

    def post():  # only the addressed slot may change
        for t, o in zip((cm, ci, cmo), old):
            keep = [s for s in range(size) if s != 3]
            exact("untouched cache slots", t[keep], o[keep].to(t.device))

    def ref():
        c = [o.to(cm.device).clone() for o in old]
        ops.fakeobj_push(mask, img, flow, slot, *c)
        return dict(zip(("cache_mask", "cache_img", "cache_motion"), c))
    return Result(rc, ref=ref, post=post)


# ------------------------------------------------------------ segment ops --
def _seg_ids(B, H, W, K, seed):
    return np.floor(hashrng.uniform((B, 1, H, W), seed) * K).clip(0, K - 1).astype(np.float32)


def segpool(r, lib, st, shape, K, bwd):
    B, C, H, W = shape
    ap, asg = hashrng.normal(shape, 180), _seg_ids(B, H, W, K, 181)
    proj, seg = r.inp("proj", ap), r.inp("seg", asg)
    nst = int(lib.usf_segpool_state_words(B, C, K))
    if not bwd:
        spread, state = r.out("spread", shape), r.out("state", (nst,), I32)
        rc = lib.usf_segpool_fwd_f32(ptr(proj), ptr(seg), ptr(spread), ptr(state), B, C, H, W, K, st)
        return Result(rc, ref=lambda: dict(zip(("spread", "state"), ops.segpool_forward(proj, seg, K))))
    state = r.inp("state", ops.segpool_forward(_dev(ap, proj.device), _dev(asg, proj.device), K)[1].cpu())
    gs, gp = r.inp("grad_spread", hashrng.normal(shape, 182)), r.out("grad_proj", shape)
    rc = lib.usf_segpool_bwd_f32(ptr(proj), ptr(seg), ptr(state), ptr(gs), ptr(gp), B, C, H, W, K, st)
    return Result(rc, ref=lambda: {"grad_proj": ops.segpool_backward(proj, seg, state, gs, K)})


def _hg_scene(bhw):
    """A small planted scene: K - 1 vertical strips following one affine flow each, a fifth of every strip occluded."""
    B, H, W = bhw
    K = 4
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    seg = np.broadcast_to(np.minimum(xs * K // W, K - 1), (B, 1, H, W)).astype(np.float32).copy()
    flow = np.stack([0.8 + 0.05 * xs - 0.02 * ys + 0.3 * seg[0, 0], -0.4 + 0.03 * xs + 0.04 * ys])[None].repeat(B, 0)
    flow = (flow + 0.01 * hashrng.symmetric((B, 2, H, W), 190)).astype(np.float32)
    occ = (hashrng.uniform((B, 1, H, W), 191) < 0.2).astype(np.float32)
    return flow, seg, occ, K


def hg(r, lib, st, bhw, entry):
    B, H, W = bhw
    af, asg, ao, K = _hg_scene(bhw)
    n_hyp, thr = 32, 0.5
    flow, seg = r.inp("flow", af), r.inp("seg", asg)
    if entry == "fit":
        occ = r.inp("occ", ao)
        rec = r.out("records", (B, _lib.HG_SLOTS, _lib.HG_RECORD_WORDS), I32)
        nws = int(lib.usf_hg_workspace_bytes(B, H, W, K, n_hyp))
        ws = r.scratch("workspace", (nws + 7) // 8, I64)
        rc = lib.usf_hg_fit_f32(ptr(flow), 2 * H * W, ptr(seg), ptr(occ), K, thr, n_hyp, 7, ptr(rec), ptr(ws), nws, B, H, W,
                                st)
        return Result(rc, ref=lambda: {"records": ops.hg_fit(flow, seg, occ, K, thr, n_hyp, 7)})
    dev = flow.device
    records = ops.hg_fit(_dev(af, dev), _dev(asg, dev), _dev(ao, dev), K, thr, n_hyp, 7).cpu()
    assert int((records[:, :, 1] == 0).sum()) > 0, "the scene must have accepted slots"
    rec = r.inp("records", records)
    if entry == "loss_fwd":
        part = r.scratch("partials", lib.usf_hg_loss_partials(B, H, W), F64)
        out = r.out("out", (1,))
        rc = lib.usf_hg_loss_fwd_f32(ptr(flow), 2 * H * W, ptr(seg), ptr(rec), ptr(part), ptr(out), B, H, W, st)
        return Result(rc, ref=lambda: {"out": ops.hg_loss_forward(flow, seg, rec).reshape(1)})
    gl, gf = r.inp("grad_loss", np.array([1.7], np.float32)), r.out("grad_flow", (B, 2, H, W))
    rc = lib.usf_hg_loss_bwd_f32(ptr(flow), 2 * H * W, ptr(seg), ptr(rec), ptr(gl), ptr(gf), B, H, W, st)
    return Result(rc, ref=lambda: {"grad_flow": ops.hg_loss_backward(flow, seg, rec, gl.reshape(()))})


# --------------------------------------------------------- conv epilogues --
def convepi_fwd(r, lib, st, shape, slope):
    B, C, H, W = shape
    ay = hashrng.normal(shape, 200)
    y, bias = r.inout("y", ay), r.inp("bias", hashrng.normal((C,), 201))
    rc = lib.usf_convepi_fwd_f32(ptr(y), ptr(bias), B, C, H, W, slope, st)
    return Result(rc, ref=lambda: {"y": ops.conv_epilogue_forward(_dev(ay, y.device), bias, slope)})


def convepi_bwd(r, lib, st, shape, slope, need_bias):
    """grad_out is a channel slice of a concat gradient of C + 3 channels."""
    B, C, H, W = shape
    CT, c0 = C + 3, 2
    act = slope != 1.0
    go = r.inp("grad_out", hashrng.normal(shape, 202), parent=(B, CT, H, W), keep=(slice(None), slice(c0, c0 + C)))
    y = r.inp("y", hashrng.normal(shape, 203)) if act else None
    gin = r.out("grad_in", shape) if act else None
    gb = r.out("grad_bias", (C,)) if need_bias else None
    nws = int(lib.usf_convepi_bwd_workspace(B, C, H, W)) if need_bias else 0
    ws = r.scratch("workspace", nws)
    rc = lib.usf_convepi_bwd_f32(ptr(go), CT * H * W, ptr(y), ptr(gin), ptr(gb), ptr(ws), nws, B, C, H, W, slope, st)

    def ref():
        a, b = ops.conv_epilogue_backward(go, y, slope, need_bias)
        return {**({"grad_in": a} if act else {}), **({"grad_bias": b} if need_bias else {})}
    return Result(rc, ref=ref)


# ------------------------------------------------------------------ table --
Case = namedtuple("Case", "id fn args safe4")
ODD, VEC = (2, 5, 5, 7), (2, 8, 6, 8)  # W % 4 != 0 and H*W % 64 != 0, odd C, B = 2 / W % 4 == 0: the vector paths
IMG_ODD, IMG_VEC = (2, 3, 5, 7), (2, 3, 6, 8)  # the losses take C <= 3 (census: C = 3, H, W >= 3)
BHW_ODD, BHW_VEC = (2, 5, 7), (2, 6, 8)
PYR_ODD, PYR_VEC = [(5, 7), (3, 5)], [(6, 8), (3, 4)]  # 2 scales / levels, the larger first
BINNED = (2, 5, 24, 40)  # H*W > 512: above the one-launch LDS form of the warp backward
HG_BHW = (2, 12, 19)

_T = []


def case(id, fn, *args, safe4=()):
    _T.append(Case(id, fn, args, tuple(safe4)))


for tag, shp in (("odd", ODD), ("vec", VEC)):
    for d in (1, 4):
        case(f"corr_fwd-{tag}-d{d}", corr_fwd, shp, d)
        case(f"corr_fwd_ex-{tag}-d{d}", corr_fwd_ex, shp, d, safe4=("out",) if tag == "odd" and d == 1 else ())
        case(f"corr_bwd-{tag}-d{d}", corr_bwd, shp, d)
        case(f"corr_bwd_ex-act_out-{tag}-d{d}", corr_bwd_ex, shp, d, "act_out",
             safe4=("gout", "act_out") if tag == "odd" and d == 1 else ())
        case(f"corr_bwd_ex-mask-{tag}-d{d}", corr_bwd_ex, shp, d, "mask")
case("corr_fwd_ex-split-d1", corr_fwd_ex, ODD, 1, True)  # the smallest C with usf_corr_fwd_workspace > 0 at 5x7
for tag, shp in (("odd", ODD), ("vec", VEC)):
    case(f"warp_fwd-{tag}-border", warp_fwd, shp, BORDER, safe4=("flow",) if tag == "odd" else ())
    case(f"warp_fwd-{tag}-zeros", warp_fwd, shp, ZEROS)
case("warp_fwd_up-6x10", warp_fwd_up, (2, 5, 6, 10), BORDER)  # even H, W; W % 4 != 0
case("warp_fwd_up-vec", warp_fwd_up, VEC, ZEROS)
for form in ("scatter", "ex", "persist"):
    case(f"warp_bwd-{form}-odd", warp_bwd, ODD, BORDER, form, safe4=("flow",))  # H*W <= 512: the small fused path
    case(f"warp_bwd-{form}-vec", warp_bwd, VEC, ZEROS, form)
    case(f"warp_bwd-{form}-binned", warp_bwd, BINNED, BORDER, form)
for form in ("ex", "persist"):
    case(f"warp_bwd-{form}-binned-pile", warp_bwd, BINNED, BORDER, form, "pile")
    case(f"warp_bwd-{form}-odd-pile", warp_bwd, ODD, BORDER, form, "pile")
for tag, bhw in (("odd", BHW_ODD), ("vec", BHW_VEC)):
    s4 = tag == "odd"
    case(f"splat_map-{tag}", splat_map, bhw, False, safe4=("flow",) if s4 else ())
    case(f"splat_map-absolute-{tag}", splat_map, bhw, True)
    case(f"occ_backward-{tag}", occ_backward, bhw, False, safe4=("flow21",) if s4 else ())
    case(f"occ_backward_persist-{tag}", occ_backward, bhw, True, safe4=("flow21",) if s4 else ())
    case(f"occ_vis_pair_persist-{tag}", occ_vis_pair, bhw, safe4=("flow4",) if s4 else ())
    case(f"occ_bidirection-{tag}", occ_bidirection, bhw, safe4=("flow12", "flow21") if s4 else ())
for kind in ("photo", "census"):
    for tag, shp, bhw, pyr in (("odd", IMG_ODD, BHW_ODD, PYR_ODD), ("vec", IMG_VEC, BHW_VEC, PYR_VEC)):
        s4 = tag == "odd"
        case(f"{kind}_fwd-{tag}", loss_fwd, kind, shp, safe4=("flow", "out") if s4 else ())
        case(f"{kind}_pair_fwd-{tag}", loss_pair_fwd, kind, shp, safe4=("flow", "out") if s4 else ())
        case(f"{kind}_bwd-{tag}-1dir", loss_bwd, kind, bhw, 1, safe4=("coef", "grad_loss") if s4 else ())
        case(f"{kind}_bwd-{tag}-2dir", loss_bwd, kind, bhw, 2)
        case(f"{kind}_pyramid_fwd-{tag}", loss_pyr_fwd, kind, 2, 3, pyr, safe4=("flow[0]", "flow[1]", "out") if s4 else ())
        case(f"{kind}_pyramid_bwd-{tag}", loss_pyr_bwd, kind, 2, pyr, safe4=("coef", "grad_loss") if s4 else ())
for tag, shp in (("odd", ODD), ("vec", VEC)):
    for form in ("fwd", "bwd", "bwd_sum"):
        case(f"flow_upsample_{form}-{tag}", flow_upsample, shp, 2, form)
for f in (2, 4, 8):
    for tag, bhw in (("odd", BHW_ODD), ("vec", BHW_VEC)):
        case(f"convex-f{f}-{tag}", convex, bhw, f, False)
        case(f"convex_bwd-f{f}-{tag}", convex, bhw, f, True)
for tag, pyr in (("odd", PYR_ODD), ("vec", PYR_VEC)):
    case(f"convex_pyramid-{tag}", convex_pyr, 2, pyr, False)
    case(f"convex_pyramid_bwd-{tag}", convex_pyr, 2, pyr, True)
case("area_pyramid-3x8x16", area_pyramid, (2, 3, 8, 16))
case("area_pyramid-5x16x8", area_pyramid, (2, 5, 16, 8))
case("stream_copy", stream_copy, 4 * 1237)
for tag, bhw in (("odd", BHW_ODD), ("vec", BHW_VEC)):
    s4 = tag == "odd"
    case(f"ar_transform-{tag}", ar_transform, bhw, False, safe4=("flow", "theta") if s4 else ())
    case(f"ar_transform-noise-{tag}", ar_transform, bhw, True)
    case(f"ar_loss_fwd-{tag}", ar_loss, bhw, False, safe4=("pred", "target", "noc", "out") if s4 else ())
    case(f"ar_loss_bwd-{tag}", ar_loss, bhw, True, safe4=("pred", "target", "noc", "coef", "grad_loss") if s4 else ())
    case(f"fakeobj_paste_crop-{tag}", fakeobj_paste, bhw, (1, 2, bhw[1] - 2, bhw[2] - 3),
         safe4=("flow", "cache_mask", "cache_img", "cache_motion", "slot", "param") if s4 else ())
    case(f"fakeobj_push-{tag}", fakeobj_push, bhw,
         safe4=("flow", "slot", "cache_mask", "cache_img", "cache_motion") if s4 else ())
for tag, shp in (("odd", ODD), ("vec", VEC)):
    s4 = tag == "odd"
    case(f"segpool_fwd-{tag}", segpool, shp, 5, False, safe4=("state",) if s4 else ())  # K = 5: no multiple of a tile
    case(f"segpool_bwd-{tag}", segpool, shp, 5, True, safe4=("state",) if s4 else ())
    case(f"convepi_fwd-{tag}-act", convepi_fwd, shp, 0.1, safe4=("bias",) if s4 else ())
    case(f"convepi_fwd-{tag}-bias", convepi_fwd, shp, 1.0)
    case(f"convepi_bwd-{tag}-act-bias", convepi_bwd, shp, 0.1, True, safe4=("grad_out", "grad_bias") if s4 else ())
    case(f"convepi_bwd-{tag}-act", convepi_bwd, shp, 0.1, False)
    case(f"convepi_bwd-{tag}-bias", convepi_bwd, shp, 1.0, True)
case("convepi_bwd-split-act-bias", convepi_bwd, (2, 3, 40, 60), 0.1, True, safe4=("workspace",))  # workspace > 0
for entry in ("fit", "loss_fwd", "loss_bwd"):
    s4 = {"fit": ("flow", "records"), "loss_fwd": ("flow", "records", "out"), "loss_bwd": ("flow", "records", "grad_loss")}
    case(f"hg_{entry}-12x19", hg, HG_BHW, entry, safe4=s4[entry])
    case(f"hg_{entry}-vec", hg, (2, 12, 16), entry)

CASES = [pytest.param(c, (), id=c.id) for c in _T]
# one guarded case per parameter declared 4-byte aligned, one word off the 16-byte boundary
CASES += [pytest.param(c, (name,), id=f"{c.id}-misalign:{name}") for c in _T for name in c.safe4]


def _run(c, dev, guarded, mis=()):
    r = Run(Arena(dev) if guarded else Plain(dev), mis)
    res = c.fn(r, _lib.load(), _lib.stream_handle(dev), *c.args)
    torch.cuda.synchronize()
    return r, res


@pytest.mark.parametrize("c,mis", CASES)
def test_buffer_contract(hip_device, c, mis):
    dev = hip_device
    ops.device_errors(dev)
    plain, pres = _run(c, dev, False)
    guard, gres = _run(c, dev, True, mis)
    err = _lib.load().usf_last_error_string().decode()
    for res in (pres, gres):  # 1: both calls succeed
        assert all(v == 0 for v in (res.rc if isinstance(res.rc, list) else [res.rc])), (res.rc, err)
    assert ops.device_errors(dev) == 0
    guard.alloc.check()  # 2: every guard word intact
    for r in (plain, guard):  # 3: inputs unchanged, bit for bit
        for name, t, before in r.inputs:
            exact(f"input {name}", t, before)
    for name, t in guard.outputs.items():  # 4: every output element written
        assert guard.alloc.poisoned(t) == 0, f"{name}: {guard.alloc.poisoned(t)} of {t.numel()} elements never written"
    assert set(guard.outputs) == set(plain.outputs)
    for name, t in guard.outputs.items():  # 5: the same numbers wherever the buffers lie
        gres.cmp.get(name, exact)(f"{name}, guarded vs plain", t, plain.outputs[name])
    for res in (pres, gres):  # 7: the persistent forms' second call, the in-place buffers' untouched parts
        if res.post:
            res.post()
    if not mis and pres.ref:  # 6: the plain run against the ops wrapper (or the oracle)
        ref = pres.ref()
        assert set(ref) == set(plain.outputs), (sorted(ref), sorted(plain.outputs))
        for name, v in ref.items():
            v = _dev(v, dev).reshape(plain.outputs[name].shape)
            pres.ref_cmp.get(name, exact)(f"{name}, plain vs reference", plain.outputs[name], v.to(plain.outputs[name].dtype))


def test_every_launching_entry_point_is_in_the_table():
    """The table names every launching entry point of the seven headers."""
    import inspect

    src = inspect.getsource(inspect.getmodule(test_buffer_contract))
    tables = (_lib._SIGNATURES, _lib.CENSUS_SYMBOLS, _lib.AR_SYMBOLS, _lib.SEGPOOL_SYMBOLS, _lib.HG_SYMBOLS,
              _lib.CONVEPI_SYMBOLS, _lib.FAKEOBJ_SYMBOLS)
    launching = [n for t in tables for n in t if n.endswith("_f32")]
    for name in launching:
        stem = name[len("usf_"):-len("_f32")]
        for kind in ("photo", "census"):
            stem = stem.replace(f"{kind}_loss_", "{kind}_loss_")
        assert f"usf_{stem}_f32" in src, name


# ---------------------------------------------- ops never forwards a misaligned 16-byte pointer --
def _tail(a, dev):
    """``a`` as the batch slice t[1:] of a tensor with one more sample: contiguous,
    and off the 16-byte boundary when a sample's float count is no multiple of 4."""
    a = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    t = torch.empty((a.shape[0] + 1,) + tuple(a.shape[1:]), device=dev, dtype=a.dtype)
    t[1:] = a.to(dev)
    v = t[1:]
    assert v.is_contiguous()
    if a[0].numel() % 4:  # an odd-sized sample: the slice cannot sit on a 16-byte boundary
        assert v.data_ptr() % 16 != 0, (tuple(a.shape), v.data_ptr() % 16)
    return v


def _same(a, b):
    a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    for x, y in zip(a, b):
        if x is not None or y is not None:
            exact("sliced vs fresh", x, y)


@pytest.mark.parametrize("family", ["corr", "warp", "occ", "photo", "census", "upsample", "convex", "ar", "segpool", "hg",
                                    "convepi", "fakeobj"])
def test_ops_realign_batch_slices(hip_device, family):
    """Inputs that are batch slices t[1:] of a (3, C, 5, 7) tensor are contiguous
    but only 4-byte aligned, and flow[:, 2:] of a [B,4,5,7] tensor is 8-byte
    aligned: ops copies the former where the C ABI wants 16 bytes and passes the
    latter in place. The results equal those of fresh allocations bit for bit."""
    dev = hip_device
    B, C, H, W = 2, 5, 5, 7
    shape = (B, C, H, W)
    T = lambda a: _tail(a, dev)  # noqa: E731
    F = lambda a: _dev(a, dev)  # noqa: E731
    f4 = F(_flow((B, 4, H, W), 300, 1.5))
    fl = f4[:, 2:]  # a channel slice: 8-byte aligned, batch stride 4*H*W
    assert fl.data_ptr() % 16 == 8
    flc = fl.contiguous()
    a, b_, g = hashrng.normal(shape, 301), hashrng.normal(shape, 302), hashrng.normal(shape, 303)
    if family == "corr":
        go = hashrng.normal((B, 9, H, W), 304)
        _same(ops.corr_forward(T(a), T(b_), 1), ops.corr_forward(F(a), F(b_), 1))
        _same(ops.corr_backward(T(a), T(b_), T(go), 1), ops.corr_backward(F(a), F(b_), F(go), 1))
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.corr_forward(F(a), F(b_), 1, out=T(go))
    elif family == "warp":
        _same(ops.warp_forward(T(a), fl), ops.warp_forward(F(a), flc))
        ops.clear_persistent_workspaces()
        one = ops.warp_backward(T(a), fl, T(g))
        ops.clear_persistent_workspaces()
        _same(one, ops.warp_backward(F(a), flc, F(g)))
    elif family == "occ":
        _same(ops.splat_map(fl), ops.splat_map(flc))
        _same(ops.occ_bidirection(fl, f4[:, :2]), ops.occ_bidirection(flc, f4[:, :2].contiguous()))
    elif family in ("photo", "census"):
        im1, im2, m = hashrng.uniform((B, 3, H, W), 305), hashrng.uniform((B, 3, H, W), 306), hashrng.uniform((B, 1, H, W), 307)
        fwd, bwd = getattr(ops, f"{family}_loss_forward"), getattr(ops, f"{family}_loss_backward")
        o1, b1 = fwd(T(im1), T(im2), T(m), fl, need_grad=True)
        o2, b2 = fwd(F(im1), F(im2), F(m), flc, need_grad=True)
        _same((o1, b1), (o2, b2))
        gl = torch.ones(1, device=dev)
        _same(bwd(T(b2.cpu()), o2, gl), bwd(b2, o2, gl))
    elif family == "upsample":
        _same(ops.flow_upsample(T(a), 2), ops.flow_upsample(F(a), 2))
        big = hashrng.normal((B, 1, 3, 9), 308)  # the gradient of a [B,1,1,3] flow at factor 3: 27 floats per sample
        _same(ops.flow_upsample_backward(T(big), 3), ops.flow_upsample_backward(F(big), 3))
        big2 = hashrng.normal((B, 1, 3, 9), 309)
        _same(ops.flow_upsample_backward(T(big), 3, T(big2)), ops.flow_upsample_backward(F(big), 3, F(big2)))
    elif family == "convex":
        fw, mk = hashrng.normal((B, 2, H, W), 310), hashrng.normal((B, 36, H, 5), 311)  # 70 / 900 floats per sample
        mk7 = hashrng.normal((B, 36, H, W), 312)
        go = hashrng.normal((B, 2, 2 * H, 2 * W), 313)
        _same(ops.convex_upsample(T(fw), F(mk7), 2), ops.convex_upsample(F(fw), F(mk7), 2))
        _same(ops.convex_upsample_backward(T(fw), F(mk7), F(go), 2), ops.convex_upsample_backward(F(fw), F(mk7), F(go), 2))
        assert mk.size  # (a mask holds 9 f^2 planes: every sample of it starts on a 16-byte boundary)
    elif family == "ar":
        i1, i2, af, am = ar_util.inputs(B, H, W, 314)
        th = F(ar_util.explicit_thetas(B))
        _same(ops.ar_transform(T(i1), T(i2), fl, T(am), th), ops.ar_transform(F(i1), F(i2), flc, F(am), th))
    elif family == "segpool":
        seg = _seg_ids(B, H, W, 5, 315)
        s1, st1 = ops.segpool_forward(T(a), T(seg), 5)
        s2, st2 = ops.segpool_forward(F(a), F(seg), 5)
        _same((s1, st1), (s2, st2))
        _same(ops.segpool_backward(T(a), T(seg), st2, T(g), 5), ops.segpool_backward(F(a), F(seg), st2, F(g), 5))
    elif family == "hg":
        af, asg, ao, K = _hg_scene((B, H, W))
        f4h = torch.zeros((B, 4, H, W), device=dev)
        f4h[:, 2:] = F(af)
        r1 = ops.hg_fit(f4h[:, 2:], T(asg), T(ao), K, 0.5, 16, 3)
        r2 = ops.hg_fit(F(af), F(asg), F(ao), K, 0.5, 16, 3)
        _same(r1, r2)
        _same(ops.hg_loss_forward(f4h[:, 2:], T(asg), r2).reshape(1), ops.hg_loss_forward(F(af), F(asg), r2).reshape(1))
    elif family == "convepi":
        bias = F(hashrng.normal((C,), 316))
        y = ops.conv_epilogue_forward(F(a), bias, 0.1)
        _same(ops.conv_epilogue_backward(T(g), T(y.cpu()), 0.1), ops.conv_epilogue_backward(F(g), y, 0.1))
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.conv_epilogue_forward(T(a), bias, 0.1)
    else:
        i1, i2, af, an = fakeobj_util.base(B, H, W, 317)
        om, oi, mo = fakeobj_util.objects(4, H, W, 318)
        slot = torch.tensor([1, 2], dtype=I32, device=dev)
        par = F(fakeobj_util.plain_params(2))
        args = (F(om), F(oi), F(mo), slot, par, (3, 4), (1, 2))
        _same(ops.fakeobj_paste_crop(T(i1), T(i2), fl, T(an), *args), ops.fakeobj_paste_crop(F(i1), F(i2), flc, F(an), *args))
