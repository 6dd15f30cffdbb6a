"""Helpers of the homography smoothness tests (tests/test_hg_cpu.py,
tests/test_gpu_hg.py, tests/golden/make_golden_hg.py): the stub estimator of the
golden, the selection and the drop rules in plain numpy, the planted scene,
hand-made records and the golden's inputs."""
import numpy as np
import torch

from oracle import hashrng

SLOTS, WORDS = 6, 16
ACCEPTED, FEW_RELIABLE, LOW_RELIABLE, LOW_INLIER, DEGENERATE, EMPTY = range(6)


# ------------------------------------------------------ the golden's stub --
def lsq_homography(pts1, pts2):
    """Plain fp64 least squares of the h33 = 1 system over all the given pairs -> [3, 3]."""
    p1, p2 = np.asarray(pts1, dtype=np.float64), np.asarray(pts2, dtype=np.float64)
    x, y, u, v = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    z, o = np.zeros_like(x), np.ones_like(x)
    A = np.concatenate([np.stack([x, y, o, z, z, z, -x * u, -y * u], 1), np.stack([z, z, z, x, y, o, -x * v, -y * v], 1)])
    h = np.linalg.lstsq(A, np.concatenate([u, v]), rcond=None)[0]
    return np.append(h, 1.0).reshape(3, 3)


def transfer_error(H, pts1, pts2):
    p1, p2 = np.asarray(pts1, dtype=np.float64), np.asarray(pts2, dtype=np.float64)
    q = np.concatenate([p1, np.ones((len(p1), 1))], 1) @ np.asarray(H, dtype=np.float64).reshape(3, 3).T
    return np.sqrt(((q[:, :2] / q[:, 2:3] - p2) ** 2).sum(1))


def stub_estimator(calls):
    """``find_homography(pts1, pts2, thr, sample, slot)`` of the golden: the least-squares fit over the
    points it is given, ``mask = residual <= thr``; appends (n_points, H) to ``calls``."""
    def find_homography(pts1, pts2, thr, sample=None, slot=None):
        H = lsq_homography(pts1, pts2)
        calls.append((len(pts1), H.copy()))
        return H, transfer_error(H, pts1, pts2) <= thr
    return find_homography


# ------------------------------------------------- selection, plain numpy --
def select_np(seg, occ, K):
    """Per sample: (counts [3, K]: pixels / occluded / reliable, ids [6], statuses [6] after the drop
    rules, -1 = goes on to the fit). seg, occ: [B, 1, h, w] arrays; ids outside [0, K) are ignored."""
    out = []
    for s, o in zip(np.asarray(seg)[:, 0], np.asarray(occ)[:, 0]):
        cnt = np.zeros((3, K), dtype=np.int64)
        for k in range(K):
            m = s == k
            cnt[0, k] = m.sum()
            cnt[1, k] = (m & (o != 0)).sum()
            cnt[2, k] = (m & ((np.float32(1) - o) != 0)).sum()
        order = sorted(range(1, K), key=lambda k: (-cnt[1, k], k))[:SLOTS]
        ids = order + [-1] * (SLOTS - len(order))
        st = []
        for k in ids:
            if k < 0:
                st.append(EMPTY)
            elif cnt[2, k] < 4:
                st.append(FEW_RELIABLE)
            elif 5 * cnt[2, k] < cnt[0, k]:
                st.append(LOW_RELIABLE)
            else:
                st.append(-1)
        out.append((cnt, ids, st))
    return out


def slot_pairs(flow, seg, occ, b, k):
    """(pts1, pts2) float32 [n, 2] of the reliable pixels of segment k of sample b, raster order."""
    f, s, o = np.asarray(flow)[b], np.asarray(seg)[b, 0], np.asarray(occ)[b, 0]
    ys, xs = np.nonzero((s == k) & ((np.float32(1) - o) != 0))
    p1 = np.stack([xs, ys], 1).astype(np.float32)
    return p1, p1 + np.stack([f[0, ys, xs], f[1, ys, xs]], 1).astype(np.float32)


def all_pixels(h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)


def apply_h(H, pts):
    q = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ np.asarray(H, dtype=np.float64).reshape(3, 3).T
    return q[:, :2] / q[:, 2:3]


def make_records(B, entries):
    """int32 [B, 6, 16] records from {(b, slot): (id, status, H [3, 3])}; the rest are empty slots."""
    rec = np.zeros((B, SLOTS, WORDS), dtype=np.int32)
    rec[:, :, 0], rec[:, :, 1], rec[:, :, 14] = -1, EMPTY, -1
    for (b, s), (k, status, H) in entries.items():
        rec[b, s, 0], rec[b, s, 1] = k, status
        rec[b, s, 5:14] = np.asarray(H, dtype=np.float32).reshape(9).view(np.int32)
    return torch.from_numpy(rec)


# --------------------------------------------------------- planted scene --
def random_homography(seed, cx, cy):
    """Rotation, scale, shear about (cx, cy), a translation and perspective terms up to 1e-4."""
    r = hashrng.symmetric((8,), seed).astype(np.float64)
    th, sc, sh = 0.05 * r[0], 1.0 + 0.05 * r[1], 0.03 * r[2]
    A = sc * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) @ np.array([[1.0, sh], [0.0, 1.0]])
    t = np.array([cx, cy]) - A @ np.array([cx, cy]) + 6.0 * r[3:5]
    H = np.array([[A[0, 0], A[0, 1], t[0]], [A[1, 0], A[1, 1], t[1]], [1e-4 * r[5], 1e-4 * r[6], 1.0]])
    return H / H[2, 2]


def planted_scene(seed=4100, B=2, h=64, w=96):
    """flow [B,2,h,w], seg, occ [B,1,h,w] (float32 tensors), K = 7 and, per (sample, id), a dict with the
    planted H, the reliable pairs' planted-inlier mask (raster order) and the kind of the segment.

    Six 28x28 segments (ids 1..6) sit in 32x32 cells, the rest is id 0. Ids 1..5 follow one
    homography each with +-0.02 px noise, 30 % of their reliable pixels displaced by 5..10 px; in
    sample 0 id 6 has 60 % such outliers, in sample 1 id 6 is a 2x2 block. Segment k has 10 + 7 k
    occluded pixels (distinct counts), whose flow is displaced as well."""
    flow = np.zeros((B, 2, h, w), dtype=np.float32)
    seg = np.zeros((B, 1, h, w), dtype=np.float32)
    occ = np.zeros((B, 1, h, w), dtype=np.float32)
    planted = {}
    for b in range(B):
        for k in range(1, 7):
            cy, cx = divmod(k - 1, 3)
            y0, x0 = 32 * cy + 2, 32 * cx + 2
            block = b == 1 and k == 6
            ys, xs = np.mgrid[y0:y0 + (2 if block else 28), x0:x0 + (2 if block else 28)]
            ys, xs = ys.ravel(), xs.ravel()
            n = len(ys)
            s = seed + 100 * b + 10 * k
            H = random_homography(s, x0 + 14.0, y0 + 14.0)
            p1 = np.stack([xs, ys], 1).astype(np.float64)
            f = apply_h(H, p1) - p1 + 0.02 * hashrng.symmetric((n, 2), s + 1).astype(np.float64)
            perm = np.argsort(hashrng.uniform((n,), s + 2), kind="stable")
            n_occ = 0 if block else 10 + 7 * k
            share = 0.0 if block else (0.6 if (b == 0 and k == 6) else 0.3)
            n_out = int(round(share * (n - n_occ)))
            moved = perm[:n_occ + n_out]
            ang = 2 * np.pi * hashrng.uniform((n,), s + 3).astype(np.float64)
            rad = 5.0 + 5.0 * hashrng.uniform((n,), s + 4).astype(np.float64)
            f[moved] += (rad[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1))[moved]
            flow[b, 0, ys, xs], flow[b, 1, ys, xs] = f[:, 0], f[:, 1]
            seg[b, 0, ys, xs] = k
            is_occ = np.zeros(n, dtype=bool)
            is_occ[perm[:n_occ]] = True
            occ[b, 0, ys, xs] = is_occ
            inl = np.ones(n, dtype=bool)
            inl[moved] = False
            kind = "block" if block else ("outliers" if share > 0.5 else "plane")
            planted[(b, k)] = dict(H=H, inliers=inl[~is_occ], kind=kind)
    return torch.from_numpy(flow), torch.from_numpy(seg), torch.from_numpy(occ), 7, planted


# -------------------------------------------------------- golden's inputs --
GOLDEN_CASES = {"b2_24x40": (2, 24, 40, 9, 6100), "b1_5x7": (1, 5, 7, 4, 6200)}  # B, h, w, K, seed
GOLDEN_THR = 0.5


def golden_inputs(name):
    """(flow, seg, occ) float32 tensors of a golden case, a pure function of its name.

    The flow is a smooth affine field plus +-0.2 px noise. b2_24x40: ids 0..7 in vertical strips of 5
    columns and a 5x3 patch of id 8, with distinct occluded counts (120, 117, 100, 30, 22, 15, 9, 5, 4),
    id 0 holding the largest, so eight candidates compete for six slots: id 1 keeps 3 reliable pixels,
    id 2 a share of 1/6, id 3 has two thirds of its reliable flow scattered by +-4 px so that the
    least-squares stub finds an inlier share below 0.5 at thr = 0.5, ids 4, 5, 6 are fitted and ids 7, 8
    get no slot. b1_5x7: ids 1, 2, 3 (4, 21 and 8 pixels in raster order after 2 of id 0) with 1, 17
    and 0 occluded pixels: 3 reliable, a share of 4/21, and all of id 3 scattered."""
    B, h, w, K, seed = GOLDEN_CASES[name]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    flow = np.zeros((B, 2, h, w))
    seg = np.zeros((B, 1, h, w), dtype=np.float32)
    occ = np.zeros((B, 1, h, w), dtype=np.float32)
    for b in range(B):
        flow[b, 0] = 1.5 + 0.03 * xs - 0.02 * ys + 0.3 * b
        flow[b, 1] = -0.8 + 0.01 * xs + 0.04 * ys
        flow[b] += 0.2 * hashrng.symmetric((2, h, w), seed + b).astype(np.float64)
        if name == "b2_24x40":
            cols = xs if b == 0 else 39 - xs  # sample 1 is mirrored
            ids = np.where((cols >= 35) & (ys < 3), 8, cols // 5)
            n_occ = {0: 120, 1: 117, 2: 100, 3: 30, 4: 22, 5: 15, 6: 9, 7: 5, 8: 4}
            keep_every = 3  # a third of id 3 stays on the plane
        else:
            r = ys * w + xs
            ids = np.where(r < 2, 0, np.where(r < 6, 1, np.where(r < 27, 2, 3)))
            n_occ = {0: 2, 1: 1, 2: 17, 3: 0}
            keep_every = 10 ** 6
        seg[b, 0] = ids
        for k, c in n_occ.items():  # the first c pixels of the segment in raster order
            py, px = np.nonzero(seg[b, 0] == k)
            occ[b, 0, py[:c], px[:c]] = 1
        py, px = np.nonzero((seg[b, 0] == 3) & (occ[b, 0] == 0))
        jit = 4.0 * hashrng.symmetric((2, len(py)), seed + 50 + b).astype(np.float64)
        move = np.arange(len(py)) % keep_every != 0
        flow[b, 0, py[move], px[move]] += jit[0][move]
        flow[b, 1, py[move], px[move]] += jit[1][move]
    return (torch.from_numpy(flow.astype(np.float32)), torch.from_numpy(seg), torch.from_numpy(occ))
