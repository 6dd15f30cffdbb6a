"""Shared by the segpool tests: the contract of include/unsamflow_hip_segpool.h
as a plain per-segment loop, and the test inputs."""
import torch


def loop_reference(proj, seg, grad_spread=None, num_segments=None):
    """(spread, grad_proj) by the contract, one (sample, channel, segment) at a
    time, in proj's dtype. Pixels whose id is not an integer in [0, K) belong to
    no segment."""
    B, C, h, w = proj.shape
    K = int(seg.max()) + 1 if num_segments is None else int(num_segments)
    hw = h * w
    x = proj.reshape(B, C, hw)
    s = seg.reshape(B, hw).to(torch.float64)
    g = None if grad_spread is None else grad_spread.reshape(B, C, hw)
    spread = torch.zeros_like(x)
    grad = torch.zeros_like(x)
    for b in range(B):
        for k in range(K):
            S = s[b] == k
            n_in = int(S.sum())
            if n_in == 0:
                continue
            n_out = hw - n_in
            for c in range(C):
                m = x[b, c][S].max()
                pooled = m if n_out == 0 else torch.clamp(m, min=0)
                spread[b, c][S] = pooled
                if g is None:
                    continue
                G = g[b, c][S].sum()
                ties = S & (x[b, c] == pooled)
                z = n_out if float(pooled.detach()) == 0.0 else 0
                t = int(ties.sum())
                if t:
                    grad[b, c][ties] = G / (t + z)
    return spread.reshape(B, C, h, w), grad.reshape(B, C, h, w)


def block_segments(B, h, w, K, block, gen, ids=None):
    """[B,1,h,w] fp32 ids, constant over block x block pixel blocks, drawn from
    ``ids`` (default: all of [0, K))."""
    ids = torch.arange(K) if ids is None else torch.as_tensor(ids)
    hb, wb = -(-h // block), -(-w // block)
    pick = ids[torch.randint(0, len(ids), (B, 1, hb, wb), generator=gen)]
    seg = pick.repeat_interleave(block, dim=2).repeat_interleave(block, dim=3)[:, :, :h, :w]
    return seg.to(torch.float32).contiguous()


def values(shape, gen, quantised):
    """randn, or round(4 randn) / 4: ties, exact zeros and all-negative segments are frequent."""
    x = torch.randn(shape, generator=gen)
    return torch.round(4 * x) / 4 if quantised else x


def input_features(proj, seg, num_segments):
    """(ties, zeros, all_negative): does some segment hold its pooled value more
    than once, is some value exactly 0, is some segment that does not cover its
    sample negative throughout."""
    B, C, h, w = proj.shape
    x, s = proj.reshape(B, C, -1), seg.reshape(B, -1)
    ties = all_negative = False
    for b in range(B):
        for k in torch.unique(s[b]).tolist():
            S = s[b] == k
            if not 0 <= k < num_segments or k != int(k):
                continue
            v = x[b][:, S]  # [C, n_in]
            m = v.max(dim=1, keepdim=True).values
            partial = int(S.sum()) < h * w
            pooled = torch.clamp(m, min=0) if partial else m
            ties |= bool(((v == pooled).sum(dim=1) > 1).any())
            all_negative |= partial and bool((m < 0).any())
    return ties, bool((x == 0).any()), all_negative


def force_negative_segment(proj, seg, b=0, c=0):
    """Make channel c of the segment holding sample b's first pixel negative throughout (in place)."""
    S = seg[b, 0] == seg[b, 0, 0, 0]
    proj[b, c][S] = -proj[b, c][S].abs() - 0.25
