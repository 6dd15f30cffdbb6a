"""Guard-band placement of device buffers (tests/test_gpu_buffer_contract.py).

An :class:`Arena` is ONE device allocation of 32-bit words that holds every
buffer of one call to a C entry point. The arena starts out filled with
``POISON`` (0x7FC5A5A5: a quiet NaN as float32, an implausible value as an
int). ``place`` carves typed views out of it:

* a view starts on a 16-byte boundary (``misalign=k`` shifts it by k words);
* its trailing guard begins at the very next word after its last element, so
  an overrun of one float lands in a guard;
* the guard before and after every buffer is at least ``max(4096, 2 * plane)``
  words, ``plane`` = product of the buffer's two innermost dimensions, so a
  wrong row or channel index still lands in a guard (a condition, not a
  measurement);
* with ``keep=`` (a tuple of slices of the placed shape) only that slice
  belongs to the buffer: the rest of the parent stays poison and is guard too
  (the correlation's concat slice, the conv epilogue's gradient slice).

``check`` compares every word that no buffer owns with the pattern through
the int32 view (NaN != NaN) and names the nearest buffer, the side and the
offset of the first damaged word. ``poisoned`` counts the elements of a view
that still hold the pattern (an output element never written).

:class:`Plain` has the same ``place`` but gives every buffer its own ordinary
torch allocation (``fill=None``: zeros), for the unguarded run of the same call.
"""
import numpy as np
import torch

POISON = 0x7FC5A5A5
MIN_GUARD = 4096


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _fill(view, fill):
    if fill is None:
        return
    if isinstance(fill, str):
        assert fill == "zero", fill
        view.zero_()
        return
    t = torch.from_numpy(np.ascontiguousarray(fill)) if isinstance(fill, np.ndarray) else fill
    assert tuple(t.shape) == tuple(view.shape) and t.dtype == view.dtype, (t.shape, t.dtype, view.shape, view.dtype)
    view.copy_(t)


class Plain:
    """Every buffer its own torch allocation; outputs and scratch zero-filled."""

    guarded = False

    def __init__(self, device):
        self.device = device

    def place(self, shape, dtype=torch.float32, fill=None, name="", misalign=0, keep=None):
        assert misalign == 0, "a plain allocation cannot be shifted"
        t = torch.zeros(tuple(shape), device=self.device, dtype=dtype)
        if keep is not None:
            t = t[keep]
        _fill(t, fill)
        return t

    def check(self):
        pass

    def poisoned(self, view):
        return 0


class Arena:
    """One poison-filled device allocation of ``words`` 32-bit words."""

    guarded = True

    def __init__(self, device, words=1 << 22):
        self.device = device
        self.words = torch.full((words,), POISON, device=device, dtype=torch.int32)
        assert self.words.data_ptr() % 16 == 0
        self.owned = torch.zeros(words, device=device, dtype=torch.bool)
        self.buffers = []  # (name, first word, words, guard words)
        self._end = 0  # first word after the last placed buffer
        self._end_guard = 0  # the guard that buffer asked for

    def place(self, shape, dtype=torch.float32, fill=None, name="", misalign=0, keep=None):
        shape = tuple(int(s) for s in shape)
        n = _numel(shape)
        assert n > 0, (name, shape)
        esize = torch.empty((), dtype=dtype).element_size()
        nwords = (n * esize + 3) // 4
        plane = _numel(shape[-2:])
        guard = max(MIN_GUARD, 2 * plane)
        start = self._end + max(guard, self._end_guard)
        start = (start + 3) // 4 * 4 + int(misalign)  # 16-byte boundary (+ the requested shift)
        assert (start * 4) % esize == 0, f"{name}: misalign={misalign} breaks the {dtype} element alignment"
        if start + nwords + guard > self.words.numel():
            raise MemoryError(f"arena of {self.words.numel()} words too small for {name} {shape}")
        raw = self.words[start:start + nwords]
        typed = raw.view(dtype) if dtype != torch.int32 else raw
        view = typed[:n].view(shape)
        own = self.owned[start:start + nwords]
        if keep is None:
            own.fill_(True)
        else:
            assert esize == 4, "strided placements hold 32-bit elements"
            own.view(shape)[keep] = True
            view = view[keep]
        _fill(view, fill)
        self.buffers.append((name or f"buffer{len(self.buffers)}", start, nwords, guard))
        self._end, self._end_guard = start + nwords, guard
        return view

    def _describe(self, idx):
        """The nearest buffer to arena word ``idx``, the side and the offset."""
        best = None
        for name, start, nwords, _ in self.buffers:
            if idx < start:
                side, off = "before", start - idx
            elif idx >= start + nwords:
                side, off = "after", idx - (start + nwords)
            else:
                side, off = "between the slices of", idx - start
            dist = 0 if side.startswith("between") else off + (0 if side == "after" else -1)
            if best is None or dist < best[0]:
                best = (dist, name, side, off)
        return best[1:]

    def check(self):
        """Every word outside the placed buffers still holds the pattern.
        Call after torch.cuda.synchronize()."""
        bad = (self.words != POISON) & ~self.owned
        nbad = int(bad.sum())
        if nbad:
            idx = int(torch.nonzero(bad)[0])
            name, side, off = self._describe(idx)
            val = int(self.words[idx]) & 0xFFFFFFFF
            where = {"before": f"{off} word(s) before the start of", "after": f"at word offset {off} after the end of",
                     "between the slices of": f"at word offset {off} of the parent, between the slices of"}[side]
            raise AssertionError(f"guard damaged: {nbad} word(s), the first {where} '{name}' "
                                 f"(arena word {idx}, value 0x{val:08X})")

    def poisoned(self, view):
        """Number of elements of ``view`` (a view of this arena) that still hold the pattern."""
        esize = view.element_size()
        v = view.contiguous()
        if esize == 4:
            return int((v.view(torch.int32) == POISON).sum())
        if esize == 8:
            return int((v.view(torch.int32).view(-1, 2) == POISON).all(dim=1).sum())
        assert esize == 1 and v.numel() % 4 == 0, "byte buffers in whole words"
        return int((v.view(-1).view(torch.int32) == POISON).sum())
