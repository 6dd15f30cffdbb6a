"""guard_util.Arena on a CPU tensor: the placement rules it promises, and that
the damage the guarded GPU tests look for (tests/test_gpu_buffer_contract.py)
is reported with the buffer, the side and the offset."""
import numpy as np
import pytest
import torch

from guard_util import MIN_GUARD, POISON, Arena, Plain

CPU = torch.device("cpu")


def test_pattern_is_a_quiet_nan():
    assert np.isnan(np.array([POISON], dtype=np.uint32).view(np.float32)[0])


def test_placement_alignment_guards_and_fill():
    a = Arena(CPU, 1 << 17)
    out = a.place((2, 3, 5, 7), torch.float32, None, name="out")
    data = np.arange(2 * 4 * 5 * 7, dtype=np.float32).reshape(2, 4, 5, 7)
    sl = a.place((2, 9, 5, 7), torch.float32, data, name="slice", keep=(slice(None), slice(2, 6)))
    w64 = a.place((10,), torch.int64, "zero", name="w64")
    big = a.place((1, 1, 60, 70), torch.float32, "zero", name="big")  # 2 * plane > MIN_GUARD
    mis = a.place((5,), torch.float32, None, name="mis", misalign=1)
    assert out.data_ptr() % 16 == 0 and w64.data_ptr() % 16 == 0 and big.data_ptr() % 16 == 0
    assert mis.data_ptr() % 16 == 4
    assert sl.shape == (2, 4, 5, 7) and sl.stride() == (9 * 35, 35, 7, 1) and torch.equal(sl, torch.from_numpy(data))
    assert a.poisoned(out) == out.numel() and a.poisoned(sl) == 0 and a.poisoned(w64) == 0
    starts = {name: (start, n, guard) for name, start, n, guard in a.buffers}
    assert starts["big"][2] == 2 * 60 * 70 and starts["out"][2] == MIN_GUARD
    order = sorted(starts.values())
    assert order[0][0] >= order[0][2]  # a guard in front of the first buffer
    for (s0, n0, g0), (s1, _, g1) in zip(order, order[1:]):
        assert s1 - (s0 + n0) >= max(g0, g1)  # each neighbour's guard fits between them
    assert a.words.numel() - (order[-1][0] + order[-1][1]) >= order[-1][2]
    a.check()
    out.fill_(1.0)
    assert a.poisoned(out) == 0
    out[1, 2, 4, 6] = torch.tensor([POISON], dtype=torch.int32).view(torch.float32)[0]
    assert a.poisoned(out) == 1  # one element never written
    a.check()


def test_one_float_past_the_end_is_caught():
    a = Arena(CPU, 1 << 16)
    a.place((3, 5, 7), torch.float32, None, name="first")
    out = a.place((2, 5, 7), torch.float32, None, name="out")
    flat = a.words.view(torch.float32)
    start = next(s for name, s, _, _ in a.buffers if name == "out")
    flat[start + out.numel()] = 2.5  # what a tail that stores one float too many does
    with pytest.raises(AssertionError, match=r"word offset 0 after the end of 'out'"):
        a.check()
    a.words[start + out.numel()] = POISON
    flat[start - 3] = 0.0  # and a store in front of the buffer
    with pytest.raises(AssertionError, match=r"3 word\(s\) before the start of 'out'"):
        a.check()


def test_a_write_between_the_slices_is_caught():
    a = Arena(CPU, 1 << 16)
    a.place((2, 9, 5, 7), torch.float32, "zero", name="cat", keep=(slice(None), slice(2, 6)))
    start = a.buffers[0][1]
    a.words[start + 9 * 35 + 1] = 0  # sample 1, channel 0: outside the slice
    with pytest.raises(AssertionError, match=r"word offset 316 of the parent, between the slices of 'cat'"):
        a.check()


def test_plain_allocations():
    p = Plain(CPU)
    t = p.place((2, 9, 5, 7), torch.float32, None, keep=(slice(None), slice(2, 6)))
    assert t.shape == (2, 4, 5, 7) and t.stride() == (9 * 35, 35, 7, 1) and float(t.abs().sum()) == 0.0
    assert p.poisoned(t) == 0
    p.check()
