"""CPU: the host arithmetic of ``lhotse_amd.augmentation.collate_in_arena`` -- the defaults of ``row_len`` and ``dst_offsets``,
``left_pad_offsets``, and every ``ValueError`` that is raised before anything is planned -- against the numpy statement of the launch,
``collate_ref`` (tests/_collate_ref.py).  No device is touched: the arenas are host tensors, and what would reach a device raises first."""
import numpy as np
import pytest
import torch

import lhotse_amd
from lhotse_amd import augmentation as A

from _collate_ref import bits_of, collate_ref


def test_names_are_exported():
    for name in ("HipCollator", "get_or_create_collator", "collate_in_arena", "left_pad_offsets", "COLLATE_TILE", "FusedAudioBatch", "HipAudioSamples"):
        assert hasattr(lhotse_amd, name) and name in lhotse_amd.__all__
    assert lhotse_amd.COLLATE_TILE == 4096


def test_collate_ref_is_zero_padding_of_bit_copies():
    arena = np.arange(1, 41, dtype=np.float32)
    arena[7] = np.float32(-0.0)
    arena.view(np.uint32)[9] = 0x7FA00001  # a signalling NaN: copied as bits
    ref = collate_ref(arena, [5, 20, 0], [6, 0, 3], dst_offsets=[1, 4, 0], row_len=8)
    assert ref.shape == (3, 8) and ref.dtype == torch.float32
    b = bits_of(ref)
    assert b[0].tolist() == [0] + arena[5:11].view(np.uint32).tolist() + [0] and not b[1].any() and b[2, :3].tolist() == arena[:3].view(np.uint32).tolist()
    assert b[0, 3] == 0x80000000 and b[0, 5] == 0x7FA00001
    # the defaults: the longest cut, right padding -- what torch's pad_sequence gives
    cuts = [torch.from_numpy(arena[5:11].copy()), torch.from_numpy(arena[20:20].copy()), torch.from_numpy(arena[0:3].copy())]
    assert np.array_equal(bits_of(collate_ref(arena, [5, 20, 0], [6, 0, 3])), bits_of(torch.nn.utils.rnn.pad_sequence(cuts, batch_first=True)))
    half = collate_ref(arena, [30], [6], dtype=torch.float16)
    assert half.dtype == torch.float16 and torch.equal(half[0], torch.from_numpy(arena[30:36].copy()).to(torch.float16))
    assert collate_ref(arena, [], []).shape == (0, 0)


def test_layout_defaults():
    so, sl, do, row_len = A.collate_layout(100, [0, 10, 50], [7, 0, 30])
    assert (so.dtype, sl.dtype, do.dtype) == (np.int64,) * 3 and row_len == 30 and do.tolist() == [0, 0, 0]  # the longest cut, right padding
    assert A.collate_layout(100, [], [])[3] == 0 and A.collate_layout(100, [3], [0])[3] == 0  # no rows / rows of nothing: 0
    assert A.collate_layout(100, [0], [7], row_len=12)[3] == 12
    assert A.collate_layout(80, [0, 10, 50], [7, 0, 30], 33, [26, 33, 3])[2].tolist() == [26, 33, 3]
    assert A.collate_layout(5, [3, 10 ** 12], [2, 0])[3] == 2  # (a row of padding reads nothing: its offset does not count)


def test_left_pad_offsets():
    lens = [0, 1, 5, 12]
    left = A.left_pad_offsets(lens, 12)
    assert left.dtype == np.int64 and left.tolist() == [12, 11, 7, 0]
    assert A.left_pad_offsets(lens, 15).tolist() == [15, 14, 10, 3] and A.left_pad_offsets([], 4).tolist() == []
    with pytest.raises(ValueError):
        A.left_pad_offsets(lens, 11)
    arena = np.arange(1, 31, dtype=np.float32)
    ref = collate_ref(arena, [0, 4, 8, 16], lens, 12, left)
    for i, n in enumerate(lens):  # every cut ends where its row ends, zeros in front
        assert not ref[i, : 12 - n].any() and np.array_equal(ref[i, 12 - n :].numpy(), arena[[0, 4, 8, 16][i] :][:n])


def test_errors_are_raised_before_anything_is_planned(monkeypatch):
    planned = []
    monkeypatch.setattr(A, "get_or_create_collator", lambda *a, **k: planned.append(1))
    arena = torch.zeros(64)
    bad = [
        dict(offsets=[0, 60], lengths=[8, 5]),  # the arena is too small
        dict(offsets=[0], lengths=[8], row_len=7),  # a cut longer than the row
        dict(offsets=[0], lengths=[8], row_len=10, dst_offsets=[3]),  # ... or that ends behind it
        dict(offsets=[-1], lengths=[8]), dict(offsets=[0], lengths=[-8]), dict(offsets=[0], lengths=[8], row_len=12, dst_offsets=[-1]),
        dict(offsets=[0, 8], lengths=[8]), dict(offsets=[0], lengths=[8], dst_offsets=[0, 0]),  # tables of unequal length
        dict(offsets=[0], lengths=[8], out=torch.zeros(7)),  # out= too small
        dict(offsets=[0, 8], lengths=[8, 8], row_len=9, out=torch.zeros(17)),
        dict(offsets=[0], lengths=[8], out=torch.zeros(8, dtype=torch.float16)),  # out= of another type
        dict(offsets=[0], lengths=[8], out=torch.zeros(16)[::2]),  # ... or not contiguous
        dict(offsets=[0], lengths=[8], out=arena[32:48]),  # out= inside the arena
        dict(offsets=[0], lengths=[8], dtype=torch.float64), dict(offsets=[0], lengths=[8], dtype=torch.int16),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            A.collate_in_arena(arena, **kw)
    assert not planned
    # no rows, and rows of nothing: an empty result, and nothing is planned or launched
    out, lens = A.collate_in_arena(arena, [], [])
    assert out.shape == (0, 0) and out.dtype == torch.float32 and lens.dtype == np.int64 and len(lens) == 0
    out, lens = A.collate_in_arena(arena, [3, 9], [0, 0], dtype=torch.bfloat16)
    assert out.shape == (2, 0) and out.dtype == torch.bfloat16 and lens.tolist() == [0, 0]
    assert A.collate_in_arena(arena, [], [], row_len=5)[0].shape == (0, 5)
    assert not planned
