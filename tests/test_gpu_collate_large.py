"""GPU: the collate launch with more than 2^31 elements on either side (in the manner of tests/test_gpu_large_offsets.py).

CoRow::src_off and the element index r * row_len + e of ``out`` are 64-bit; no other test makes the upper dword of either non-zero.
First call: the source items lie where tests/_large_buffers.py puts them in an arena of 2^31 + 2^24 floats (8.06 GiB) -- astride and
behind float 2^29, 2^30 and 2^31.  Second call: a binary16 ``out`` of 2049 rows of 2^20 + 3 elements (4.0 GiB), row 2047 astride element
2^31, row 2048 behind it; every row not under test has ``src_len == 0``, so the run only stores zeros there.  The bar is derived: each
result is bit-equal to the same rows collated from a small near twin (same offsets modulo 4), which is bit-equal to ``collate_ref``."""
import numpy as np
import pytest
import torch

import _large_buffers as LB
from _collate_ref import bits_of, collate_ref

from lhotse_amd import augmentation as A

pytestmark = pytest.mark.gpu
CHUNK = 2 ** 28
NEED_FREE = 14 << 30
T = A.COLLATE_TILE


def _sig(seed, n):
    return (np.random.RandomState(seed).rand(int(n)).astype(np.float32) - np.float32(0.5)).astype(np.float32)


def test_sources_and_a_destination_row_astride_element_2_31():
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"the large collate test needs 14 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    torch.cuda.reset_peak_memory_stats()
    # ---- sources past 2^31 ------------------------------------------------------------------------------------------------------
    lens = [257, 2 * T + 7, 4099, T + 1, 12289, 3 * T + 5, T - 1]
    p = LB.place(lens)
    LB.check(p)
    xs = [_sig(900 + i, n) for i, n in enumerate(lens)]
    row_len = max(lens) + 3
    dst = np.minimum([0, 1, 2, 3, 5, 0, 9], row_len - np.asarray(lens))

    def run(arena, offs, dtype):
        for o, x in zip(offs, xs):
            arena[int(o) : int(o) + len(x)] = torch.from_numpy(x).cuda()
        res, _ = A.collate_in_arena(arena, offs, lens, row_len=row_len, dst_offsets=dst, dtype=dtype)
        torch.cuda.synchronize()
        return res

    near_arena = torch.full((p.near_size,), 0.25, device="cuda")
    near = {dt: run(near_arena, p.near, dt) for dt in (torch.float32, torch.bfloat16)}
    host = near_arena.cpu().numpy()
    for dt, res in near.items():
        assert np.array_equal(bits_of(res), bits_of(collate_ref(host, p.near, lens, row_len, dst, dt)))
    far_arena = torch.empty(LB.BUFFER_ELEMS, dtype=torch.float32, device="cuda")
    far_arena.fill_(0.25)
    for dt in near:
        far = run(far_arena, p.far, dt)
        assert torch.equal(far.view(torch.int32 if dt == torch.float32 else torch.int16), near[dt].view(torch.int32 if dt == torch.float32 else torch.int16)), str(dt)
    inside = sum(int((far_arena[int(o) : int(o) + n] != 0.25).sum()) for o, n in zip(p.far, lens))
    changed = sum(int((c != 0.25).sum()) for c in far_arena.split(CHUNK))
    assert changed == inside  # the arena is only read
    print(f"[far] hipfeat_collate_run: read up to element {p.far[-1] + lens[-1] - 1} (2^31 + {p.far[-1] + lens[-1] - 1 - 2 ** 31})")
    del far_arena, far
    torch.cuda.empty_cache()
    # ---- a destination row astride element 2^31 of out ----------------------------------------------------------------------------
    rows, row_len = 2049, 2 ** 20 + 3
    astride = 2 ** 31 // row_len
    assert astride == 2047 and astride * row_len < 2 ** 31 < (astride + 1) * row_len and rows * row_len > 2 ** 31
    under_test = [0, astride, astride + 1]
    item_lens = [row_len - 2, row_len, row_len - 7]  # (the row astride the mark is full: the store that crosses it carries samples)
    item_dst = [2, 0, 3]
    arena_h, item_offs = np.full(3 * row_len + 64, 0.25, dtype=np.float32), []
    pos = 5
    for k, n in enumerate(item_lens):
        item_offs.append(pos)
        arena_h[pos : pos + n] = _sig(950 + k, n)
        pos += n + 1 + k
    arena = torch.from_numpy(arena_h).cuda()
    so, sl, do = np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int64)
    so[under_test], sl[under_test], do[under_test] = item_offs, item_lens, item_dst
    guard = 64
    big = torch.empty(rows * row_len + guard, dtype=torch.int16, device="cuda")
    big.fill_(0x5A5A)
    out = big.view(torch.float16)[: rows * row_len]
    res, _ = A.collate_in_arena(arena, so, sl, row_len=row_len, dst_offsets=do, dtype=torch.float16, out=out)
    torch.cuda.synchronize()
    twin, _ = A.collate_in_arena(arena, item_offs, item_lens, row_len=row_len, dst_offsets=item_dst, dtype=torch.float16)
    torch.cuda.synchronize()
    assert np.array_equal(bits_of(twin), bits_of(collate_ref(arena_h, item_offs, item_lens, row_len, item_dst, torch.float16)))
    for k, r in enumerate(under_test):
        assert torch.equal(res[r].view(torch.int16), twin[k].view(torch.int16)), r
    # every other row is +0 (bits), counted on the device; nothing behind the end was written
    nonzero = sum(int((c != 0).sum()) for c in big[: rows * row_len].split(CHUNK))
    assert nonzero == sum(int((twin[k].view(torch.int16) != 0).sum()) for k in range(3))
    assert bool((big[rows * row_len :] == 0x5A5A).all())
    print(f"[far] hipfeat_collate_run: wrote up to element {rows * row_len - 1} (2^31 + {rows * row_len - 1 - 2 ** 31})")
    peak = torch.cuda.max_memory_allocated()
    print(f"[far] peak device memory: {peak / 2 ** 30:.2f} GiB")
    assert peak < 20 << 30, peak
