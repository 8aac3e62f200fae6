"""GPU: the feature-mix launches with more than 2^31 elements on either side (in the manner of tests/test_gpu_collate_large.py).

FmTrack::src_off (a BYTE offset) and the element index c * row_len + e of ``out`` are 64-bit; no other test makes the upper dword of
either non-zero.  First call: the tracks lie where tests/_large_buffers.py puts them in an arena of 2^31 + 2^24 float32 elements (8.06 GiB)
-- astride and behind element 2^29, 2^30 and 2^31, i.e. byte 2^31, 2^32 and 2^33 -- as float32 and as binary16 tracks, in copy-form and
fold-form cuts (energies included).  Second call: an ``out`` of 2049 rows of 2^20 + 3 elements (8.0 GiB), row 2047 astride element 2^31,
row 2048 behind it; every row not under test is a cut of no frames, so the run only stores log(1e-10) there.  The bar is derived: each
result is bit-equal to the same cuts run from a small near twin (same offsets modulo 16 bytes), which tests/test_gpu_featmix.py holds to
the float64 truth."""
import numpy as np
import pytest
import torch

import _featmix_ref as R
import _large_buffers as LB

from lhotse_amd import augmentation as A
from lhotse_amd.augmentation import FEATMIX_COPY as COPY, FEATMIX_FOLD as FOLD, FeatCut, FeatTrack

pytestmark = pytest.mark.gpu
CHUNK = 2 ** 28
NEED_FREE = 14 << 30
F = 23


def _feats(seed, n, f16):
    m = np.random.RandomState(seed).uniform(-15.0, 5.0, (n, F)).astype(np.float32)
    return m.astype(np.float16) if f16 else m


def test_tracks_and_a_destination_row_astride_element_2_31():
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"the large feature-mix test needs 14 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    torch.cuda.reset_peak_memory_stats()
    # ---- tracks past 2^31 -------------------------------------------------------------------------------------------------------
    frames = [30, 750, 40, 200, 64, 720, 90]  # (750 x 23 and 720 x 23 floats: more than one energy item)
    f16 = [False, False, True, False, True, False, True]  # (a binary16 track takes half the floats it was given room for)
    p = LB.place([n * F for n in frames])
    LB.check(p)
    mats = [_feats(700 + i, n, h) for i, (n, h) in enumerate(zip(frames, f16))]

    def cuts_of(offs):
        t = [FeatTrack(int(o) * 4, n, None, h) for o, n, h in zip(offs, frames, f16)]
        return [FeatCut([t[0]], 32, COPY, pad_value=-5.0),
                FeatCut([t[1], t[2]._replace(first=100, snr=10.0)], 750, FOLD, ref_track=0),
                FeatCut([t[3]._replace(snr=3.0), t[4]._replace(first=20), t[5]._replace(first=30, snr=15.0)], 750, FOLD, ref_track=1, dst_first=1),
                FeatCut([t[6]], 90, COPY, dst_first=600)]

    def run(arena, offs):
        for o, m in zip(offs, mats):
            b = torch.from_numpy(m.reshape(-1).view(np.uint8)).cuda()
            arena[int(o) * 4: int(o) * 4 + b.numel()] = b
        res, _ = A.featmix_in_arena(arena, cuts_of(offs), F)
        torch.cuda.synchronize()
        return res

    near_arena = torch.full((p.near_size * 4,), 0x3B, dtype=torch.uint8, device="cuda")
    near = run(near_arena, p.near)
    truth = R.batch(near_arena.cpu().numpy(), cuts_of(p.near), F)
    assert np.abs(near.cpu().numpy().astype(np.float64) - truth).max() < 1e-5  # (the near twin itself is sane; its bar: test_gpu_featmix.py)
    far_arena = torch.empty(LB.BUFFER_ELEMS * 4, dtype=torch.uint8, device="cuda")
    far_arena.fill_(0x3B)
    far = run(far_arena, p.far)
    assert torch.equal(far.view(torch.int32), near.view(torch.int32))
    inside = sum(int((far_arena[int(o) * 4: int(o) * 4 + m.nbytes] != 0x3B).sum()) for o, m in zip(p.far, mats))
    changed = sum(int((c != 0x3B).sum()) for c in far_arena.split(CHUNK * 4))
    assert changed == inside  # the arena is only read
    last = int(p.far[-1]) * 4 + mats[-1].nbytes - 1
    print(f"[far] hipfeat_featmix_run: read up to byte {last} (2^33 + {last - 2 ** 33})")
    assert last > 2 ** 33
    del far_arena, far
    torch.cuda.empty_cache()
    # ---- a destination row astride element 2^31 of out ----------------------------------------------------------------------------
    rows, row_len = 2049, 2 ** 20 + 3  # F = 1: a row of 2^20 + 3 frames
    astride = 2 ** 31 // row_len
    assert astride == 2047 and astride * row_len < 2 ** 31 < (astride + 1) * row_len and rows * row_len > 2 ** 31
    under_test = [0, astride, astride + 1]
    rs = np.random.RandomState(77)
    a, b, c, d = (rs.uniform(-15.0, 5.0, n).astype(np.float32) for n in (row_len - 2, row_len, 4099, row_len - 7))
    buf, offs = bytearray(b"\x00" * 4), []
    for m in (a, b, c.astype(np.float16), d):
        buf += b"\x00" * (-len(buf) % 4)
        offs.append(len(buf))
        buf += m.tobytes() + b"\x00" * 2
    arena = torch.from_numpy(np.frombuffer(bytes(buf) + b"\x00" * (-len(buf) % 16), dtype=np.uint8).copy()).cuda()
    tested = [FeatCut([FeatTrack(offs[0], row_len - 2)], row_len - 2, COPY, dst_first=2),
              # (the row astride the mark is a full fold: the store that crosses it carries mixed values)
              FeatCut([FeatTrack(offs[1], row_len), FeatTrack(offs[2], 4099, None, True, row_len - 5000, 10.0)], row_len, FOLD, ref_track=0),
              FeatCut([FeatTrack(offs[3], row_len - 7)], row_len - 4, COPY, pad_value=-3.5, dst_first=3)]
    empty = FeatCut([FeatTrack(-1, 0)], 0, COPY)
    cuts = [empty] * rows
    for r, cut in zip(under_test, tested):
        cuts[r] = cut
    guard = 64
    big = torch.empty(rows * row_len + guard, dtype=torch.int32, device="cuda")
    big.fill_(0x5A5A5A5A)
    res, _ = A.featmix_in_arena(arena, cuts, 1, row_frames=row_len, out=big.view(torch.float32)[: rows * row_len])
    torch.cuda.synchronize()
    twin, _ = A.featmix_in_arena(arena, tested, 1, row_frames=row_len)
    torch.cuda.synchronize()
    for k, r in enumerate(under_test):
        assert torch.equal(res[r, :, 0].view(torch.int32), twin[k, :, 0].view(torch.int32)), r
    # every other row is log(1e-10) (bits), counted on the device; nothing behind the end was written
    eps = int(np.float32(R.LOG_EPSILON).view(np.int32))
    other = sum(int((ch != eps).sum()) for ch in big[: rows * row_len].split(CHUNK))
    assert other == int((twin.view(torch.int32) != eps).sum())
    assert bool((big[rows * row_len:] == 0x5A5A5A5A).all())
    print(f"[far] hipfeat_featmix_run: wrote up to element {rows * row_len - 1} (2^31 + {rows * row_len - 1 - 2 ** 31})")
    peak = torch.cuda.max_memory_allocated()
    print(f"[far] peak device memory: {peak / 2 ** 30:.2f} GiB")
    assert peak < 20 << 30, peak
