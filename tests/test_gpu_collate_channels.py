"""GPU: the sources form of the collate launch (``collate_mean_kernel``, lhotse_amd/csrc/kernel_collate.hpp) against its numpy statement
(tests/_multichannel_ref.py), bit for bit, for float32, binary16 and bfloat16 output -- and ``FusedAudioBatch.audio_of_channels`` on the
inputs of tests/golden/multichannel.npz against what the reference's live ``collate_audio`` returned for them.

Shapes: source counts 0, 1, 2, 3, 7, 8 and 32 mixed within one launch; row lengths 0, 1, 3, 4, 5 and the ``kCoTile`` edges 4095, 4096, 4097;
``row_len`` with every residue mod 8 (every alignment of a row's first byte for the 4- and the 2-byte types); the two sources of a row at
every combination of residues mod 4, seven sources at differing residues; right padding, left padding and a destination in between; rows
without sources between sample rows.  ``out`` is pre-filled with a sentinel (every element is written, nothing behind the end is), the
arena is compared before and after (it is only read).

Bits: a NaN compares equal to a NaN (IEEE leaves the sign and payload of an invalid operation's NaN to the implementation: Inf - Inf is
0x7fc00000 on the device and 0xffc00000 on x86); every other value compares by its bits."""
import math

import numpy as np
import pytest
import torch

import _multichannel_golden as MG
from _collate_ref import bits_of
from _multichannel_ref import collate_sources_ref, downmix_ref, ulp32

from lhotse_amd import augmentation as A
from lhotse_amd.input_strategies import FusedAudioBatch

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
KS = [0, 1, 2, 3, 7, 8, 32]
LENS = [0, 1, 3, 4, 5, 4095, 4096, 4097]
T = A.COLLATE_TILE
SENTINEL = {torch.float32: 0x5A5A5A5A, torch.float16: 0x5A5A, torch.bfloat16: 0x5A5A}
GUARD = 64


def same_bits(got: torch.Tensor, want: torch.Tensor) -> bool:
    g, w = bits_of(got), bits_of(want)
    both_nan = torch.isnan(got.detach().cpu().float()).numpy() & torch.isnan(want.float()).numpy()
    return got.shape == want.shape and bool(((g == w) | both_nan).all())


def launch(arena, first, src, lens, row_len, dst, dtype):
    """One launch into a sentinel-filled ``out`` with a guard behind it -> the (rows, row_len) result; asserts the guard is intact."""
    rows = len(lens)
    ints = torch.int32 if dtype == torch.float32 else torch.int16
    big = torch.full((rows * row_len + GUARD,), SENTINEL[dtype], dtype=ints, device="cuda")
    res, sl = A.collate_sources_in_arena(arena, first, src, lens, row_len=row_len, dst_offsets=dst, dtype=dtype, out=big.view(dtype)[: rows * row_len])
    torch.cuda.synchronize()
    assert res.data_ptr() == big.data_ptr() and tuple(res.shape) == (rows, row_len) and sl.tolist() == list(lens)
    assert bool((big[rows * row_len :] == SENTINEL[dtype]).all())  # nothing behind the end was written
    return res


@pytest.fixture(scope="module")
def arena():
    rs = np.random.RandomState(77)
    pcm = rs.randint(-32768, 32768, size=200_000).astype(np.float32) / np.float32(32768.0)
    wild = (rs.randn(100_000) * 10.0 ** rs.uniform(-30, 30, size=100_000)).astype(np.float32)  # every binade the 2-byte types round in
    host = np.concatenate([pcm, wild]).astype(np.float32)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    host[1000:1016] = [inf, -inf, nan, -0.0, 0.0, 1.0, -1.0, inf, 65504.0, 65520.0, 1e-8, -1e-8, 3.4e38, 3.4e38, -0.0, nan]
    host[2003:2019] = [inf, inf, 1.0, -0.0, -0.0, nan, 1.0, -inf, 65504.0, 65520.0, 5.9e-8, 1e-8, 3.4e38, -3.4e38, 0.0, nan]
    host[3001:3017] = [1.0, 2.0, 3.0, -0.0, 4.0, 5.0, -2.0, 6.0, -65504.0, 0.0, 1e-41, 2e-45, 3.4e38, 1.0, -0.0, 7.0]
    return host, torch.from_numpy(host).cuda()


@pytest.fixture(scope="module")
def mixed_rows():
    """One row per (source count, length), sources at scattered residues, three kinds of destination."""
    rs = np.random.RandomState(5)
    first, src, lens, kinds = [0], [], [], []
    for i, (k, n) in enumerate((k, n) for n in LENS for k in KS):
        src += [int(4 * rs.randint(0, 70_000) + (c + i) % 4) for c in range(k)]
        first.append(len(src)), lens.append(n), kinds.append(i % 3)
    order = rs.permutation(len(lens))  # (counts and lengths in no particular order within the launch)
    return first, src, lens, kinds, order


def _dst(lens, kinds, row_len):
    return [0 if kind == 0 else row_len - n if kind == 1 else (row_len - n) // 2 for n, kind in zip(lens, kinds)]


def _reorder(first, src, lens, dst, order):
    f, s = [0], []
    for r in order:
        s += src[first[r] : first[r + 1]]
        f.append(len(s))
    return f, s, [lens[r] for r in order], [dst[r] for r in order]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_source_counts_lengths_and_row_alignments_in_one_launch(arena, mixed_rows, dtype):
    host, dev = arena
    first, src, lens, kinds, order = mixed_rows
    before = dev.clone()
    for residue in range(8):
        row_len = 4097 + 7 + residue  # every residue mod 8, and room to pad the longest row on either side
        assert row_len % 8 == residue
        dst = _dst(lens, kinds, row_len)
        f, s, l, d = _reorder(first, src, lens, dst, order)
        got = launch(dev, f, s, l, row_len, d, dtype)
        want = collate_sources_ref(host, f, s, l, row_len, d, dtype)
        assert same_bits(got, want), (dtype, residue)
        if residue in (0, 5):
            again = launch(dev, f, s, l, row_len, d, dtype)  # a second run: the same bits
            assert torch.equal(again.view(torch.int16 if dtype != torch.float32 else torch.int32), got.view(torch.int16 if dtype != torch.float32 else torch.int32))
            plain = launch(dev, first, src, lens, row_len, dst, dtype)  # the other ordering of the rows: the same rows
            ints = torch.int16 if dtype != torch.float32 else torch.int32
            assert torch.equal(plain[torch.as_tensor(order).cuda()].view(ints), got.view(ints))
    assert torch.equal(dev.view(torch.int32), before.view(torch.int32))  # the arena is only read


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_channels_at_every_combination_of_residues(arena, dtype):
    host, dev = arena
    n = T + 3
    first, src, lens = [0], [], []
    for a in range(4):  # k = 2: every pair of residues mod 4
        for b in range(4):
            src += [4 * (100 + 7 * a) + a, 4 * (30_000 + 11 * b) + b]
            first.append(len(src)), lens.append(n)
    src += [4 * (1000 * c + 50) + r for c, r in enumerate([0, 1, 2, 3, 1, 3, 2])]  # k = 7: differing residues
    first.append(len(src)), lens.append(n)
    first.append(len(src)), lens.append(n)  # a row without sources between sample rows
    src += [4 * 40_000 + 3, 4 * 40_000 + 3 + n]  # k = 2 again, behind it
    first.append(len(src)), lens.append(n)
    for row_len in (n, n + 2):
        dst = [(row_len - n) * (r % 2) for r in range(len(lens))]
        got = launch(dev, first, src, lens, row_len, dst, dtype)
        assert same_bits(got, collate_sources_ref(host, first, src, lens, row_len, dst, dtype)), (dtype, row_len)
        assert not bits_of(got[-2]).any()  # the row without sources is +0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_nan_inf_and_signed_zero_propagate(arena, dtype):
    host, dev = arena
    first, src, lens = [0, 2, 5, 6, 6], [1000, 2003, 1000, 2003, 3001, 1000], [16, 16, 16, 16]
    got = launch(dev, first, src, lens, 19, [0, 3, 1, 0], dtype)
    want = collate_sources_ref(host, first, src, lens, 19, [0, 3, 1, 0], dtype)
    assert same_bits(got, want)
    f = got.float().cpu().numpy()
    assert np.isnan(f[0, 2]) and np.isnan(f[0, 1]) and np.isposinf(f[0, 0]) and np.isnan(f[0, 7])  # NaN; Inf - Inf; Inf + Inf; Inf - Inf
    assert bits_of(got[0, 3:5].cpu()).tolist() == [0, 0]  # (-0 + -0) / 2 and (0 + -0) / 2 from a sum that starts at +0.0
    assert np.isnan(f[1, 3 + 15]) and np.isnan(f[1, 3 + 5])
    if dtype == torch.float32:
        assert np.array_equal(bits_of(got[2, 1:17].cpu()), host[1000:1016].view(np.uint32))  # one source: the bits, NaN payloads and -0 included
        assert f[0, 12] == np.float32(3.4e38) and f[0, 13] == 0.0  # no float32 overflow inside the sum


def test_no_rows_and_rows_of_no_elements(arena):
    host, dev = arena
    res, lens = A.collate_sources_in_arena(dev, [0], [], [], row_len=5)
    assert tuple(res.shape) == (0, 5) and len(lens) == 0
    res, _ = A.collate_sources_in_arena(dev, [0, 2, 2], [0, 8], [0, 0])
    assert tuple(res.shape) == (2, 0)
    res, _ = A.collate_sources_in_arena(dev, [0, 0, 0], [], [3, 0], row_len=4)  # nothing but rows without sources: zeros, no arena needed
    assert not bits_of(res).any()
    with pytest.raises(ValueError):
        A.collate_sources_in_arena(dev, [0, 33], [0] * 33, [4])
    with pytest.raises(ValueError):
        A.collate_sources_in_arena(dev, [0, 1], [dev.numel() - 3], [4])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_rows_of_one_source_equal_collate_in_arena(arena, dtype):
    host, dev = arena
    offs = [3, 4101, 9002, 1000, 300_000 - 4097, 77]
    lens = [4096, 4097, 1, 16, 4097, 0]
    row_len = 4100
    dst = A.left_pad_offsets(lens, row_len)
    want, _ = A.collate_in_arena(dev, offs, lens, row_len=row_len, dst_offsets=dst, dtype=dtype)
    got = launch(dev, np.arange(len(offs) + 1), offs, lens, row_len, dst, dtype)
    ints = torch.int16 if dtype != torch.float32 else torch.int32
    assert torch.equal(got.view(ints), want.view(ints))


# ---- FusedAudioBatch.audio_of_channels on the golden inputs -----------------------------------------------------------------------
SR = MG.SR


@pytest.fixture(scope="module")
def golden():
    g = MG.load()
    g["rows"] = [[np.ascontiguousarray(ch) for ch in (pcm.astype(np.float32) / np.float32(32768.0))] for pcm in g["inputs"]]  # what the stdlib backend reads
    return g


def _call(batch, rows, ids, mode):
    cuts = [rows[i] for i in ids]
    wants = [len(c[0]) for c in cuts]
    return batch.audio_of_channels(cuts, [1.0] * len(cuts), [None] * len(cuts), wants, SR, mode)


def test_the_channel_form_is_the_goldens(golden):
    batch = FusedAudioBatch("cuda:0")
    for c, ids in MG.FALSE_BATCHES.items():
        audio, lens = _call(batch, golden["rows"], ids, False)
        assert audio.is_cuda and audio.dtype == torch.float32 and lens.tolist() == [MG.SHAPES[i][1] for i in ids]
        assert np.array_equal(audio.cpu().numpy(), golden[f"false/{c}"]), c
    audio, _ = _call(batch, golden["rows"], MG.NONE_MULTI, None)  # every cut has more than one channel: (B, C, T)
    assert np.array_equal(audio.cpu().numpy(), golden["none_multi"])
    # cuts of 2, 3, 1 and 8 channels in one batch: zero rows for the channels a cut does not have, a mono cut in channel 0
    audio, lens = _call(batch, golden["rows"], range(5), False)
    assert tuple(audio.shape) == (5, 8, 2100)
    a = audio.cpu().numpy()
    for i, (c, n) in enumerate(MG.SHAPES):
        assert np.array_equal(a[i, :c, :n], np.stack(golden["rows"][i])) and not a[i, c:].view(np.uint32).any() and not a[i, :, n:].view(np.uint32).any()
    half, _ = FusedAudioBatch("cuda:0", torch.bfloat16).audio_of_channels([golden["rows"][i] for i in range(5)], [1.0] * 5, [None] * 5,
                                                                        [n for _, n in MG.SHAPES], SR, False)
    assert torch.equal(half.cpu().view(torch.int16), audio.cpu().to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("mode", [True, None])
def test_the_downmix_is_the_goldens_or_closer_to_the_truth(golden, mode):
    audio, lens = _call(FusedAudioBatch("cuda:0"), golden["rows"], range(5), mode)
    assert tuple(audio.shape) == (5, 2100) and lens.tolist() == golden["lens"].tolist() and lens.dtype == torch.int64
    a, want = audio.cpu().numpy(), golden["true" if mode else "none"]
    for i, (c, n) in enumerate(MG.SHAPES):
        assert not a[i, n:].view(np.uint32).any()
        if c <= 2:
            assert np.array_equal(a[i], want[i]), i
            continue
        x = np.stack(golden["rows"][i])
        t = np.array([math.fsum(float(v) for v in x[:, j]) / c for j in range(n)])  # (PCM samples: the float64 sum is exact)
        err = np.abs(a[i, :n].astype(np.float64) - t)
        print(f"cut {i} C={c}: max |y - t| / ulp32(t) = {float((err / ulp32(t)).max()):.6f}; the golden's: {float((np.abs(want[i, :n] - t) / ulp32(t)).max()):.6f}")
        assert (err <= 0.5 * ulp32(t) * (1.0 + 2.0 ** -20)).all(), i


def test_a_pending_chain_runs_per_channel_as_the_mono_chain_does(golden):
    """A speed factor and a source rate on a 3-channel cut: every channel equals the same row sent through ``audio_of_tracks`` as a mono
    cut, bit for bit -- and the downmix of the cut is the mean of those rows."""
    rows = [np.ascontiguousarray(r[:1600]) for r in golden["rows"][1]]
    batch = FusedAudioBatch("cuda:0")
    for factor, rate in ((1.1, None), (1.0, 22050), (0.9, 22050)):
        n = len(rows[0])
        if rate is not None:
            n = int(A.resample_layout(np.zeros(1, dtype=np.int64), np.array([n]), [(rate, SR)], 0)[1][0])
        want = int(A.perturbed_layout(np.zeros(1, dtype=np.int64), np.array([n]), [factor], SR, 0)[1][0])
        mono, mono_lens = batch.audio_of_tracks([[(r, factor, 0, None, True, want, None, rate)] for r in rows], [want] * 3, SR)
        plain = golden["rows"][0]  # a 2-channel cut with nothing pending in the same batch
        audio, lens = batch.audio_of_channels([rows, plain], [factor, 1.0], [rate, None], [want, len(plain[0])], SR, False)
        assert lens.tolist() == [want, len(plain[0])] and mono_lens.tolist() == [want] * 3
        assert torch.equal(audio[0, :, :want].view(torch.int32), mono.view(torch.int32)), (factor, rate)
        assert not bool(audio[0, :, want:].view(torch.int32).any()) and not bool(audio[1, 2].view(torch.int32).any())
        assert np.array_equal(audio[1, :2].cpu().numpy(), np.stack(plain))
        down, _ = batch.audio_of_channels([rows, plain], [factor, 1.0], [rate, None], [want, len(plain[0])], SR, True)
        ref = collate_sources_ref(mono.cpu().reshape(-1), [0, 3], [0, want, 2 * want], [want])
        assert same_bits(down[0, :want].cpu().reshape(1, -1), ref), (factor, rate)


def test_a_padded_cut_and_a_mono_track_list_share_the_launch(golden):
    """``offsets`` / ``totals`` (a cut padded with silence on either side) and an entry that is the track list of a mono cut."""
    batch = FusedAudioBatch("cuda:0")
    c3, c2 = golden["rows"][1], golden["rows"][0]
    mono = golden["rows"][2][0]
    tracks = [(mono, 1.0, 0, None, True), (300, 1.0, len(mono), None, False, 300)]  # a mono cut padded to the right by the device mix
    wants = [len(c3[0]), len(c2[0]), len(mono) + 300]
    audio, lens = batch.audio_of_channels([c3, c2, tracks], [1.0] * 3, [None] * 3, wants, SR, True, offsets=[480, None, None], totals=[len(c3[0]) + 500, None, None])
    assert lens.tolist() == [len(c3[0]) + 500, len(c2[0]), len(mono) + 300] and tuple(audio.shape) == (3, 2200)
    a = audio.cpu().numpy()
    assert np.array_equal(a[0, 480 : 480 + 1700].view(np.uint32), downmix_ref(c3).view(np.uint32))
    assert not a[0, :480].view(np.uint32).any() and not a[0, 2180:].view(np.uint32).any()
    assert np.array_equal(a[1, :2100], golden["true"][0]) and np.array_equal(a[2, :1900], mono) and not a[2, 1900:].view(np.uint32).any()
