"""GPU: the feature-mix launches (lhotse_amd/csrc/kernel_featmix.hpp through ``lhotse_amd.augmentation.featmix_in_arena``) against their
numpy statement (tests/_featmix_ref.py): copy-form rows bit for bit, fold-form rows against the float64 truth.

The bound of a fold-form element (no recorded reference error here; the golden groups carry theirs, and there the bar is the issue's
alone): ``2 * spacing(float32(|truth|)) + carried``.  The first term is the issue's: a 1-ulp ``logf`` plus one rounding of the result.
``carried`` (tests/_featmix_ref.py, derived there) bounds what reaches ``log`` from the float32 ``e``, per frame from the number k of
tracks that COVER the frame, not from the tracks of the cut: about ``(4 + k) * 2^-24``, i.e. 4.8e-7 where four of the 256 tracks of
the largest fold overlap.

Shapes: F in {1, 23, 40, 80, 257}; cuts of 1, 2 and 77 frames; B = 1 and B = 5; folds of 1, 2, 5 and 256 tracks; a track that starts
behind every other track's end; a track of 0 frames; binary16 tracks at odd 2-byte offsets; rows longer than a tile (77 x 257 > 4 x 4096)."""
import numpy as np
import pytest
import torch

import _featmix_ref as R
from _featmix_cases import Arena

from lhotse_amd import augmentation as A
from lhotse_amd.augmentation import FEATMIX_COPY as COPY, FEATMIX_FOLD as FOLD, FeatCut, FeatTrack

pytestmark = pytest.mark.gpu
GUARD = 64
POISON = 0x5A5A5A5A
FS = [1, 23, 40, 80, 257]


def run(host: np.ndarray, cuts, F, row_frames=None):
    """featmix_in_arena into a slice of a poisoned tensor -> the (B, T, F) result as numpy; the guards on either side and the arena must
    come back as they were."""
    lay = A.featmix_layout(len(host), cuts, F, row_frames)
    B, T = len(cuts), lay["row_frames"]
    whole = torch.full((GUARD + B * T * F + GUARD,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    d_arena = torch.from_numpy(host).cuda()
    res, lens = A.featmix_in_arena(d_arena, cuts, F, row_frames, out=whole[GUARD: GUARD + B * T * F])
    torch.cuda.synchronize()
    bits = whole.view(torch.int32).cpu().numpy()
    assert (bits[:GUARD] == POISON).all() and (bits[-GUARD:] == POISON).all(), "a guard element was written"
    assert np.array_equal(d_arena.cpu().numpy(), host), "the arena was written"
    assert res.shape == (B, T, F) and lens.tolist() == [c.num_frames for c in cuts]
    return res.cpu().numpy()


def check(host, cuts, F, got, row_frames=None, label=""):
    truth = R.batch(host, cuts, F, row_frames)
    for b, c in enumerate(cuts):
        if c.form == COPY:
            assert np.array_equal(got[b].view(np.uint32), truth[b].astype(np.float32).view(np.uint32)), (label, b)
            continue
        inside = np.zeros(got.shape[1], dtype=bool)
        inside[c.dst_first: c.dst_first + c.num_frames] = True
        assert np.array_equal(got[b][~inside].view(np.uint32), truth[b][~inside].astype(np.float32).view(np.uint32)), (label, b)
        err = np.abs(got[b][inside].astype(np.float64) - truth[b][inside])
        bound = R.bar(truth[b][inside]) + R.carried(c)[:, None]
        worst = int(np.argmax(err - bound))
        print(f"{label} cut {b}: K={len(c.tracks)} max |out - truth| = {err.max():.3e}, bound there {bound.ravel()[np.argmax(err)]:.3e}")
        assert (err <= bound).all(), (label, b, err.ravel()[worst], bound.ravel()[worst])


def mixed_batch(F, seed=0):
    """B = 5: a copy with padding, a 2-track fold with an SNR (noise behind the speech's start, binary16), a 5-track fold with a track
    behind every other track's end, a track of 0 frames and a padding track in front (left padding), a cut of 1 frame, a cut of 2."""
    a = Arena(seed)
    cuts = [
        FeatCut([a.track(70, F)], 77, COPY, pad_value=R.LOG_EPSILON),
        FeatCut([a.track(77, F), a.track(40, F, f16=True, first=11, snr=10.0)], 77, FOLD, ref_track=0),
        FeatCut([FeatTrack(-1, 9, value=R.LOG_EPSILON), a.track(30, F, first=9), a.track(0, F, first=20, snr=5.0), a.track(25, F, f16=True, first=12, snr=15.0),
                 a.track(20, F, first=57, snr=12.5)], 77, FOLD, ref_track=1),
        FeatCut([a.track(1, F, f16=True)], 1, COPY),
        FeatCut([a.track(2, F), a.track(1, F, first=1, snr=0.0)], 2, FOLD, ref_track=0, dst_first=3),
    ]
    return a.host(), cuts


@pytest.mark.parametrize("F", FS)
def test_a_mixed_batch_of_five(F):
    host, cuts = mixed_batch(F)
    got = run(host, cuts, F)
    check(host, cuts, F, got, label=f"F={F}")
    again = run(host, cuts, F)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two runs differ"


@pytest.mark.parametrize("F", [1, 23, 80])
def test_a_cut_does_not_depend_on_the_rest_of_the_batch(F):
    host, cuts = mixed_batch(F)
    full = run(host, cuts, F, row_frames=80)
    for b, c in enumerate(cuts):  # B = 1, the same row length
        alone = run(host, [c], F, row_frames=80)
        assert np.array_equal(alone[0].view(np.uint32), full[b].view(np.uint32)), (F, b)
    rev = run(host, cuts[::-1], F, row_frames=80)
    assert np.array_equal(rev[::-1].view(np.uint32), full.view(np.uint32))


@pytest.mark.parametrize("F", [1, 23, 257])
def test_copy_form_is_a_bit_copy(F):
    a = Arena(3)
    m = a.feats(77, F)
    specials = np.array([0x80000000, 0x7FC00001, 0xFFC12345, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001], dtype=np.uint32).view(np.float32)
    m.reshape(-1)[: min(m.size, 8)] = specials[: min(m.size, 8)]
    m.reshape(-1)[-1] = specials[0]
    cuts = [FeatCut([FeatTrack(a.add(m), 77)], 77, COPY),
            FeatCut([FeatTrack(a.add(m[:30]), 30)], 40, COPY, pad_value=-5.0, dst_first=2),
            FeatCut([FeatTrack(a.add(m[:31]), 30, rows=31)], 30, COPY),  # one stored row too many
            FeatCut([FeatTrack(a.add(m[:29]), 30, rows=29)], 33, COPY, pad_value=-0.0),  # one too few: the last row repeats
            FeatCut([FeatTrack(-1, 7, value=-23.5)], 12, COPY, pad_value=1.25)]
    host = a.host()
    got = run(host, cuts, F)
    check(host, cuts, F, got, label=f"copy F={F}")
    assert np.array_equal(got[0].view(np.uint32), m.view(np.uint32))
    assert np.array_equal(got[3][29].view(np.uint32), m[28].view(np.uint32)) and np.array_equal(got[3][28].view(np.uint32), m[28].view(np.uint32))
    assert (got[3][30:33].view(np.uint32) == 0x80000000).all() and (got[1][:2] == np.float32(R.LOG_EPSILON)).all()


@pytest.mark.parametrize("F", [23, 80])
def test_binary16_tracks_equal_float32_tracks_of_the_widened_values(F):
    a16, a32 = Arena(5), Arena(5)
    shapes = [(77, 0, None), (40, 11, 10.0), (25, 60, 20.0)]
    t16, t32 = [], []
    for n, first, snr in shapes:
        m = a16.feats(n, F, f16=True)
        t16.append(FeatTrack(a16.add(m, f16=True), n, None, True, first, snr))
        t32.append(FeatTrack(a32.add(m), n, None, False, first, snr))
    for form, tr in ((FOLD, slice(None)), (COPY, slice(0, 1))):
        c16, c32 = FeatCut(t16[tr], 85, form, ref_track=0), FeatCut(t32[tr], 85, form, ref_track=0)
        assert all(t.offset % 4 == 2 for t in t16)  # odd 2-byte offsets
        g16, g32 = run(a16.host(), [c16], F), run(a32.host(), [c32], F)
        assert np.array_equal(g16.view(np.uint32), g32.view(np.uint32)), (F, form)


@pytest.mark.parametrize("K", [1, 2, 5, 256])
def test_folds_of_k_tracks(K):
    F, a = 40, Arena(K)
    if K == 256:  # 3-frame constant tracks, one frame apart, behind a stored first track
        tracks = [a.track(20, F)] + [FeatTrack(-1, 3, first=i, snr=10.0 + (i % 7), value=-3.0 - 0.01 * i) for i in range(1, K)]
        T = K + 2
    else:
        tracks = [a.track(30, F)] + [a.track(10 + i, F, f16=bool(i % 2), first=7 * i, snr=5.0 * i) for i in range(1, K)]
        T = max(t.first + t.frames for t in tracks)
    cuts = [FeatCut(tracks, T, FOLD, ref_track=0)]
    host = a.host()
    got = run(host, cuts, F)
    check(host, cuts, F, got, label=f"K={K}")
    if K == 256:  # frames 20 ... behind the first track's end were floored before the first constant track that covers them arrived
        assert np.isfinite(got).all()


def test_off_by_one_mixes_and_a_reference_that_is_not_the_first_track():
    F, a = 23, Arena(9)
    tr = lambda: [a.track(20, F, snr=3.0), a.track(31, F, f16=True, first=4)]  # noqa: E731  (the first track carries the SNR: the reference is track 1)
    cuts = [FeatCut(tr(), 35, FOLD, ref_track=1), FeatCut(tr(), 34, FOLD, ref_track=1),  # N = 35: as long, one frame dropped,
            FeatCut(tr(), 36, FOLD, ref_track=1, dst_first=1),  # the last frame repeated
            FeatCut([a.track(12, F, rows=11), a.track(12, F, rows=13, first=2, snr=7.0)], 14, FOLD, ref_track=0)]  # the fix-up per track
    host = a.host()
    got = run(host, cuts, F)
    check(host, cuts, F, got, label="off by one")
    assert np.array_equal(got[2][36].view(np.uint32), got[2][35].view(np.uint32))  # the repeated frame


def test_zero_energy_guards():
    F, a = 23, Arena(11)
    silent = lambda n: FeatTrack(a.add(np.full((n, F), -1000.0, dtype=np.float32)), n)  # noqa: E731
    ref_silent = [silent(20), a.track(20, F, first=3, snr=10.0)]  # E_ref == 0: gain 1
    noise_silent = [a.track(20, F), silent(12)._replace(first=5, snr=10.0)]  # S(x_t) == 0: gain 1
    both = [silent(8), silent(8)._replace(snr=0.0)]  # nothing but floors: log(1e-10)
    cuts = [FeatCut(ref_silent, 23, FOLD, ref_track=0), FeatCut(noise_silent, 20, FOLD, ref_track=0), FeatCut(both, 8, FOLD, ref_track=0)]
    host = a.host()
    got = run(host, cuts, F)
    check(host, cuts, F, got, label="zero energy")
    assert np.isfinite(got).all() and np.allclose(got[2][:8], np.log(1e-10), rtol=0, atol=4e-6)


def test_a_tail_two_paddings_cover_holds_log_2e_10():
    F, a = 40, Arena(13)
    pad = lambda n, first=0: FeatTrack(-1, n, first=first, value=R.LOG_EPSILON)  # noqa: E731
    cuts = [FeatCut([pad(5), a.track(30, F, first=5), pad(7, 35)], 42, FOLD, ref_track=1)]  # padded on both sides
    host = a.host()
    got = run(host, cuts, F)
    check(host, cuts, F, got, label="both")
    # the tail was floored to 1e-10 before its padding arrived; the head's padding came first and the floors left it alone
    assert np.allclose(got[0][35:], np.log(2e-10), rtol=0, atol=4e-6) and np.allclose(got[0][:5], np.log(1e-10), rtol=0, atol=4e-6)


def test_a_17th_plan_is_refused_by_the_handle_and_the_16_still_run():
    """``hipfeat_featmix_plan``'s own ticket path on a device handle: 16 plans without a run, a 17th refused (and nothing planned by it),
    every one of the 16 still gives its result, in any order, and the next plan takes ticket 16."""
    from lhotse_amd import _lib

    F, a = 23, Arena(17)
    cuts = [FeatCut([a.track(9, F), a.track(5, F, f16=True, first=3, snr=8.0)], 9, FOLD, ref_track=0), FeatCut([a.track(4, F)], 6, COPY, pad_value=-2.0)]
    host = a.host()
    want = run(host, cuts, F)
    fm = A.HipFeatureMixer("cuda")  # a private one: the plans below stay outstanding on purpose
    try:
        d_arena = torch.from_numpy(host).cuda()
        lay = A.featmix_layout(len(host), cuts, F)
        tickets = [fm.plan(lay)[0] for _ in range(16)]
        assert tickets == list(range(16))
        for _ in range(2):
            with pytest.raises(_lib.HipFeatError, match="16 planned feature mixes are outstanding: run ticket 0 first"):
                fm.plan(lay)
        for t in tickets[::-1]:
            out = torch.empty((2, 9, F), dtype=torch.float32, device="cuda")
            fm.run(t, d_arena, out)
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), t
        with pytest.raises(_lib.HipFeatError, match="not a planned feature mix"):
            fm.run(3, d_arena, out)  # a ticket runs once
        assert fm.plan(lay)[0] == 16
        fm.run(16, d_arena, out)
        torch.cuda.synchronize()
    finally:
        fm.close()
