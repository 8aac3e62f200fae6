"""GPU: the reverberation by partitioned FFT convolution (hipfeat_reverb_plan_method with method fft / auto, kernel_reverb_fft.hpp;
``reverb_in_arena(method=...)``, ``HipReverbWithImpulseResponse(method=...)``, ``reverb_method=`` of the two input strategies).

Bars: those of tests/test_gpu_reverb.py (tests/_reverb_ref.py::bars) -- the device and the reference's arithmetic (``fft32``) are both
judged against the exact float64 convolution; rel-L2 <= 2 x the reference's own + 2^-24, max abs <= 2 x the reference's own + 2^-24 x peak.
An FFT route has no summation-order-free integers, so where test_gpu_reverb.py compares with ``integer_expected`` this file compares with
the bars, and ``array_equal`` only device against device.

Worst rel-L2 / bar and max-abs / bar measured on an MI355X: see the print of test_grid_meets_both_audio_bars_against_float64 and
DESIGN 4.19."""
import numpy as np
import pytest
import torch

import _reverb_ref as R

from lhotse_amd import _lib
from lhotse_amd.augmentation import (HipReverb, HipReverbWithImpulseResponse, get_or_create_reverb, reverb_fft_tail_floats, reverb_in_arena, reverb_tail_floats,
                                     scaled_rir)

pytestmark = pytest.mark.gpu

BLOCK = 1024             # kRfBlock, lhotse_amd/csrc/reverb_fft_tables.hpp: new samples per transform
SPEC = 2048              # kRfSpecFloats: floats of one spectrum
WAVES = 4                # kRfWaves: work items of launches A and B per workgroup trip
GRID_SLOTS = 1792        # kRfGridSlots: workgroups of launches A and B at the most
INLINE_BYTES = 3328      # kMbInlineBytes, kernel_minibatch.hpp: a table up to this size travels in the kernel arguments
LDS_TABLE_BYTES = 24576  # kMbLdsTableBytes: a staged table up to this size is copied to LDS, a larger one searched in HBM
ITEM_BYTES, RIR_BYTES = 80, 32  # sizeof(RfItem), sizeof(RfRir)
LS = (1, 1023, 1024, 1025, 2047, 2048, 2049, 3001)
NS = (1, 1023, 1024, 1025, 2049, 5000)


def _signal(rng, n):
    """Gated noise: bursts of different levels with silence between them (as tests/test_gpu_reverb.py)."""
    x = rng.standard_normal(n).astype(np.float32) * np.float32(0.1)
    gate = np.repeat(rng.choice([0.0, 0.3, 1.0], size=n // 500 + 1), 500)[:n].astype(np.float32)
    return x * gate if n > 1 else x


def _rir(rng, taps, peak_at):
    """Decaying noise with a dominant peak, as int16 samples in float32."""
    h = rng.standard_normal(taps) * np.exp(-6.0 * np.arange(taps) / max(taps, 2)) * 0.2
    h[peak_at] = 1.0
    return (np.round(h * 20000.0) / 32768.0).astype(np.float32)


def _shifts(taps):
    """0, L - 1, 1023 and 1024 where L allows, and one mid value: the first one from L / 2 on that is 1 mod 4, so that with the others the
    outputs of a block start at all four 4-byte alignments mod 16 (a block's first output sits at 1024 j - shift)."""
    mid = taps // 2 + (1 - taps // 2) % 4
    return sorted({s for s in (0, taps - 1, 1023, 1024, mid) if 0 <= s < taps})


def _item(rng, n, taps, shift, norm, x=None):
    hs, found = scaled_rir(_rir(rng, taps, shift))
    assert found == shift
    return (_signal(rng, n) if x is None else x, hs, shift, norm)


def _grid():
    rng = np.random.default_rng(20241021)
    items = []
    for n in NS:
        for taps in LS:
            x = _signal(rng, n)
            for shift in _shifts(taps):
                it = _item(rng, n, taps, shift, False, x)
                items += [it, it[:3] + (True,)]
    return items


def _run(items, method="fft", min_fft_taps=None, share=False, fill=float("nan"), info=None):
    """items: [(x, hs, shift, normalize)] -> the outputs (numpy) through reverb_in_arena alone.  ``share``: items whose ``hs`` is the same
    object share one copy of it in the arena.  Sources and RIRs must come back unchanged, and nothing may be written outside the outputs
    and the spectra workspace the plan reports."""
    chunks, so, ro, pos, placed = [], [], [], 0, {}
    for x, hs, _, _ in items:
        so.append(pos), chunks.append(x)
        pos += len(x)
        if share and id(hs) in placed:
            ro.append(placed[id(hs)])
            continue
        placed[id(hs)] = pos
        ro.append(pos), chunks.append(hs)
        pos += len(hs)
    front = np.concatenate(chunks)
    lens, taps, shifts = [len(x) for x, _, _, _ in items], [len(h) for _, h, _, _ in items], [s for _, _, s, _ in items]
    guard = 64
    arena = torch.full((((pos + 3) & ~3) + reverb_fft_tail_floats(lens, taps, shifts, ro) + guard,), fill, dtype=torch.float32, device="cuda:0")
    arena[:pos] = torch.from_numpy(front)
    rv = get_or_create_reverb(arena.device)
    ticket, offs, block = rv.plan(so, lens, ro, taps, shifts, [int(f) for _, _, _, f in items], pos, method, min_fft_taps)
    assert int(block[1]) <= arena.numel() - guard
    if info is not None:
        info.append(block.copy())
    rv.run(ticket, arena)
    host = arena.cpu().numpy()
    assert np.array_equal(host[:pos], front)  # sources and impulse responses are untouched
    used = np.zeros(len(host), dtype=bool)
    used[:pos] = True
    for o, n in zip(offs.tolist(), lens):
        assert o % 4 == 0 and o >= pos and not used[o : o + n].any()
        used[o : o + n] = True
    end_out = max(o + ((n + 3) & ~3) for o, n in zip(offs.tolist(), lens))
    if len(block) == 8:  # the workspace: from the first 16-byte boundary behind the outputs to the plan's arena floats
        assert (int(block[1]) - end_out) == SPEC * int(block[4]) and not used[end_out : int(block[1])].any()
        assert np.isfinite(host[end_out : int(block[1])]).all()  # every spectrum that may be read has been written
        used[end_out : int(block[1])] = True
    if np.isnan(fill):
        assert np.isnan(host[~used]).all()  # nothing else was written
    return [host[o : o + n].copy() for o, n in zip(offs.tolist(), lens)]


def _ratios(item, y):
    """-> (rel-L2 / its bar, max abs / its bar) of one output against the float64 truth."""
    x, hs, shift, norm = item
    truth = R.exact(x, hs, shift, norm)
    ref_rel, ref_max = R.distances(R.fft32(x, hs, shift, norm), truth)
    rel, mx = R.distances(y, truth)
    bar_rel, bar_max = R.bars(ref_rel, ref_max, truth)
    assert np.isfinite(y).all()
    # (an all-zero item -- a gated-off stretch of the signal -- has a max-abs bar of 0 when the reference returns zeros too: 0 meets it)
    return tuple(0.0 if v == 0.0 else v / bar if bar > 0.0 else float("inf") for v, bar in ((rel, bar_rel), (mx, bar_max)))


def _assert_bars(items, got, what):
    worst = (0.0, 0.0)
    for k, (item, y) in enumerate(zip(items, got)):
        r = _ratios(item, y)
        assert r[0] <= 1.0 and r[1] <= 1.0, (what, k, len(item[0]), len(item[1]), item[2], item[3], r)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print(f"{what}: worst rel-L2 / bar {worst[0]:.3f}, worst max-abs / bar {worst[1]:.3f} over {len(items)} items")
    return worst


@pytest.fixture(scope="module")
def grid():
    items = _grid()
    return items, _run(items)


def test_grid_meets_both_audio_bars_against_float64(grid):
    """Measured on an MI355X: the worst of the 372 items is at 0.369 x the rel-L2 bar and 0.419 x the max-abs bar.  The N = 1 items are
    the hard ones: the output is ONE sample, h[shift] x[0], the reference's FFT of a single sample returns it almost exactly, so the bar
    is 2^-24 relative -- half an ulp.  With all three transforms in float32 the item (N, L, shift) = (1, 1023, 0) was one ulp off, 1.177 x
    both bars (and the N >= 1023 items at <= 0.60 / 0.72); the RIR spectra and the inverse transform therefore run in float64
    (kernel_reverb_fft.hpp, PRECISION)."""
    items, got = grid
    assert {s % 4 for _, _, s, _ in items} == {0, 1, 2, 3}  # a block's first output at every 4-byte alignment mod 16
    assert any(len(h) > len(x) for x, h, _, _ in items)     # L > N
    assert len(items) * ITEM_BYTES > LDS_TABLE_BYTES        # (this ticket's table is searched in HBM)
    over, worst, worst_long = [], [0.0, 0.0], [0.0, 0.0]
    for (x, hs, shift, norm), y in zip(items, got):
        r = _ratios((x, hs, shift, norm), y)
        print(f"N {len(x)} L {len(hs)} shift {shift} norm {int(norm)}: rel / bar {r[0]:.3f}  max / bar {r[1]:.3f}")
        for w in (worst,) + ((worst_long,) if len(x) > 1 else ()):
            w[0], w[1] = max(w[0], r[0]), max(w[1], r[1])
        if max(r) > 1.0:
            over.append((len(x), len(hs), shift, norm, round(r[0], 3), round(r[1], 3)))
    print(f"grid: worst rel-L2 / bar {worst[0]:.3f}, worst max-abs / bar {worst[1]:.3f} over {len(items)} items; "
          f"N > 1 alone: {worst_long[0]:.3f}, {worst_long[1]:.3f}; over a bar: {over}")
    assert not over, over


def test_zero_input_gives_exact_zeros_and_the_gain_is_skipped():
    rng = np.random.default_rng(5)
    it = _item(rng, 3000, 1500, 10, True)
    z, y = _run([(np.zeros(3000, np.float32), it[1], 10, True), it])
    assert np.array_equal(z, np.zeros(3000, np.float32)) and not np.isnan(z).any()
    _assert_bars([it], [y], "beside a zero item")


def test_runs_repeat_and_items_do_not_depend_on_their_neighbours(grid):
    items, got = grid
    k = next(k for k, it in enumerate(items) if len(it[0]) == 5000 and len(it[1]) == 3001 and it[2] == 1501 and it[3])
    alone = _run([items[k]])[0]
    again = _run([items[k]])[0]
    assert np.array_equal(alone, again)
    among = _run([items[1], items[30], items[50], items[k], items[60], items[8], items[70], items[127]])[3]
    assert np.array_equal(alone, among)
    assert np.array_equal(alone, got[k])  # ... nor on the route of the table: kernel arguments here, HBM in the grid's ticket


def test_items_sharing_an_impulse_response_equal_private_copies():
    rng = np.random.default_rng(6)
    a, b = _item(rng, 5000, 2049, 700, True), _item(rng, 1500, 300, 0, False)
    items = [a, (_signal(rng, 2049), a[1], a[2], False), b, (_signal(rng, 100), a[1], a[2], True), (_signal(rng, 7), b[1], b[2], True)]
    shared_info, private_info = [], []
    shared = _run(items, share=True, info=shared_info)
    private = _run(items, share=False, info=private_info)
    assert int(shared_info[0][7]) == 2 and int(private_info[0][7]) == 5  # distinct RIR spectra: 3 + 1 partitions against 3 + 3 + 1 + 3 + 1
    assert int(private_info[0][4]) - int(shared_info[0][4]) == 3 + 3 + 1
    for s, p in zip(shared, private):
        assert np.array_equal(s, p)
    _assert_bars(items, shared, "shared RIR")


def test_auto_ticket_holds_both_routes_and_each_item_equals_its_own_route():
    rng = np.random.default_rng(7)
    items = [_item(rng, 5000, 800, 400, True), _item(rng, 2049, 1024, 1023, True), _item(rng, 3000, 1023, 0, False), _item(rng, 1025, 2049, 2048, False)]
    info = []
    got = _run(items, method="auto", min_fft_taps=1024, info=info)
    direct = _run([items[0], items[2]], method="direct")
    fft = _run([items[1], items[3]], method="fft")
    assert int(info[0][2]) == 3 + 2 and int(info[0][7]) == 2  # direct-form work items (2048 outputs each) of items 0 and 2; two RIR spectra sets
    assert np.array_equal(got[0], direct[0]) and np.array_equal(got[2], direct[1])
    assert np.array_equal(got[1], fft[0]) and np.array_equal(got[3], fft[1])
    # all under the threshold: the direct form's ticket; all above: the FFT's
    assert np.array_equal(_run([items[0]], method="auto", min_fft_taps=801)[0], direct[0])
    assert np.array_equal(_run([items[1]], method="auto", min_fft_taps=0)[0], fft[0])


def test_workgroups_that_take_a_second_trip():
    """kRfWaves x kRfGridSlots = 4 x 1792 = 7168 transforms are one trip of a full grid: 7169 output blocks (and the 7169 input blocks of
    launch A; the one RIR partition is the launch in front of it) are 1793 workgroup trips, one more than the cap, so the launches take 897
    workgroups of two trips each -- the wave buffers are re-used and the work item is no longer 4 blockIdx.x + wave."""
    rng = np.random.default_rng(8)
    hs, shift = scaled_rir(_rir(rng, 5, 0))
    lens = [BLOCK * BLOCK] * 7 + [1]
    items = [(_signal(rng, n), hs, shift, bool(k % 2)) for k, n in enumerate(lens)]
    info = []
    got = _run(items, share=True, info=info)
    a_work, b_work = int(info[0][4]), int(info[0][5])
    assert b_work == WAVES * GRID_SLOTS + 1 and a_work == b_work + 1
    pick = [0, 6, 7]  # the first item, the last long one (all its blocks on second trips) and the one-sample item behind it
    _assert_bars([items[k] for k in pick], [got[k] for k in pick], "second trip")
    for k in (1, 7):
        assert np.array_equal(_run([items[k]])[0], got[k]), k


@pytest.mark.parametrize("count", [41, 42, 306, 307])
def test_table_routes_at_their_boundaries(count):
    """Items sharing ONE impulse response: the table is 80 count + 32 bytes.  41 | 42: the last that fits the kernel arguments and the first
    that is staged; 306 | 307: the last that is searched in LDS and the first that is searched in HBM."""
    bytes_ = count * ITEM_BYTES + RIR_BYTES
    want = {41: "kernel arguments", 42: "LDS copy", 306: "LDS copy", 307: "HBM"}[count]
    assert ("kernel arguments" if bytes_ <= INLINE_BYTES else "LDS copy" if bytes_ <= LDS_TABLE_BYTES else "HBM") == want
    rng = np.random.default_rng(count)
    hs, shift = scaled_rir(_rir(rng, 40, 7))
    items = [(_signal(rng, int(n)), hs, shift, bool(f)) for n, f in zip(rng.integers(1, 1500, size=count), rng.integers(0, 2, size=count))]
    info = []
    got = _run(items, share=True, info=info)
    assert int(info[0][7]) == 1
    _assert_bars(items, got, f"{count} items ({want})")
    for k in (0, count // 2, count - 1):
        assert np.array_equal(_run([items[k]])[0], got[k]), k


def test_transform_with_a_method_equals_the_items_and_direct_is_the_default():
    rng = np.random.default_rng(9)
    x = np.stack([_signal(rng, 5000), _signal(rng, 5000)])
    rir = _rir(rng, 1500, 40)[None]
    y = HipReverbWithImpulseResponse(rir=rir, device="cuda:0", method="fft")(x, 16000)
    want = _run([(x[a],) + scaled_rir(rir[0]) + (True,) for a in range(2)])
    assert np.array_equal(y[0], want[0]) and np.array_equal(y[1], want[1])
    d = HipReverbWithImpulseResponse(rir=rir, device="cuda:0", method="direct")(x, 16000)
    assert np.array_equal(d, HipReverbWithImpulseResponse(rir=rir, device="cuda:0")(x, 16000))
    assert not np.array_equal(d, y) and np.abs(d - y).max() < 1e-4  # another arithmetic, the same signal


def test_an_arena_without_the_workspace_is_refused():
    rng = np.random.default_rng(10)
    x, hs, shift, _ = _item(rng, 3000, 1500, 3, False)
    front = np.concatenate([x, hs])
    arena = torch.zeros(len(front) + reverb_tail_floats([3000]), dtype=torch.float32, device="cuda:0")  # the direct form's size
    rv = HipReverb("cuda:0")  # (a handle of its own: the refused ticket stays planned)
    with pytest.raises(ValueError):
        reverb_in_arena(arena, [0], [3000], [3000], [1500], [shift], None, len(front), reverb=rv, method="fft")
    ticket, _, info = rv.plan([0], [3000], [3000], [1500], [shift], None, len(front), "fft")
    assert int(info[1]) == len(front) + reverb_fft_tail_floats([3000], [1500], [shift]) - 3
    with pytest.raises(_lib.HipFeatError) as e:
        rv.run(ticket, arena)  # the library's own check: nothing launched
    assert e.value.status == _lib.ERR_INVALID
    rv.close()


# ---- the two strategies' route over the reference's goldens (tests/golden/reverb.*), with the bars of tests/test_gpu_reverb.py ----------
# HipOnTheFlyFeatures(reverb_method=...) hands its keyword to FusedMiniBatch.features_of_tracks, HipAudioSamples(reverb_method=...) to
# FusedAudioBatch.audio_of_tracks (tests/test_reverb_fft_abi.py pins that); these two are called here, as the direct route's tests do.
import lhotse_amd as LA  # noqa: E402
from _golden import err_stats  # noqa: E402
from _reverb_golden import GROUPS, corpus_files, exact_audio, load_reverb_goldens, rir_samples, tracks_of  # noqa: E402
from lhotse_amd.compat import LOG_EPSILON  # noqa: E402
from lhotse_amd.input_strategies import FusedAudioBatch, FusedMiniBatch  # noqa: E402

REL_TOL, ABS_TOL = 1e-4, 2e-3  # the suite's bar for driver goldens (tests/test_gpu_reverb.py, tests/test_gpu_reference_drivers.py)
RESAMPLER_TOL = 1e-5           # (tests/test_gpu_resample.py)
SR = 16000


@pytest.fixture(scope="module")
def goldens():
    return load_reverb_goldens()


@pytest.fixture(scope="module")
def paths(tmp_path_factory, goldens):
    return corpus_files(tmp_path_factory.mktemp("wav"), goldens[1])


def _features(goldens, paths, group, **kw):
    arrays, meta = goldens
    entries = meta["groups"][group]
    cfg = LA.HipFbankConfig(device="cuda:0", edge_rule="batch_zero_pad") if group == "k2" else LA.HipFbankConfig(device="cuda:0")
    fm = FusedMiniBatch(LA.HipFbank(cfg), return_audio=True)
    feats, lens, audio = fm.features_of_tracks([tracks_of(e, paths, arrays) for e in entries], [e["want"] for e in entries], SR, **kw)
    return feats.cpu().numpy(), [int(x) for x in lens], [a.numpy() for a in audio]


def _audio_bars(goldens, group, audio_of):
    """The check of tests/test_gpu_reverb.py::test_returned_audio_meets_the_audio_bars over ``audio_of(i)``."""
    arrays, meta = goldens
    checked = 0
    for i, e in enumerate(meta["groups"][group]):
        if not e["audio"]:
            continue
        got, row = audio_of(i), e["tracks"][0]
        truth = exact_audio(arrays, group, i)
        rel, mx = R.distances(got, truth)
        bar_rel, bar_max = R.bars(e["reference_rel_l2"], e["reference_max_abs"], truth)
        if row["factor"] != 1.0:
            hs = R.scale_and_shift(rir_samples(arrays, row["reverb"]))[0]
            slack = RESAMPLER_TOL * e["gain"] * float(np.abs(hs.astype(np.float64)).sum())
            d = float(np.abs(got.astype(np.float64) - arrays[f"{group}/{i}/audio"]).max())
            print(group, i, "max abs from load_audio()", d, "bound", slack + bar_max + e["reference_max_abs"])
            assert d <= slack + bar_max + e["reference_max_abs"], (group, i, d, slack)
        else:
            print(group, i, f"device rel / bar {rel / bar_rel:.3f}  max / bar {mx / bar_max:.3f}")
            assert rel <= bar_rel and mx <= bar_max, (group, i, rel, bar_rel, mx, bar_max)
        checked += 1
    return checked


@pytest.mark.parametrize("group", GROUPS)
def test_features_of_tracks_on_the_fft_route_equal_the_reference_features(goldens, paths, group):
    arrays, meta = goldens
    entries = meta["groups"][group]
    got, lens, audio = _features(goldens, paths, group, reverb_method="fft")
    want = [arrays[f"{group}/{i}/feats"] for i in range(len(entries))]
    assert got.shape == (len(entries), max(len(w) for w in want), 80) and lens == [len(w) for w in want]
    for i, w in enumerate(want):
        s = err_stats(got[i, : len(w)], w)
        print(group, i, s)
        assert s["rel_l2"] <= REL_TOL and s["max_abs"] <= ABS_TOL, (group, i, s)
        assert np.all(got[i, len(w) :] == np.float32(LOG_EPSILON)) and len(audio[i]) == entries[i]["want"]
    if group in ("reverb", "options", "speed_reverb"):
        assert _audio_bars(goldens, group, lambda i: audio[i]) >= 2
    if group == "reverb":  # "direct" is the route without the keyword, bit for bit
        plain, explicit = _features(goldens, paths, group), _features(goldens, paths, group, reverb_method="direct")
        assert np.array_equal(plain[0], explicit[0]) and all(np.array_equal(a, b) for a, b in zip(plain[2], explicit[2]))
        assert not all(np.array_equal(a, b) for a, b in zip(plain[2], audio))  # (and the FFT route is another arithmetic)


@pytest.mark.parametrize("group", ["reverb", "options", "speed_reverb"])
def test_audio_of_tracks_on_the_fft_route_meets_the_audio_bars(goldens, paths, group):
    arrays, meta = goldens
    entries = meta["groups"][group]
    tracks, wants = [tracks_of(e, paths, arrays) for e in entries], [e["want"] for e in entries]
    batch = FusedAudioBatch("cuda:0")
    audio, lens = batch.audio_of_tracks(tracks, wants, SR, reverb_method="fft")
    assert audio.is_cuda and [int(x) for x in lens] == wants
    host = audio.cpu().numpy()
    assert _audio_bars(goldens, group, lambda i: host[i, : wants[i]]) >= 2
    plain, explicit = batch.audio_of_tracks(tracks, wants, SR), batch.audio_of_tracks(tracks, wants, SR, reverb_method="direct")
    assert torch.equal(plain[0], explicit[0]) and torch.equal(plain[1], explicit[1])
