"""GPU: the tracks of MixedCuts mixed on the device (hipfeat_mix_*, lhotse_amd.augmentation.mix_in_arena,
FusedMiniBatch.features_of_tracks) against what the REFERENCE returned for the same cuts (tests/golden/mix.*, written by
tools/make_golden_mix.py under the real lhotse: CutMix, PerturbSpeed -> CutMix, pad, fixed-SNR mixes, one K2 mini-batch).

Bars.  Features: the suite's bar for driver goldens (rel-L2 <= 1e-4, max abs <= 2e-3, tests/test_gpu_reference_drivers.py).  Audio of
unperturbed tracks: against the exact float64 mix of the same float32 tracks; the device's rel-L2 may be at most 2 x the reference's own
distance from that mix + 2^-24 (both round the gain to float32 and add in the same order; the factor 2 covers the different rounding of
the energies).  Audio behind a device Speed: against load_audio() at the resampler's 1e-5 (tests/test_gpu_resample.py)."""
import numpy as np
import pytest
import torch

from _golden import err_stats, record_parity
from _mix_golden import corpus_files, exact_mix, load_mix_goldens, ref_tracks_of, tracks_of
from _mix_ref import mix_tracks

import lhotse_amd as LA
from lhotse_amd import _lib
from lhotse_amd.augmentation import HipMixer, get_or_create_mixer, mix_in_arena, mixed_tail_floats
from lhotse_amd.compat import LOG_EPSILON
from lhotse_amd.input_strategies import FusedMiniBatch

pytestmark = pytest.mark.gpu
REL_TOL, ABS_TOL = 1e-4, 2e-3
RESAMPLER_TOL = 1e-5
SR = 16000


@pytest.fixture(scope="module")
def goldens():
    return load_mix_goldens()


@pytest.fixture(scope="module")
def paths(tmp_path_factory, goldens):
    return corpus_files(tmp_path_factory.mktemp("wav"), goldens[1])


def _rel_l2(got, want):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / np.linalg.norm(want))


def _mix_on_device(cuts, wants=None, info=None):
    """cuts: [(tracks as _mix_ref.mix_tracks takes them, reference index)] -> the mixed cuts (numpy) through mix_in_arena alone.
    ``info``: a list that receives the plan's info block (the two calls mix_in_arena consists of are then made here)."""
    first, so, sl, do, snrs, refs, chunks, pos = [0], [], [], [], [], [], [], 0
    for tracks, ref in cuts:
        for x, o, snr in tracks:
            if np.isscalar(x):
                so.append(-1), sl.append(int(x))
            else:
                so.append(pos), sl.append(len(x)), chunks.append(np.asarray(x, dtype=np.float32))
                pos += len(x)
            do.append(int(o)), snrs.append(snr)
        first.append(len(so)), refs.append(ref)
    front = pos
    arena = torch.full((((front + 3) & ~3) + mixed_tail_floats(first, sl, do, wants),), float("nan"), dtype=torch.float32, device="cuda:0")
    arena[:front] = torch.from_numpy(np.concatenate(chunks))
    if info is None:
        offs, lens = mix_in_arena(arena, first, so, sl, do, snrs, refs, wants, front)
    else:
        mixer = get_or_create_mixer(arena.device)
        ticket, offs, lens, block = mixer.plan(first, so, sl, do, snrs, refs, wants, front)
        assert int(block[1]) <= arena.numel()
        info.append(block.copy())
        mixer.run(ticket, arena)
    host = arena.cpu().numpy()
    assert np.array_equal(host[:front], np.concatenate(chunks))  # the sources are untouched
    used = np.zeros(len(host), dtype=bool)
    used[:front] = True
    for o, n in zip(offs.tolist(), lens.tolist()):
        assert o % 4 == 0 and o >= front and not used[o : o + n].any()
        used[o : o + n] = True
    assert np.isnan(host[~used]).all()  # nothing else was written
    return [host[o : o + n].copy() for o, n in zip(offs.tolist(), lens.tolist())]


@pytest.mark.parametrize("group", ["cutmix", "speed_cutmix", "pad", "fixed", "k2"])
def test_features_of_tracks_equal_the_reference_features(goldens, paths, group):
    arrays, meta = goldens
    entries = meta["groups"][group]
    # groups 1-4: the reference framed every cut on its own; the K2 batch is ONE zero-padded batch
    ex = LA.HipFbank(LA.HipFbankConfig(device="cuda:0", edge_rule="batch_zero_pad")) if group == "k2" else LA.HipFbank(LA.HipFbankConfig(device="cuda:0"))
    feats, lens, _ = FusedMiniBatch(ex).features_of_tracks([tracks_of(e, paths) for e in entries], [e["want"] for e in entries], SR)
    want = [arrays[f"{group}/{i}/feats"] for i in range(len(entries))]
    assert feats.is_cuda and tuple(feats.shape) == (len(entries), max(len(w) for w in want), 80)
    assert [int(x) for x in lens] == [len(w) for w in want]
    got = feats.cpu().numpy()
    for i, w in enumerate(want):
        s = err_stats(got[i, : len(w)], w)
        print(group, i, s)
        record_parity("mix_features", (group, i), ex.kernel_name, got[i, : len(w)], w, w.astype(np.float64))
        assert s["rel_l2"] <= REL_TOL and s["max_abs"] <= ABS_TOL, (group, i, s)
        assert np.all(got[i, len(w) :] == np.float32(LOG_EPSILON))


@pytest.mark.parametrize("group", ["cutmix", "pad", "fixed"])
def test_mixed_audio_of_unperturbed_tracks_against_the_exact_mix(goldens, paths, group):
    arrays, meta = goldens
    entries = meta["groups"][group]
    ex = LA.HipFbank(LA.HipFbankConfig(device="cuda:0"))
    _, _, audio = FusedMiniBatch(ex, return_audio=True).features_of_tracks([tracks_of(e, paths) for e in entries], [e["want"] for e in entries], SR)
    checked = 0
    for i, e in enumerate(entries):
        got = audio[i].numpy()
        assert len(got) == e["want"]
        tracks, ref = ref_tracks_of(e, paths)
        covered = np.zeros(e["want"], dtype=bool)
        for x, o, _ in tracks:
            if not np.isscalar(x):
                covered[o : o + len(x)] = True
        assert np.all(got[~covered] == 0.0)  # samples no track covers are written, as zeros
        if all(r["snr"] is None or r["file"] == "zero" for r in e["tracks"]):  # gain exactly 1: the plain sum, bit for bit
            plain = mix_tracks([(x, o, None) for x, o, _ in tracks], -1, e["want"])
            assert np.array_equal(got, plain), (group, i)
        if e["exact"]:
            m64 = exact_mix(arrays, group, i)
            d, bound = _rel_l2(got, m64), 2.0 * e["reference_rel_l2"] + 2.0 ** -24
            print(group, i, "device rel-L2", d, "reference", e["reference_rel_l2"], "ratio", d / e["reference_rel_l2"] if e["reference_rel_l2"] else float("nan"))
            record_parity("mix_audio", (group, i), "mix_kernel", got, arrays[f"{group}/{i}/audio"], m64, rel_tol=bound, abs_tol=1.0)
            assert d <= bound, (group, i, d, bound)
            checked += 1
    assert checked >= 3


def test_mixed_audio_behind_a_device_speed_against_load_audio(goldens, paths):
    arrays, meta = goldens
    entries = meta["groups"]["speed_cutmix"]
    assert any(r["factor"] != 1.0 for e in entries for r in e["tracks"])
    ex = LA.HipFbank(LA.HipFbankConfig(device="cuda:0"))
    _, _, audio = FusedMiniBatch(ex, return_audio=True).features_of_tracks([tracks_of(e, paths) for e in entries], [e["want"] for e in entries], SR)
    checked = 0
    for i, e in enumerate(entries):
        assert len(audio[i]) == e["want"]
        if e["audio"]:
            d = float(np.abs(audio[i].numpy() - arrays[f"speed_cutmix/{i}/audio"]).max())
            print("speed_cutmix", i, "max abs", d)
            assert d <= RESAMPLER_TOL, (i, d)
            checked += 1
    assert checked >= 2


def test_routes_are_bit_identical(goldens, paths):
    arrays, meta = goldens
    entries = meta["groups"]["cutmix"] + meta["groups"]["fixed"]
    ex = LA.HipFbank(LA.HipFbankConfig(device="cuda:0"))
    fm = FusedMiniBatch(ex, return_audio=True)
    _, _, audio = fm.features_of_tracks([tracks_of(e, paths) for e in entries], [e["want"] for e in entries], SR)
    alone = _mix_on_device([ref_tracks_of(e, paths) for e in entries], [e["want"] for e in entries])
    for a, b in zip(audio, alone):
        assert np.array_equal(a.numpy(), b)
    # nothing changes for a batch without a mixed cut
    plain = [torch.from_numpy(ref_tracks_of(e, paths)[0][0][0]) for e in meta["groups"]["cutmix"]]
    f0, l0 = ex.extract_collated(plain, sampling_rate=SR, padding_value=LOG_EPSILON)
    f1, l1, a1 = fm.features_of_tracks([[(x, 1.0, 0, None, True)] for x in plain], [len(x) for x in plain], SR)
    assert torch.equal(f0, f1) and torch.equal(l0, l1) and all(torch.equal(a, x) for a, x in zip(a1, plain))


def _random_cut(rs, n_speech, noises, odd=True):
    speech = (rs.rand(n_speech).astype(np.float32) - 0.5) * 0.6
    tracks = [(speech, 0, None)]
    for n, off, snr in noises:
        tracks.append(((rs.rand(n).astype(np.float32) - 0.5) * rs.uniform(0.05, 1.0), off, snr))
    return tracks, 0


def _check_against_rule(cuts, wants, got):
    """Synthetic cuts have no golden: the yardsticks are the numpy rule of tests/_mix_ref.py -- `like_reference` (float32 energies) is tied
    to MixedCut.load_audio bit for bit only by the CPU tests under the real lhotse (tests/test_mix_reference.py), not here."""
    for (tracks, ref), w, g in zip(cuts, wants, got):
        m64 = mix_tracks(tracks, ref, w, accumulate=np.float64)
        like_reference = mix_tracks(tracks, ref, w, energy="float32")  # bit-equal to MixedCut.load_audio (tests/test_mix_reference.py)
        assert len(g) == len(m64)
        d, bound = _rel_l2(g, m64), 2.0 * _rel_l2(like_reference, m64) + 2.0 ** -24
        assert d <= bound, (d, bound)


# Sizes the large shapes sit on (tests/test_mix_abi.py::test_launch_constants_the_gpu_shapes_sit_on fails when one of them moves):
INLINE_BYTES = 3328      # kMbInlineBytes, lhotse_amd/csrc/kernel_minibatch.hpp:31: tables up to this size travel in the kernel arguments
LDS_TABLE_BYTES = 24576  # kMbLdsTableBytes, kernel_minibatch.hpp:32: staged tables up to this size are copied to LDS, larger ones searched in HBM
MAX_WORKGROUPS = 1792    # items_grid (hipfeat_mix_run), lhotse_amd/csrc/hipfeat.hip:1910: grid = ceil(items / ceil(items / 1792))
DESCRIPTOR_BYTES = 32    # sizeof(MixCut) = sizeof(MixTrack), lhotse_amd/csrc/mix_tables.hpp:39: one per cut and one per track
MIX_BLOCK, ENERGY_BLOCK = 4096, 16384  # kMixBlock, kMixEnergyBlock (mix_tables.hpp:18-19): samples per mix item / energy item


def _route(table_bytes):
    return "kernel arguments" if table_bytes <= INLINE_BYTES else "LDS copy" if table_bytes <= LDS_TABLE_BYTES else "HBM"


def _work(cuts, info):
    """info: what the plan that ran reported -> (its energy items, its mix items, the bytes of its tables)"""
    mix_items = sum(-(-max(o + (x if np.isscalar(x) else len(x)) for x, o, _ in tracks) // MIX_BLOCK) for tracks, _ in cuts)
    assert int(info[3]) == mix_items
    return int(info[2]), mix_items, DESCRIPTOR_BYTES * (len(cuts) + sum(len(tracks) for tracks, _ in cuts))


def _check_batch(cuts, wants, got, alone=6):
    """The rule bar for every cut; the plain sum, bit for bit, where no track carries an SNR; `alone` spread-out cuts equal to the same
    cut mixed on its own (its launch has one or a few work items: no workgroup takes a second one, the tables travel in the arguments)."""
    _check_against_rule(cuts, wants, got)
    plain = 0
    for (tracks, ref), w, g in zip(cuts, wants, got):
        if all(snr is None for _, _, snr in tracks):
            assert np.array_equal(g, mix_tracks(tracks, -1, w))
            plain += 1
    for k in sorted({int(i) for i in np.linspace(0, len(cuts) - 1, alone)}):
        assert np.array_equal(_mix_on_device([cuts[k]], [wants[k]])[0], got[k]), k
    return plain


def test_determinism_and_order_independence():
    rs = np.random.RandomState(5)
    cuts = [_random_cut(rs, n, [(m, o, s)]) for n, m, o, s in [(16000, 9000, 1201, 12.5), (40000, 40000, 0, 10.0), (5000, 777, 4223, 20.0), (20001, 20000, 1, 17.0)]]
    a = _mix_on_device(cuts)
    b = _mix_on_device(cuts)
    c = _mix_on_device(cuts[::-1])[::-1]
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    _check_against_rule(cuts, [-1] * len(cuts), a)


def test_shapes_that_break_work_distribution():
    rs = np.random.RandomState(6)
    # one 30 s cut with six short noise tracks (an odd offset, a track that starts on the last sample of the cut)
    n = 30 * SR
    long_cut = _random_cut(rs, n, [(8000, 1, 10.0), (12345, 100003, 15.0), (4001, 250000, 20.0), (16000, 399999, 12.0), (5000, n - 5000, 18.0), (1, n - 1, 10.0)])
    got = _mix_on_device([long_cut])
    _check_against_rule([long_cut], [-1], got)
    # 200 cuts of 0.1-1 s: the tables travel through pinned memory
    many = [_random_cut(rs, int(rs.randint(1600, 16000)), [(int(rs.randint(800, 1600)), int(rs.randint(0, 800)), float(rs.uniform(10, 20)))]) for _ in range(200)]
    got = _mix_on_device(many)
    _check_against_rule(many, [-1] * len(many), got)
    # 1900 cuts of 50-100 ms: 178 KB of tables, searched where they are staged (they do not fit the LDS copy); 3800 energy items and
    # 1900 mix items, both more than the 1792 workgroups of a launch: the workgroups of both kernels take a second item
    tiny = [_random_cut(rs, int(rs.randint(800, 1600)), [(int(rs.randint(100, 800)), int(rs.randint(0, 100)), float(rs.uniform(10, 20)))]) for _ in range(1900)]
    info = []
    got = _mix_on_device(tiny, info=info)
    energy_items, mix_items, table_bytes = _work(tiny, info[0])
    print(f"tiny: {energy_items} energy items, {mix_items} mix items, tables {table_bytes} B ({_route(table_bytes)})")
    assert energy_items == 3800 and mix_items == 1900 and min(energy_items, mix_items) > MAX_WORKGROUPS and _route(table_bytes) == "HBM"
    _check_batch(tiny, [-1] * len(tiny), got)
    # truncation by one sample; a padding track that only lengthens the cut
    cut = ([((rs.rand(8001).astype(np.float32) - 0.5), 0, None), ((rs.rand(4000).astype(np.float32) - 0.5), 333, 15.0)], 0)
    padded = ([(2000, 0, None), ((rs.rand(3000).astype(np.float32) - 0.5), 2000, None), (9000, 0, None)], 1)
    got = _mix_on_device([cut, padded], [8000, -1])
    assert len(got[0]) == 8000 and len(got[1]) == 9000
    _check_against_rule([cut, padded], [8000, -1], got)
    assert np.all(got[1][:2000] == 0) and np.all(got[1][5000:] == 0) and np.array_equal(got[1][2000:5000], padded[0][1][0])


def test_long_cuts_in_the_kernel_arguments_with_more_mix_items_than_workgroups():
    """30 cuts of 17.5 s = 69 mix items each, 2070 in all: the workgroups of the mix launch take a second item while the tables still
    travel in the kernel arguments -- 30 cuts + 30 speech tracks + 44 noise tracks (two for 14 of the cuts, one for the others) are the
    104 descriptors that just fit."""
    rs = np.random.RandomState(11)
    n = 280000
    cuts = []
    for k in range(30):
        noises = [(int(rs.randint(2000, 9000)), int(rs.randint(0, n - 9000)), float(rs.uniform(5, 20))) for _ in range(2 if k % 2 == 0 and k < 28 else 1)]
        cuts.append(_random_cut(rs, n, noises))
    info = []
    got = _mix_on_device(cuts, info=info)
    energy_items, mix_items, table_bytes = _work(cuts, info[0])
    print(f"long: {energy_items} energy items, {mix_items} mix items, tables {table_bytes} B ({_route(table_bytes)})")
    assert mix_items == 2070 > MAX_WORKGROUPS and table_bytes == INLINE_BYTES and _route(table_bytes) == "kernel arguments"
    assert energy_items == 30 * -(-n // ENERGY_BLOCK) + 44
    _check_batch(cuts, [-1] * len(cuts), got)


@pytest.mark.parametrize("descriptors,mixed,single,padding", [(104, 34, 1, 0), (105, 34, 1, 1), (768, 254, 3, 0), (769, 254, 3, 1)])
def test_table_routes_at_their_boundaries(descriptors, mixed, single, padding):
    """104 | 105 descriptors (cuts + tracks, 32 bytes each): the last tables that fit the kernel arguments and the first that are staged;
    768 | 769: the last that are searched in LDS and the first that are searched in HBM.  `mixed` cuts of a speech and a noise track at
    an SNR (3 descriptors), `single` cuts of one track (2; the plain sum applies), and `padding` = 1: a padding track on one of them."""
    rs = np.random.RandomState(descriptors)
    cuts = [_random_cut(rs, int(rs.randint(800, 3000)), [(int(rs.randint(100, 800)), int(rs.randint(0, 100)), float(rs.uniform(10, 20)))]) for _ in range(mixed)]
    for k in range(single):  # spread over the list; the first one takes the padding track, which lengthens it
        x = (rs.rand(int(rs.randint(800, 3000))).astype(np.float32) - 0.5) * 0.6
        tracks = [(x, 0, None)] + ([(len(x) + 500, 0, None)] if padding and k == 0 else [])
        cuts.insert((k * len(cuts)) // single + k, (tracks, -1))
    assert len(cuts) + sum(len(t) for t, _ in cuts) == descriptors
    info = []
    got = _mix_on_device(cuts, info=info)
    energy_items, mix_items, table_bytes = _work(cuts, info[0])
    print(f"{descriptors} descriptors: {energy_items} energy items, {mix_items} mix items, tables {table_bytes} B ({_route(table_bytes)})")
    assert table_bytes == DESCRIPTOR_BYTES * descriptors
    assert _route(table_bytes) == {104: "kernel arguments", 105: "LDS copy", 768: "LDS copy", 769: "HBM"}[descriptors]
    assert energy_items == 2 * mixed and mix_items == len(cuts)
    assert _check_batch(cuts, [-1] * len(cuts), got) == single
    if padding:
        k = next(i for i, (t, _) in enumerate(cuts) if len(t) == 2 and np.isscalar(t[1][0]))
        assert len(got[k]) == len(cuts[k][0][0][0]) + 500 and np.all(got[k][-500:] == 0)


def test_gains_follow_the_reference_track_and_the_snr():
    """Tracks whose energies lie 20-50 dB apart and a reference track that is NOT the first one: a wrong reference index, a wrong sign of
    the SNR or a swapped energy ratio moves a gain by orders of magnitude, far outside the bar."""
    rs = np.random.RandomState(9)
    n = 24000
    loud = (rs.rand(n).astype(np.float32) - 0.5)                # ~ -11 dB
    quiet = (rs.rand(20000).astype(np.float32) - 0.5) * 3e-3    # ~ -61 dB
    mid = (rs.rand(9000).astype(np.float32) - 0.5) * 0.05       # ~ -37 dB
    cuts = [([(2000, 0, None), (quiet, 2000, 5.0), (loud, 1000, None), (mid, 7001, -10.0)], 2),  # padding first, reference = track 2
            ([(quiet, 0, None), (loud, 0, 30.0), (mid, 11, 0.0)], 0),                             # reference = the quiet first track
            ([(mid, 0, 12.0), (loud, 0, 3.0), (quiet, 5, None)], 2)]                               # first track scaled against track 2
    got = _mix_on_device(cuts)
    _check_against_rule(cuts, [-1] * len(cuts), got)
    # the gains themselves, read back from a region only one track covers
    from _mix_ref import track_gains

    g = track_gains(cuts[1][0], 0)  # reference = the quiet first track: the loud one is pushed 30 dB below it
    assert 5e-5 < g[1] < 2e-4 and np.allclose(got[1][20000:], g[1] * loud[20000:], rtol=1e-6, atol=0)  # (only the loud track lies there)
    g = track_gains(cuts[0][0], 2)  # reference = track 2 behind a padding track: the quiet one is lifted to 5 dB below it
    assert g[1] > 100 and g[3] > 30
    assert np.array_equal(got[0][22000:], loud[21000:]) and np.array_equal(got[0][1000:2000], loud[:1000]) and np.all(got[0][:1000] == 0)
    assert np.allclose(got[0][2000:7001], g[1] * quiet[:5001] + loud[1000:6001], rtol=0, atol=1e-6)


def test_a_batch_in_which_no_cut_needs_mixing_launches_no_mix():
    """A mixed cut whose other tracks are muted arrives as ONE unscaled track at offset 0 (lhotse_amd.input_strategies.deferred_mix):
    the route of mixed mini-batches must serve it without a mix plan (hipfeat_mix_plan refuses an empty batch)."""
    rs = np.random.RandomState(10)
    xs = [torch.from_numpy((rs.rand(n).astype(np.float32) - 0.5)) for n in (16000, 9000)]
    ex = LA.HipFbank(LA.HipFbankConfig(device="cuda:0"))
    fm = FusedMiniBatch(ex, return_audio=True)
    f0, l0 = ex.extract_collated(xs, sampling_rate=SR, padding_value=LOG_EPSILON)
    f1, l1, a1 = fm._mix_and_extract([[(x, 1.0, 0, None, True, len(x))] for x in xs], [len(x) for x in xs], SR)
    assert torch.equal(f0, f1) and torch.equal(l0, l1) and all(torch.equal(a, x) for a, x in zip(a1, xs))
    # ... and behind a device Speed: the same as the speed route
    f2, l2, a2 = fm._mix_and_extract([[(xs[0], 1.1, 0, None, True, 14545)], [(xs[1], 1.0, 0, None, True, 9000)]], [14545, 9000], SR)
    f3, l3, a3 = fm.features_of_tracks([[(xs[0], 1.1, 0, None, True, 14545)], [(xs[1], 1.0, 0, None, True, 9000)]], [14545, 9000], SR)
    assert torch.equal(f2, f3) and torch.equal(l2, l3) and all(torch.equal(a, b) for a, b in zip(a2, a3))


def test_bad_tables_are_refused_and_launch_nothing():
    mixer = HipMixer("cuda:0")
    arena = torch.zeros(4096, dtype=torch.float32, device="cuda:0")
    sentinel = arena.clone()

    def status(**kw):
        args = dict(track_first=[0, 2], src_offsets=[0, 1000], src_lens=[1000, 500], dst_offsets=[0, 10], snrs=[None, 10.0], ref_tracks=[0], max_samples=None,
                    tail_start=1500)
        args.update(kw)
        with pytest.raises(_lib.HipFeatError) as e:
            mixer.plan(**args)
        return e.value.status

    assert status(src_offsets=[0, 1200]) == _lib.ERR_INVALID  # a source reaches into the tail, where the mixed cuts are written
    assert status(ref_tracks=[2]) == _lib.ERR_INVALID and status(ref_tracks=[-2]) == _lib.ERR_INVALID  # reference index outside the cut
    assert status(src_offsets=[-1, 1000]) == _lib.ERR_INVALID  # the reference track is a padding track
    assert status(dst_offsets=[0, -1]) == _lib.ERR_INVALID and status(src_offsets=[0, -5]) == _lib.ERR_INVALID  # negative offsets
    assert status(track_first=[0, 0], src_offsets=[], src_lens=[], dst_offsets=[], snrs=[], ref_tracks=[-1]) == _lib.ERR_INVALID  # a cut without tracks
    assert status(src_lens=[1000, 0]) == _lib.ERR_INVALID
    n = 257
    assert status(track_first=[0, n], src_offsets=[0] * n, src_lens=[10] * n, dst_offsets=[0] * n, snrs=[None] * n, ref_tracks=[-1]) == _lib.ERR_UNSUPPORTED
    ticket, offs, lens, info = mixer.plan([0, 2], [0, 1000], [1000, 500], [0, 10], [None, 10.0], [0], None, 1500)
    assert int(offs[0]) == 1500 and int(lens[0]) == 1000 and int(info[1]) == 2500
    with pytest.raises(_lib.HipFeatError) as e:  # arena too small
        mixer.run(ticket, arena[:2496])
    assert e.value.status == _lib.ERR_INVALID
    with pytest.raises(_lib.HipFeatError) as e:  # unknown ticket
        mixer.run(ticket + 5, arena)
    assert e.value.status == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(arena, sentinel)  # nothing was launched
    mixer.run(ticket, arena)  # (the refused calls left the plan as it was)
    with pytest.raises(_lib.HipFeatError):  # a ticket runs once
        mixer.run(ticket, arena)
    torch.cuda.synchronize()
    tickets = [mixer.plan([0, 1], [0], [100], [0], None, None, None, 1500)[0] for _ in range(16)]
    with pytest.raises(_lib.HipFeatError) as e:  # a 17th plan would drop a live one
        mixer.plan([0, 1], [0], [100], [0], None, None, None, 1500)
    assert e.value.status == _lib.ERR_INVALID
    mixer.run(tickets[0], arena)
    mixer.plan([0, 1], [0], [100], [0], None, None, None, 1500)  # (a slot is free again)
    torch.cuda.synchronize()
    # destroy with planned but unrun tickets is clean
    mixer.close()
    assert mixer.handle == 0
