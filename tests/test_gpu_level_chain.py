"""GPU: cuts whose recordings carry ``Volume`` / ``Clipping`` through the fused route (``FusedMiniBatch.features_of_tracks`` with 9-element
tracks, ``lhotse_amd.augmentation.level_in_arena``) against what the REFERENCE returned for the same cuts (tests/golden/level.*, written by
tools/make_golden_level.py under the real lhotse), and ``HipVolume`` / ``HipClipping`` on the same audio.

Bars.  Audio of a chain that holds only Volume or a hard Clipping: ``array_equal`` to the reference's ``load_audio()``.  Wherever a
resample, a speed, a reverb, a soft or an oversampled clip is involved: max-abs distance from the exact float64 chain at most 2 x the
reference's own stored distance + 2^-24 (the bar tests/test_gpu_resample_chain.py applies to its chains), and for the soft clip alone the
soft bar of tests/_level_ref.py.  Features: rel-L2 <= 1e-4, max abs <= 2e-3 (the suite's bar for driver goldens)."""
import numpy as np
import pytest
import torch

import _level_golden as LG
import _level_ref as L
from _golden import err_stats

import lhotse_amd as LA
from lhotse_amd.augmentation import HipClipping, HipVolume
from lhotse_amd.compat import LOG_EPSILON
from lhotse_amd.input_strategies import FusedMiniBatch

pytestmark = pytest.mark.gpu
REL_TOL, ABS_TOL = 1e-4, 2e-3
SR = 16000


@pytest.fixture(scope="module")
def goldens():
    return LG.load_level_goldens()


@pytest.fixture(scope="module")
def paths(tmp_path_factory, goldens):
    return LG.corpus_files(tmp_path_factory.mktemp("levelwav"), goldens[1])


def run_group(goldens, paths, group):
    arrays, meta = goldens
    entries = meta["groups"][group]
    # the reference framed every cut on its own; the K2 batch is ONE zero-padded batch
    ex = LA.HipFbank(LA.HipFbankConfig(device="cuda:0", edge_rule="batch_zero_pad")) if group == "k2" else LA.HipFbank(LA.HipFbankConfig(device="cuda:0"))
    rirs = {}
    tracks = [LG.tracks_of(e, paths, arrays, rirs) for e in entries]
    assert any(len(t) == 9 and t[8] is not None for cut in tracks for t in cut)
    feats, lens, audio = FusedMiniBatch(ex, return_audio=True).features_of_tracks(tracks, [e["want"] for e in entries], SR)
    return entries, feats, lens, audio


def check_features(goldens, group, entries, feats, lens):
    arrays, _ = goldens
    want = [arrays[f"{group}/{i}/feats"] for i in range(len(entries))]
    assert feats.is_cuda and tuple(feats.shape) == (len(entries), max(len(w) for w in want), 80)
    assert [int(x) for x in lens] == [len(w) for w in want]
    got = feats.cpu().numpy()
    for i, w in enumerate(want):
        s = err_stats(got[i, : len(w)], w)
        print(group, i, s)
        assert s["rel_l2"] <= REL_TOL and s["max_abs"] <= ABS_TOL, (group, i, s)
        assert np.all(got[i, len(w) :] == np.float32(LOG_EPSILON))


@pytest.mark.parametrize("group", ["volume", "clip_hard", "clip_soft", "clip_oversampled", "speed_volume_clip_reverb"])
def test_audio_then_features_of_the_chain_against_the_reference(goldens, paths, group):
    arrays, _ = goldens
    entries, feats, lens, audio = run_group(goldens, paths, group)
    for i, e in enumerate(entries):  # audio first: a wrong sample explains a wrong feature, not the other way round
        got = audio[i].numpy()
        assert len(got) == e["want"] and e["audio"]
        if group in LG.EXACT_GROUPS:
            assert np.array_equal(got, arrays[f"{group}/{i}/audio"]), (group, i)
            continue
        truth = LG.exact_audio(arrays, group, i)
        d_max, d_rel = L.distances(got, truth)
        print(group, i, "device max abs / rel-L2 from the float64 chain", d_max, d_rel, "reference", e["reference_max_abs"], e["reference_rel_l2"])
        assert d_max <= 2.0 * e["reference_max_abs"] + 2.0 ** -24, (group, i, d_max)
        if group == "clip_soft":
            bar_max, bar_rel = L.soft_bars(e["reference_max_abs"], e["reference_rel_l2"], truth)
            assert d_max <= bar_max and d_rel <= bar_rel, (group, i, d_max, bar_max, d_rel, bar_rel)
    check_features(goldens, group, entries, feats, lens)


@pytest.mark.parametrize("group", ["volume_cutmix", "k2"])
def test_features_of_mixed_batches_against_the_reference(goldens, paths, group):
    entries, feats, lens, audio = run_group(goldens, paths, group)
    assert [len(a) for a in audio] == [e["want"] for e in entries]
    if group == "k2":
        assert {"mixed", "level"} <= set(goldens[1]["k2_kinds"])
    check_features(goldens, group, entries, feats, lens)


def test_transforms_on_the_golden_audio(goldens, paths):
    """HipVolume / HipClipping over the file a golden cut read, against the reference's load_audio() of that cut."""
    arrays, meta = goldens
    for group, i in (("volume", 0), ("clip_hard", 0), ("clip_hard", 1)):
        row, = meta["groups"][group][i]["tracks"]
        (_, ops), = LG.steps_of(row["level"][0])
        y = LG.track_samples(row, paths)[None, :]
        for op in ops:
            y = (HipVolume(op[1]) if op[0] == "volume" else HipClipping(hard=op[1], gain_db=op[2], normalize=op[3]))(y, SR)
        assert y.dtype == np.float32 and np.array_equal(y[0], arrays[f"{group}/{i}/audio"]), (group, i)


def test_cuts_without_a_level_op_are_what_they_are_without_the_level_cuts(goldens, paths):
    """A mini-batch of level cuts, a plain cut, a speed-only cut and a mixed cut: the cuts without a level op come out exactly as from
    the same call without the level cuts."""
    arrays, meta = goldens
    rirs = {}
    level = [LG.tracks_of(meta["groups"][g][i], paths, arrays, rirs) for g, i in (("volume", 0), ("clip_oversampled", 1), ("speed_volume_clip_reverb", 0))]
    wants_level = [meta["groups"][g][i]["want"] for g, i in (("volume", 0), ("clip_oversampled", 1), ("speed_volume_clip_reverb", 0))]
    x = LG.track_samples({"file": "utt0", "first": 0, "count": 16000}, paths)
    noise = LG.track_samples({"file": "utt1", "first": 100, "count": 9000}, paths)
    others = [[(x[:7000], 1.0, 0, None, True)], [(x[:4000], 1.1, 0, None, True, 3636)],
              [(x[:8000], 1.0, 0, None, True, 8000), (noise, 0.9, 500, 12.0, False, 9000)]]
    wants_others = [7000, 3636, 9500]
    fm = FusedMiniBatch(LA.HipFbank(LA.HipFbankConfig(device="cuda:0")), return_audio=True)
    f0, l0, a0 = fm.features_of_tracks(others, wants_others, SR)
    order = [level[0], others[0], level[1], others[1], others[2], level[2]]
    wants = [wants_level[0], wants_others[0], wants_level[1], wants_others[1], wants_others[2], wants_level[2]]
    f1, l1, a1 = fm.features_of_tracks(order, wants, SR)
    for j, i in enumerate((1, 3, 4)):
        assert int(l0[j]) == int(l1[i]) and torch.equal(a0[j], a1[i]) and torch.equal(f0[j, : int(l0[j])], f1[i, : int(l1[i])]), (j, i)
