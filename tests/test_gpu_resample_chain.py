"""GPU: cuts with a ``Resample`` at the front of their recording's transforms through the fused route
(``FusedMiniBatch.features_of_tracks`` with 8-element tracks, ``lhotse_amd.augmentation.resample_in_arena``) against what the REFERENCE
returned for the same cuts (tests/golden/resample_chain.*, written by tools/make_golden_resample_chain.py under the real lhotse: [Resample],
[Resample, Speed], CutMix over resampled tracks, [Resample, Speed, Reverb], one K2 mini-batch of mixed source rates).

Bars.  Features: the suite's bar for driver goldens (rel-L2 <= 1e-4, max abs <= 2e-3, tests/test_gpu_reference_drivers.py).  Audio:
max-abs distance from the exact float64 chain at most 2 x the reference's own stored distance + 2^-24 (the house rule of the mix and the
reverb); a single stage also within ABS_TOL = 1e-5 of ``load_audio()`` (tests/test_gpu_resample.py).  The reverb group is tested apart
from the others, so that a failure of the reverb kernels is told from one of the resampling route."""
import numpy as np
import pytest
import torch

import _resample_chain as RC
from _golden import err_stats

import lhotse_amd as LA
from lhotse_amd import augmentation as A
from lhotse_amd.compat import LOG_EPSILON
from lhotse_amd.input_strategies import FusedMiniBatch

pytestmark = pytest.mark.gpu
REL_TOL, ABS_TOL = 1e-4, 2e-3
RESAMPLER_TOL = 1e-5
SR = 16000


@pytest.fixture(scope="module")
def goldens():
    return RC.load_goldens()


@pytest.fixture(scope="module")
def paths(tmp_path_factory, goldens):
    return RC.source_files(tmp_path_factory.mktemp("srcwav"), goldens[1])


def run_group(goldens, paths, group):
    arrays, meta = goldens
    entries = meta["groups"][group]
    # groups 1-4: the reference framed every cut on its own; the K2 batch is ONE zero-padded batch
    ex = LA.HipFbank(LA.HipFbankConfig(device="cuda:0", edge_rule="batch_zero_pad")) if group == "k2" else LA.HipFbank(LA.HipFbankConfig(device="cuda:0"))
    rirs = {}
    tracks = [RC.tracks_of(e, paths, arrays, rirs) for e in entries]
    assert any(r["source_rate"] not in (None, SR) for e in entries for r in e["tracks"])
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


@pytest.mark.parametrize("group", ["resample", "resample_speed", "resample_cutmix"])
def test_audio_then_features_of_the_chain_against_the_reference(goldens, paths, group):
    arrays, _ = goldens
    entries, feats, lens, audio = run_group(goldens, paths, group)
    for i, e in enumerate(entries):  # audio first: a wrong sample explains a wrong feature, not the other way round
        got = audio[i].numpy()
        assert len(got) == e["want"] and e["audio"]
        truth = RC.exact_audio(arrays, group, i)
        d, bound = float(np.abs(got.astype(np.float64) - truth).max()), 2.0 * e["reference_max_abs"] + 2.0 ** -24
        print(group, i, "device max abs from the float64 chain", d, "reference", e["reference_max_abs"])
        assert d <= bound, (group, i, d, bound)
        rows = e["tracks"]
        if len(rows) == 1 and len(RC.stages(rows[0]["source_rate"], rows[0]["factor"])) == 1:
            assert float(np.abs(got - arrays[f"{group}/{i}/audio"]).max()) <= RESAMPLER_TOL, (group, i)
    check_features(goldens, group, entries, feats, lens)


def test_resample_speed_reverb_chain_against_the_reference(goldens, paths):
    entries, feats, lens, audio = run_group(goldens, paths, "resample_speed_reverb")
    assert all(r.get("reverb") for e in entries for r in e["tracks"]) and [len(a) for a in audio] == [e["want"] for e in entries]
    check_features(goldens, "resample_speed_reverb", entries, feats, lens)


def test_k2_batch_of_mixed_source_rates_against_the_reference(goldens, paths):
    entries, feats, lens, audio = run_group(goldens, paths, "k2")
    assert {"mixed", "resample", "resample+speed"} <= set(goldens[1]["k2_kinds"]) and [len(a) for a in audio] == [e["want"] for e in entries]
    check_features(goldens, "k2", entries, feats, lens)


def test_resample_in_arena_places_by_the_layout_and_equals_the_resampler(paths):
    xs = [np.ascontiguousarray(RC.read_wav(paths[k])[0]) for k in ("s44a", "s16a", "s22a", "s44b", "n8a", "s22b")]
    ratios = [(44100, SR), None, (22050, SR), (44100, SR), (8000, SR), (22050, SR)]
    lens = np.array([len(x) for x in xs], dtype=np.int64)
    offs = np.zeros(len(xs), dtype=np.int64)
    np.cumsum(((lens + 3) & ~3)[:-1], out=offs[1:])
    front = int(offs[-1] + lens[-1])
    host = np.full(((front + 3) & ~3) + A.resampled_tail_floats(lens, ratios), np.nan, dtype=np.float32)
    for x, o in zip(xs, offs):
        host[o : o + len(x)] = x
    arena = torch.from_numpy(host).cuda()
    po, pl = A.resample_in_arena(arena, offs, lens, ratios, front)
    lo, ll, end = A.resample_layout(offs, lens, ratios, front)
    assert np.array_equal(po, lo) and np.array_equal(pl, ll) and end == len(host)
    got = arena.cpu().numpy()
    assert np.array_equal(got[:front].view(np.uint32), host[:front].view(np.uint32))  # the inputs are untouched
    for x, r, o, n in zip(xs, ratios, po, pl):
        if r is None:
            assert np.array_equal(got[o : o + n], x)
        else:
            assert o % 4 == 0 and o >= front
            want = A.get_or_create_resampler(*r)(torch.from_numpy(x).cuda()).cpu().numpy()
            assert np.array_equal(got[o : o + n], want)
    with pytest.raises(ValueError, match="arena too small"):
        A.resample_in_arena(arena[: len(host) - 8], offs, lens, ratios, front)
    # on speed ratios it is perturb_speed_in_arena, bit for bit
    fac = [0.9, 1.0, 1.1, 1.1, 1.0, 0.9]
    a1, a2 = torch.from_numpy(np.resize(host, 2 * len(host))).cuda(), torch.from_numpy(np.resize(host, 2 * len(host))).cuda()
    p1 = A.perturb_speed_in_arena(a1, offs, lens, fac, SR, front)
    p2 = A.resample_in_arena(a2, offs, lens, [None if f == 1.0 else (round(SR * f), SR) for f in fac], front)
    assert np.array_equal(p1[0], p2[0]) and np.array_equal(p1[1], p2[1])
    for o, n in zip(p1[0], p1[1]):
        assert torch.equal(a1[o : o + n], a2[o : o + n])
