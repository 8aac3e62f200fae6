"""GPU: cuts whose recordings carry the band bracket of ``LowpassUsingResampling`` -- ``Resample(sr -> 2c) Resample(2c -> sr)`` -- through
the fused route (``FusedMiniBatch.features_of_tracks`` / ``FusedAudioBatch.audio_of_tracks`` with 9-element tracks whose blocks hold
``("rate", src, dst)`` steps; ``resample_in_arena`` routes them to the bankless kernel or the dense bank) against what the REFERENCE
returned for the same cuts (tests/golden/lowpass.*, written by tools/make_golden_lowpass.py under the real lhotse).

Bars.  Audio: max_abs <= 1e-4 against the reference's ``load_audio()``, the project's north-star bar; the bare bracket is expected near
2e-7 (two passes whose float32 sums alone differ), and the measured maximum per group is printed.  Features: per-cut rel-L2 <= 1e-4 against
the reference's ``Fbank`` (the K2 group: against the stored batch rows), and max abs <= 2e-3 -- the suite's bar for driver goldens
(tests/test_gpu_level_chain.py) -- over the mel bins that lie wholly below 0.8 x the lowest cutoff of the cut's brackets (all bins where a
track without a bracket fills the band).  Above the cutoff a lowpassed cut has next to nothing, and the logarithm turns an audio difference
of 1e-7 into 1e-3 there: those bins are held by the rel-L2 bar alone, and their max abs is printed."""
import numpy as np
import pytest
import torch

import _lowpass_golden as LP
from _golden import err_stats

import lhotse_amd as LA
from lhotse_amd.compat import LOG_EPSILON
from lhotse_amd.input_strategies import FusedAudioBatch, FusedMiniBatch

pytestmark = pytest.mark.gpu
REL_TOL, ABS_TOL, AUDIO_TOL = 1e-4, 2e-3, 1e-4
SR = 16000


@pytest.fixture(scope="module")
def goldens():
    return LP.load_lowpass_goldens()


@pytest.fixture(scope="module")
def paths(tmp_path_factory, goldens):
    return LP.corpus_files(tmp_path_factory.mktemp("lowpasswav"), goldens[1])


def run_group(goldens, paths, group):
    arrays, meta = goldens
    entries = meta["groups"][group]
    # the reference framed every cut on its own; the K2 batch is ONE zero-padded batch
    ex = LA.HipFbank(LA.HipFbankConfig(device="cuda:0", edge_rule="batch_zero_pad")) if group == "k2" else LA.HipFbank(LA.HipFbankConfig(device="cuda:0"))
    rirs = {}
    tracks = [LP.tracks_of(e, paths, arrays, rirs) for e in entries]
    assert any(len(t) == 9 and any(st[0] == "rate" for b in t[8] for st in b or []) for cut in tracks for t in cut)
    feats, lens, audio = FusedMiniBatch(ex, return_audio=True).features_of_tracks(tracks, [e["want"] for e in entries], SR)
    return entries, tracks, feats, lens, audio


def bins_below_the_cutoff(entry, num_bins=80, low=20.0, high=7600.0):
    """How many of the mel bins (lhotse's Fbank: 80 triangles between 20 Hz and sr / 2 - 400 Hz, evenly spaced in mel = 1127 ln(1 + f / 700),
    bin b reaching up to mel point b + 2) end below 0.8 x the lowest cutoff of the cut (half the lowest rate a track passes through); all
    of them when a track passes through no lower rate."""
    cutoffs = []
    for r in entry["tracks"]:
        if r["file"] is None:
            continue
        rates = [st[2] for b in (r.get("level") or [None, None]) for st in b or [] if st[0] == "rate" and st[2] < SR]
        rates += [r["source_rate"]] if r.get("source_rate") and r["source_rate"] < SR else []  # (a recording at a lower rate has nothing above its half)
        if not rates:
            return num_bins
        cutoffs.append(min(rates) / 2)
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)  # noqa: E731
    top = 700.0 * (np.exp((mel(low) + (np.arange(num_bins) + 2) * (mel(high) - mel(low)) / (num_bins + 1)) / 1127.0) - 1.0)
    return int((top <= 0.8 * min(cutoffs)).sum())


def check_features(goldens, group, entries, feats, lens):
    arrays, _ = goldens
    want = [arrays[f"{group}/{i}/feats"] for i in range(len(entries))]
    assert feats.is_cuda and tuple(feats.shape) == (len(entries), max(len(w) for w in want), 80)
    assert [int(x) for x in lens] == [len(w) for w in want]
    got = feats.cpu().numpy()
    for i, w in enumerate(want):
        s = err_stats(got[i, : len(w)], w)
        print(group, i, s)
        assert s["rel_l2"] <= REL_TOL, (group, i, s)
        nb = bins_below_the_cutoff(entries[i])
        below = float(np.abs(got[i, : len(w), :nb].astype(np.float64) - w[:, :nb]).max())
        print(group, i, f"max abs over the {nb} bins below the cutoff", below)
        assert nb >= 40 and below <= ABS_TOL, (group, i, nb, below)
        assert np.all(got[i, len(w) :] == np.float32(LOG_EPSILON))


def test_the_goldens_cover_the_ratios_and_the_groups(goldens):
    _, meta = goldens
    assert tuple(meta["groups"]) == LP.GROUPS or set(meta["groups"]) == set(LP.GROUPS)
    rates = {tuple(st[1:]) for e in meta["groups"]["band"] for r in e["tracks"] for st in r["level"][0]}
    assert rates == {(SR, 2 * c) for c in (4673, 3501, 7999, 4000)} | {(2 * c, SR) for c in (4673, 3501, 7999, 4000)}
    from lhotse_amd.augmentation import resample_route

    assert {resample_route(*r) for r in rates} == {"bank", "sinc"} and resample_route(SR, 8000) == "bank"
    assert {"mixed", "band"} <= set(meta["k2_kinds"])


@pytest.mark.parametrize("group", list(LP.AUDIO_GROUPS))
def test_audio_then_features_of_the_chain_against_the_reference(goldens, paths, group):
    arrays, _ = goldens
    entries, tracks, feats, lens, audio = run_group(goldens, paths, group)
    worst = 0.0
    for i, e in enumerate(entries):  # audio first: a wrong sample explains a wrong feature, not the other way round
        got = audio[i].numpy()
        assert len(got) == e["want"] and e["audio"]
        d = float(np.abs(got - arrays[f"{group}/{i}/audio"]).max())
        t = float(np.abs(got - LP.exact_audio(arrays, group, i)).max())
        print(group, i, "device max abs from load_audio()", d, "from the float64 chain", t, "reference's own", e["reference_max_abs"])
        assert d <= AUDIO_TOL, (group, i, d)
        worst = max(worst, d)
    print(f"{group}: max |audio - load_audio()| = {worst:.3g}")
    if group == "band":
        assert worst <= 1e-5  # (anything above needs an explanation, not a looser bar)
    check_features(goldens, group, entries, feats, lens)
    # the same cuts collated on the device: the arena's audio, bit for bit, zeros behind it
    coll, clens = FusedAudioBatch("cuda:0").audio_of_tracks(tracks, [e["want"] for e in entries], SR)
    coll = coll.cpu()
    assert [int(n) for n in clens] == [e["want"] for e in entries]
    for i, e in enumerate(entries):
        assert torch.equal(coll[i, : e["want"]], audio[i]) and not coll[i, e["want"] :].any()


@pytest.mark.parametrize("group", ["band_cutmix", "k2"])
def test_features_of_mixed_batches_against_the_reference(goldens, paths, group):
    entries, tracks, feats, lens, audio = run_group(goldens, paths, group)
    assert [len(a) for a in audio] == [e["want"] for e in entries]
    check_features(goldens, group, entries, feats, lens)
