"""CPU, under the real lhotse (authoring container only): the band bracket ``Resample(sr -> m) Resample(m -> sr)`` that
``LowpassUsingResampling`` (lhotse/dataset/cut_transforms/lowpass.py) appends, taken by the level rule.

  * ``parse_chain`` takes every lowpassed cut -- alone, behind a ``Speed``, with ``Volume`` / ``Clipping``, around a reverb, as the
    track of a mix -- and gives the expected steps; it refuses the counter-examples, each by its own case;
  * ``read_before_chain`` / ``chain_num_samples`` give the sample counts the reference's own transforms produce;
  * ``HipOnTheFlyFeatures`` with CPU stand-ins for the device (``_sinc_ref``, the banded float64 truth rounded to float32, in place of the
    resampling launches) is within the audio bar of the reference's ``load_audio()`` -- max_abs <= 1e-4, the project's north-star bar --
    and within the feature bar of its ``Fbank``, without one ``load_audio()`` of a lowpassed cut.
The cutoffs cover 8000:4673, 8000:3501 and 8000:7999 (no dense bank is built for them here) and 2:1 (under the 2^20 threshold)."""

import numpy as np
import pytest
import torch

import _sinc_ref as SRF
from test_level_reference import _level_chain, _rir, _with_transforms, cpu_level
from test_resample_chain_reference import cpu_perturb, cpu_reverb

SR = 16000
REL_TOL, ABS_TOL = 1e-4, 2e-3  # the suite's bar for driver goldens (tests/test_gpu_reference_drivers.py)
AUDIO_TOL = 1e-4
CUTOFFS = [4673, 3501, 7999, 4000]
pytestmark = pytest.mark.reference


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from _dropin_support import import_lhotse, install_wave_backend, write_cutset

    import_lhotse()
    import lhotse.augmentation.torchaudio as ref_ta
    from lhotse.audio.backend import set_current_audio_backend

    was = ref_ta.is_torchaudio_available
    ref_ta.is_torchaudio_available = lambda: True  # the reference's sinc branch
    prev = install_wave_backend()
    cuts = list(write_cutset(tmp_path_factory.mktemp("lowpasswav"), [6000, 4800, 7200, 5000, 8000, 3000], seed=7))
    yield cuts
    set_current_audio_backend(prev)
    ref_ta.is_torchaudio_available = was


def lowpass(cut, cutoff):
    return cut.resample(2 * cutoff).resample(SR)  # lowpass.py:45


def band(cutoff):
    return [("rate", SR, 2 * cutoff), ("rate", 2 * cutoff, SR)]


def test_the_transform_itself_appends_the_bracket_and_the_rule_takes_it(env):
    from lhotse import CutSet
    from lhotse.dataset.cut_transforms.lowpass import LowpassUsingResampling

    import lhotse_amd.input_strategies as IS

    cuts = list(LowpassUsingResampling(p=1.0, seed=3)(CutSet.from_cuts(env)))
    assert len(cuts) == len(env)
    for cut in cuts:
        names = [IS._transform_name(t) for t in cut.recording.transforms]
        (a, m), (m2, b) = (IS._resample_rates(t) for t in cut.recording.transforms)
        assert names == ["Resample", "Resample"] and a == b == SR == cut.sampling_rate and m == m2 and 7000 <= m < 16000 and m % 2 == 0
        assert _level_chain(IS, cut) == (None, 1.0, None, ([("rate", SR, m), ("rate", m, SR)], None)), cut.id
        assert IS.parse_chain(cut, gpu_level=False) is None and IS.parse_chain(cut, gpu_level=False, bankless=True) is None  # the level route off


def test_pending_level_chain_accepts_the_bracket_in_its_grammar_and_refuses_the_rest(env, tmp_path, monkeypatch):
    import wave

    import lhotse.augmentation.torchaudio as ref_ta
    from lhotse import MonoCut, Recording
    from lhotse.audio import AudioSource
    from lhotse.audio import resampling_backend as RB
    from lhotse.augmentation import Resample, Volume

    import lhotse_amd.input_strategies as IS

    c = env[0]
    rir = _rir(tmp_path)
    lvl = lambda *ops: ("level", list(ops))  # noqa: E731
    for cutoff in CUTOFFS:
        assert _level_chain(IS, lowpass(c, cutoff)) == (None, 1.0, None, (band(cutoff), None))
    assert _level_chain(IS, lowpass(c.perturb_speed(1.1), 4673)) == (None, 1.1, None, (band(4673), None))
    got = _level_chain(IS, lowpass(c, 3501).perturb_volume(0.5).clip_amplitude(hard=True, gain_db=6.0, normalize=False, oversampling=None))
    assert got == (None, 1.0, None, (band(3501) + [lvl(("volume", 0.5), ("clip", True, 6.0, False))], None))
    got = _level_chain(IS, lowpass(c.perturb_volume(0.5), 3501).perturb_volume(2.0))  # four ops: Volume, the bracket (two), Volume
    assert got[3] == ([lvl(("volume", 0.5))] + band(3501) + [lvl(("volume", 2.0))], None)
    assert _level_chain(IS, lowpass(lowpass(c, 4673), 3501))[3] == (band(4673) + band(3501), None)  # two brackets: four ops
    src, factor, rv, blocks = _level_chain(IS, lowpass(c, 7999).reverb_rir(rir))
    assert (src, factor) == (None, 1.0) and rv["normalize_output"] is True and blocks == (band(7999), None)
    assert _level_chain(IS, lowpass(c.reverb_rir(rir), 7999))[3] == (None, band(7999))
    res = _with_transforms(c, [Resample(44100, SR), Resample(SR, 9346), Resample(9346, SR)])
    assert _level_chain(IS, res) == (44100, 1.0, None, (band(4673), None))
    mixed = lowpass(c, 4673).pad(duration=c.duration + 0.1)
    tracks = IS.deferred_mix(mixed, gpu_resample=True, gpu_level=True)
    assert tracks is not None and tracks[0].chain == IS.Chain(pre=band(4673))
    assert IS.deferred_mix(mixed, gpu_resample=True) is None and IS.deferred_mix(mixed) is None  # without gpu_level: the reference's path

    # what keeps cut.load_audio(), each by its own case
    two = tmp_path / "two.wav"
    with wave.open(str(two), "wb") as f:
        f.setnchannels(2), f.setsampwidth(2), f.setframerate(SR)
        f.writeframes((np.random.RandomState(9).rand(4000, 2) * 20000 - 10000).astype(np.int16).tobytes())
    rec2 = Recording(id="two", sources=[AudioSource(type="file", channels=[0, 1], source=str(two))], sampling_rate=SR, num_samples=4000, duration=4000 / SR)
    refused = {
        "a window beyond the kernel's cap (16000 -> 2001: 100 taps per phase, and no dense bank)": _with_transforms(c, [Resample(SR, 2001), Resample(2001, SR)]),
        "a stereo recording": lowpass(MonoCut(id="mono-of-two", start=0, duration=4000 / SR, channel=0, recording=rec2), 4673),
        "a lone Resample(sr -> m)": _with_transforms(c, [Resample(SR, 9346)]),
        "a bracket that closes at another rate": _with_transforms(c, [Resample(SR, 9346), Resample(9346, 8000)]),
        "a bracket that closes from another rate": _with_transforms(c, [Resample(SR, 9346), Resample(9348, SR)]),
        "two brackets and two other ops: six ops": lowpass(lowpass(c.perturb_volume(0.5), 4673), 3501).perturb_volume(2.0),
        "a bracket and three other ops: five ops": lowpass(c.perturb_volume(0.5).perturb_volume(0.5), 4673).perturb_volume(2.0),
        "a bracket in front of the Speed": lowpass(c, 4673).perturb_speed(1.1),
    }
    for why, cut in refused.items():
        assert _level_chain(IS, cut) is None, why
    ok = lowpass(c, 4673)
    assert _level_chain(IS, ok, gpu_resample=False) is None
    monkeypatch.setattr(RB, "CURRENT_RESAMPLING_BACKEND", "sox")
    assert _level_chain(IS, ok) is None
    monkeypatch.setattr(RB, "CURRENT_RESAMPLING_BACKEND", "default")
    monkeypatch.setattr(ref_ta, "is_torchaudio_available", lambda: False)  # the reference would resample with scipy's resample_poly
    assert _level_chain(IS, ok) is None
    monkeypatch.setattr(ref_ta, "is_torchaudio_available", lambda: True)
    assert _level_chain(IS, ok) is not None
    # the small pair is served too (its two stages go to the dense bank), and Volume alone is what it was
    assert _level_chain(IS, _with_transforms(c, [Volume(0.5)])) == (None, 1.0, None, ([lvl(("volume", 0.5))], None))


def test_sample_counts_are_the_reference_s(env):
    from lhotse.augmentation import AudioTransform
    from lhotse.utils import compute_num_samples

    import lhotse_amd.input_strategies as IS

    for cut, cutoff, factor in ((env[0], 4673, 1.0), (env[2], 3501, 1.0), (env[1], 7999, 1.0), (env[3], 4000, 1.0), (env[2].truncate(offset=0.05, duration=0.3), 4673, 1.0),
                                (env[4], 5000, 0.9), (env[4], 6811, 1.1)):
        lp = lowpass(cut if factor == 1.0 else cut.perturb_speed(factor), cutoff)
        lc = _level_chain(IS, lp)
        raw = IS.read_before_chain(lp)
        # the reference's own transforms over what was read, with its own objects
        y = raw[None, :]
        for t in lp.recording.transforms:
            y = (AudioTransform.from_dict(t) if isinstance(t, dict) else t)(y, SR)
        n = IS.chain_num_samples(len(raw), lc[0], lc[1], SR, lc[3])
        want = compute_num_samples(lp.duration, SR)
        assert n == y.shape[1] and n >= want and len(lp.load_audio()[0]) == want, (cut.id, cutoff, factor, n, y.shape, want)
        track = IS._read_track(lp, IS.parse_chain(lp, bankless=True))
        assert track is not None and track.cap == want and np.array_equal(track.samples, raw) and track.levels == lc[3]
    assert IS.chain_num_samples(1000, None, 1.0, SR, (band(4673), None)) == int(np.ceil(np.float32(8000 * int(np.ceil(np.float32(4673 * 1000 / 8000))) / 4673)))
    assert IS.chain_num_samples(1000, None, 1.0, SR, ([("up", 2), ("level", []), ("down", 2)], None)) == 1000 == IS.chain_num_samples(1000, None, 1.0, SR)


def cpu_sinc_resample(arena, offsets, lengths, ratios, tail_start):
    """``resample_in_arena`` on a host arena: the layout is the product's own, the samples are the banded float64 truth, rounded once."""
    from lhotse_amd.augmentation import resample_layout

    po, pl, _ = resample_layout(offsets, lengths, ratios, tail_start)
    served = [i for i, r in enumerate(ratios) if r is not None]
    for i in served:  # what hipfeat_sinc_plan refuses: an output that meets an input of the call (the head-room was counted wrongly)
        for j in served:
            assert int(po[i]) + int(pl[i]) <= int(offsets[j]) or int(offsets[j]) + int(lengths[j]) <= int(po[i]), (i, j, "an output overlaps an input")
    for i, r in enumerate(ratios):
        if r is not None:
            x = arena[int(offsets[i]) : int(offsets[i]) + int(lengths[i])].numpy().copy()
            y = SRF.resample(x, int(r[0]), int(r[1])).astype(np.float32)
            assert len(y) == int(pl[i])
            arena[int(po[i]) : int(po[i]) + int(pl[i])] = torch.from_numpy(y)
    return po, pl


@pytest.fixture
def stand_ins(monkeypatch):
    import lhotse_amd.extractors as E
    import lhotse_amd.input_strategies as IS
    from _dropin_support import make_cpu_plan
    from _mix_ref import mix_in_arena_cpu

    calls = {"resample": 0, "ratios": set()}

    def resample(arena, offsets, lengths, ratios, tail_start):
        calls["resample"] += 1
        calls["ratios"] |= {r for r in ratios if r is not None}
        return cpu_sinc_resample(arena, offsets, lengths, ratios, tail_start)

    monkeypatch.setattr(E, "_Plan", make_cpu_plan())
    monkeypatch.setattr(IS, "_level_in_arena", cpu_level)
    monkeypatch.setattr(IS, "_resample_in_arena", resample)
    monkeypatch.setattr(IS, "_perturb_in_arena", cpu_perturb)
    monkeypatch.setattr(IS, "_mix_in_arena", mix_in_arena_cpu)
    monkeypatch.setattr(IS, "_reverb_in_arena", cpu_reverb)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    return calls


def test_the_route_with_stand_ins_is_within_the_audio_bar_of_the_reference(env, tmp_path, stand_ins, monkeypatch):
    from lhotse import CutSet
    from lhotse.dataset.cut_transforms import CutMix
    from lhotse.dataset.input_strategies import OnTheFlyFeatures
    from lhotse.features.kaldi.extractors import Fbank

    import lhotse_amd as LA
    import lhotse_amd.input_strategies as IS

    c0, c1, c2, c3, c4, c5 = env
    rir = _rir(tmp_path)
    mixed = list(CutMix(CutSet.from_cuts([c4]), snr=15, p=1.0, pad_to_longest=False, random_mix_offset=False, seed=3)(CutSet.from_cuts([lowpass(c3, 4673)])))[0]
    assert type(mixed).__name__ == "MixedCut"
    groups = {"band": [lowpass(c0, 4673), lowpass(c1, 3501), lowpass(c5, 7999), lowpass(c2, 4000)],
              "speed_band": [lowpass(c1.perturb_speed(1.1), 4673)],
              "band_volume_clip": [lowpass(c2, 3501).perturb_volume(1.7).clip_amplitude(hard=False, gain_db=9.0, oversampling=None)],
              "band_reverb": [lowpass(c2, 3501).reverb_rir(rir), lowpass(c5.reverb_rir(rir), 4673)],  # (in front of the reverb: a sample more reaches it)
              "band_cutmix": [mixed]}
    labelled = [(g, c) for g, members in groups.items() for c in members]
    labelled = labelled[:3] + [(None, c4), (None, c1.perturb_speed(0.9))] + labelled[3:]
    batch = CutSet.from_cuts([c for _, c in labelled])
    want_f, want_l, want_a, want_al = OnTheFlyFeatures(Fbank(), return_audio=True)(batch)

    def is_lowpassed(cut):
        if type(cut).__name__ == "MixedCut":
            return any(is_lowpassed(t.cut) for t in cut.tracks)
        return type(cut).__name__ == "MonoCut" and any(IS._transform_name(t) == "Resample" for t in cut.recording.transforms or [])

    loads = []
    for cls in {type(c) for c in batch}:
        real = cls.load_audio
        monkeypatch.setattr(cls, "load_audio", lambda self, *a, _real=real, **k: (loads.append(is_lowpassed(self)), _real(self, *a, **k))[1])
    strat = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), return_audio=True, gpu_resample=True)
    got_f, got_l, got_a, got_al = strat(batch)
    assert loads and not any(loads)  # no lowpassed cut went through load_audio(): only the plain ones did
    assert stand_ins["resample"] >= 2 and {(SR, 9346), (9346, SR), (SR, 7002), (7002, SR), (SR, 15998), (15998, SR), (SR, 8000), (8000, SR)} <= stand_ins["ratios"]
    assert torch.equal(got_l, want_l) and torch.equal(got_al, want_al)
    got_f, got_a = got_f.numpy().astype(np.float64), got_a.numpy()
    worst = {}
    for i, cut in enumerate(batch):
        n, t = int(want_al[i]), int(want_l[i])
        w = want_f[i, :t].numpy().astype(np.float64)
        rel, mx = float(np.linalg.norm(got_f[i, :t] - w) / np.linalg.norm(w)), float(np.abs(got_f[i, :t] - w).max())
        assert rel <= REL_TOL and mx <= ABS_TOL, (i, cut.id, rel, mx)
        d = float(np.abs(got_a[i, :n] - want_a[i, :n].numpy()).max())
        assert d <= AUDIO_TOL, (i, cut.id, d)
        if labelled[i][0] is not None:
            worst[labelled[i][0]] = max(worst.get(labelled[i][0], 0.0), d)
    print("max |audio - load_audio()| per group:", {g: "%.2e" % v for g, v in worst.items()})
    assert set(worst) == set(groups) and worst["band"] <= 1e-5  # (the bare bracket: about 2e-7 expected; anything above 1e-5 needs an explanation)
    # with the flag off every lowpassed cut is loaded the reference's way: its audio is the reference's, bit for bit
    off = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), return_audio=True, gpu_resample=True, gpu_level=False)
    a_off = off(CutSet.from_cuts(groups["band"][:2]))[2].numpy()
    for j in range(2):
        n = int(want_al[j])
        assert np.array_equal(a_off[j, :n], want_a[j, :n].numpy())


def test_a_leading_resample_over_the_threshold_is_taken_where_the_strategies_ask_for_it(env, tmp_path, stand_ins, monkeypatch):
    """``cuts.resample(16000)`` over a recording at 11130 Hz: 1113 : 1600, a bank of 1.8 M floats.  ``parse_chain`` keeps refusing it with
    its default arguments; with ``bankless=True`` -- what the reader and ``deferred_mix`` pass -- it is taken, alone, in
    front of a ``Speed`` and of a band bracket, and as the track of a mix; what no kernel serves stays refused."""
    from lhotse import CutSet, MonoCut, Recording
    from lhotse.audio import AudioSource
    from lhotse.dataset.input_strategies import OnTheFlyFeatures
    from lhotse.features.kaldi.extractors import Fbank
    from lhotse.utils import fastcopy
    from oracle.driver_corpus import write_wav

    import lhotse_amd as LA
    import lhotse_amd.input_strategies as IS

    pcm = np.round(np.convolve(np.random.RandomState(5).randn(4015), np.hanning(16) / 4.0, mode="valid") * 4000.0).astype(np.int16)
    write_wav(tmp_path / "odd.wav", pcm, 11130)
    rec = Recording(id="odd", sources=[AudioSource(type="file", channels=[0], source=str(tmp_path / "odd.wav"))], sampling_rate=11130, num_samples=len(pcm),
                    duration=len(pcm) / 11130)
    odd = MonoCut(id="odd", start=0, duration=rec.duration, channel=0, recording=rec).resample(SR)
    assert IS._sinc_bank_floats(11130, SR) > IS.MAX_RESAMPLE_BANK_FLOATS
    assert IS.parse_chain(odd) is None and IS.parse_chain(odd, gpu_level=False) is None
    assert IS.parse_chain(odd, bankless=True) == IS.parse_chain(odd, gpu_level=False, bankless=True) == IS.Chain(source_rate=11130)
    assert IS.parse_chain(odd, gpu_resample=False, bankless=True) is None
    assert IS.parse_chain(odd.perturb_speed(1.1), bankless=True) == IS.Chain(11130, 1.1)
    assert _level_chain(IS, lowpass(odd, 4673)) == (11130, 1.0, None, (band(4673), None))
    assert _level_chain(IS, odd.perturb_volume(0.5))[:3] == (11130, 1.0, None)
    tracks = IS.deferred_mix(odd.pad(duration=odd.duration + 0.1), gpu_resample=True)
    assert tracks is not None and tracks[0].chain == IS.Chain(source_rate=11130)
    up = fastcopy(odd, recording=fastcopy(odd.recording, transforms=[{"name": "Resample", "kwargs": {"source_sampling_rate": 2001, "target_sampling_rate": SR}}]))
    assert IS.parse_chain(up, bankless=True) == IS.Chain(source_rate=2001)  # 2001 -> 16000 is served (W = 16); the other direction is not (W = 100):
    down = fastcopy(odd, recording=fastcopy(odd.recording, sampling_rate=2001, transforms=[{"name": "Resample", "kwargs": {"source_sampling_rate": SR, "target_sampling_rate": 2001}}]))
    assert IS.parse_chain(down, bankless=True) is None
    batch = CutSet.from_cuts([odd, env[1], lowpass(odd, 3501), odd.perturb_speed(0.9)])
    want_f, want_l, want_a, want_al = OnTheFlyFeatures(Fbank(), return_audio=True)(batch)
    loads = []
    real = MonoCut.load_audio
    monkeypatch.setattr(MonoCut, "load_audio", lambda self, *a, **k: (loads.append(bool(self.recording.transforms)), real(self, *a, **k))[1])
    got_f, got_l, got_a, got_al = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), return_audio=True, gpu_resample=True)(batch)
    assert loads == [False] and (11130, SR) in stand_ins["ratios"]  # only the plain cut was loaded the reference's way
    assert torch.equal(got_l, want_l) and torch.equal(got_al, want_al)
    for i in range(len(batch)):
        n, t = int(want_al[i]), int(want_l[i])
        d = float(np.abs(got_a[i, :n].numpy() - want_a[i, :n].numpy()).max())
        w = want_f[i, :t].numpy().astype(np.float64)
        rel = float(np.linalg.norm(got_f[i, :t].numpy() - w) / np.linalg.norm(w))
        print(i, "max |audio - load_audio()|", d, "features rel-L2", rel)
        assert d <= AUDIO_TOL and rel <= REL_TOL, (i, d, rel)
