"""CPU: the reverberation rule and its lhotse binding against the REAL lhotse (authoring container; the golden reload runs anywhere).

  * tests/_reverb_ref.py (the contract of hipfeat_reverb_*) against the committed ``load_audio()`` goldens: its float64 form is the stored
    truth, the reference lies at its stored distance from it, the device's summation order keeps the audio bars and ONE serial float32
    chain does not;
  * ``parse_chain`` / ``deferred_mix`` accept the four transform lists and refuse the rest;
  * ``HipReverbWithImpulseResponse`` round-trips through the reference's dict form;
  * HipOnTheFlyFeatures with CPU stand-ins for the device (plan, resampler, reverb, mixer) returns what OnTheFlyFeatures(Fbank()) returns
    on a mini-batch of the three-transform recipe, WITHOUT a ReverbWithImpulseResponse call on the CPU for the eligible cuts."""
import random

import numpy as np
import pytest
import torch

import _reverb_ref as R
from _reverb_golden import GROUPS, corpus_files, exact_audio, load_reverb_goldens, rir_samples, tracks_of


@pytest.fixture(scope="module")
def goldens():
    return load_reverb_goldens()


def test_goldens_reload_and_the_rule_reproduces_the_stored_truth(tmp_path, goldens):
    arrays, meta = goldens
    paths = corpus_files(tmp_path, meta)
    assert set(meta["groups"]) == set(GROUPS) and {"mixed", "reverb", "speed", "plain"} <= set(meta["k2_kinds"])
    taps = {k: len(arrays[f"rir/{k}"]) for k in meta["rirs"]}
    assert sorted(taps.values()) == [257, 3001, 4000, 8003]
    peaks = {k: int(np.argmax(arrays[f"rir/{k}"])) for k in taps}
    assert 0 in peaks.values() and any(peaks[k] == taps[k] - 1 for k in taps)  # a peak at tap 0 and one at the last tap
    n_audio = 0
    for group, entries in meta["groups"].items():
        for i, e in enumerate(entries):
            f = arrays[f"{group}/{i}/feats"]
            assert f.dtype == np.float32 and f.shape[1] == 80 and abs(f.shape[0] - e["want"] / 160) <= 1
            if not e["audio"]:
                continue
            row, audio, truth = e["tracks"][0], arrays[f"{group}/{i}/audio"], exact_audio(arrays, group, i)
            assert len(e["tracks"]) == 1 and len(audio) == e["want"]
            d = R.distances(audio, truth)
            assert abs(d[0] - e["reference_rel_l2"]) <= 1e-9 and abs(d[1] - e["reference_max_abs"]) <= 1e-9 * max(1.0, np.abs(truth).max())
            if row["factor"] != 1.0:
                continue  # (the truth was formed over the reference's resampled samples, which are not stored)
            x = tracks_of(e, paths, arrays)[0][0]
            hs, shift = R.scale_and_shift(rir_samples(arrays, row["reverb"]))
            norm = row["reverb"]["normalize"]
            mine = R.exact(x, hs, shift, norm)
            # the stored truth is this float64 form (kept as a float32 difference from the audio: 2^-24 of that difference is lost)
            assert np.abs(mine - truth).max() <= 2.0 ** -23 * np.abs(mine - audio).max() + 1e-15
            # rounded to float32 it is nearer to the truth than the reference is, and within the reference's distance of the reference
            assert R.distances(mine.astype(np.float32), truth)[0] <= e["reference_rel_l2"]
            assert np.abs(mine.astype(np.float32).astype(np.float64) - audio).max() <= e["reference_max_abs"] + 2.0 ** -24 * np.abs(truth).max()
            bar_rel, bar_max = R.bars(e["reference_rel_l2"], e["reference_max_abs"], truth)
            m = R.distances(R.chunked32(x, hs, shift, norm), truth)
            s = R.distances(R.chunked32(x, hs, shift, norm, chunk=None), truth)
            assert m[0] <= bar_rel and m[1] <= bar_max, (group, i, m)
            assert s[0] > bar_rel or s[1] > bar_max, (group, i, s)
            assert R.distances(R.fft32(x, hs, shift, norm), truth)[0] <= 2 * e["reference_rel_l2"]  # the FFT restatement is the CPU path's arithmetic
            n_audio += 1
    assert n_audio >= 5


@pytest.mark.parametrize("n,taps", [(300, 257), (2049, 300), (600, 513)])
def test_integer_valued_items_come_out_the_same_in_every_summation_order(n, taps):
    """The yardstick of the large GPU batches (tests/test_gpu_reverb.py): for integer-valued items the float64 form, the device's order and one
    serial float32 chain are the same numbers, and the normalised output is float32(exact) x float32(gain), one rounded multiply."""
    rng = np.random.default_rng(1000 * n + taps)
    for shift in sorted({0, taps // 2, taps - 1}):
        x, hs, s, _ = R.integer_item(rng, n, taps, shift, False)
        assert s == shift and x.dtype == hs.dtype == np.float32 and np.abs(x).max() == 15 and hs[shift] == np.float32(16 * 2.0 ** -15)
        want = R.integer_expected(x, hs, shift, False)
        assert want.dtype == np.float32 and np.array_equal(want.astype(np.float64), R.exact(x, hs, shift, False))
        assert np.array_equal(want, R.chunked32(x, hs, shift, False))
        assert np.array_equal(want, R.chunked32(x, hs, shift, False, chunk=None))
        scaled = R.integer_expected(x, hs, shift, True)
        gain = np.float32(np.sqrt((np.sum(x.astype(np.float64) ** 2) / n) / (np.sum(want.astype(np.float64) ** 2) / n)))
        assert np.array_equal(scaled, want * gain) and not np.array_equal(scaled, want)
        assert np.array_equal(scaled, R.chunked32(x, hs, shift, True))
        # ... and it is the rule: within one float32 rounding of the float64 form scaled by the float64 gain
        assert np.abs(scaled - R.exact(x, hs, shift, True)).max() <= 2.0 ** -23 * np.abs(scaled).max()


def test_integer_items_refuse_sizes_that_would_not_be_exact():
    R.assert_integer_exact(100000, 300)
    with pytest.raises(AssertionError):
        R.assert_integer_exact(10, 2 ** 24 // (15 * 16) + 1)  # 15 * 16 * L >= 2^24
    with pytest.raises(AssertionError):
        R.assert_integer_exact(2 ** 31, 300)                  # sum(y^2) past 2^53 units
    with pytest.raises(AssertionError):
        R.integer_expected(np.full(8, 0.5, np.float32), np.ones(1, np.float32) * R.SCALE, 0)


# ---- under the real lhotse ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(tmp_path_factory):
    import wave

    from _dropin_support import import_lhotse, install_wave_backend, write_cutset

    import_lhotse()
    from lhotse import Recording
    from lhotse.audio import AudioSource
    from lhotse.audio.backend import set_current_audio_backend

    prev = install_wave_backend()
    d = tmp_path_factory.mktemp("rvbwav")
    (d / "s").mkdir(), (d / "n").mkdir()
    speech = write_cutset(d / "s", [16000, 12345, 8000, 5000, 20480, 9999, 7000], seed=1)
    noise = write_cutset(d / "n", [24000, 7000], seed=2)
    rirs = []
    rs = np.random.RandomState(4)
    for k, (taps, peak, ch) in enumerate([(300, 0, 1), (1200, 40, 1), (2000, 7, 2)]):
        h = rs.randn(taps, ch) * np.exp(-5.0 * np.arange(taps) / taps)[:, None] * 0.1
        h[peak] = 1.0
        p = d / f"rir{k}.wav"
        with wave.open(str(p), "wb") as f:
            f.setnchannels(ch), f.setsampwidth(2), f.setframerate(16000)
            f.writeframes(np.round(h * 20000).astype(np.int16).tobytes())
        rirs.append(Recording(id=f"rir{k}", sources=[AudioSource(type="file", channels=list(range(ch)), source=str(p))], sampling_rate=16000,
                              num_samples=taps, duration=taps / 16000))
    yield speech, noise, rirs
    set_current_audio_backend(prev)


@pytest.mark.reference
def test_classifier_accepts_the_four_transform_lists_and_refuses_the_rest(env):
    import lhotse_amd.input_strategies as IS
    from lhotse.utils import fastcopy

    speech, noise, rirs = env
    s, n = list(speech)[0], list(noise)[1]
    def speed_and_reverb(cut, **kw):  # the rule with the resampling and level routes off: [Speed]? [Reverb]? is all it serves
        ch = IS.parse_chain(cut, gpu_resample=False, gpu_level=False, **kw)
        assert ch is None or (ch.source_rate, ch.pre, ch.post) == (None, None, None)
        return None if ch is None else (ch.factor, ch.reverb)

    assert speed_and_reverb(s) == (1.0, None) and not IS.parse_chain(s).pending
    assert speed_and_reverb(s.perturb_speed(1.1)) == (1.1, None)
    f, rv = speed_and_reverb(s.reverb_rir(rirs[0]))
    assert f == 1.0 and rv["rir"].id == "rir0" and rv["normalize_output"] and not rv["early_only"] and rv["rir_channels"] == [0]
    f, rv = speed_and_reverb(s.perturb_speed(0.9).reverb_rir(rirs[1], normalize_output=False, early_only=True))
    assert f == 0.9 and rv["rir"].id == "rir1" and not rv["normalize_output"] and rv["early_only"]
    assert IS.parse_chain(s).reverb is None and IS.parse_chain(s.perturb_speed(1.1)).reverb is None
    assert IS.parse_chain(s.reverb_rir(rirs[0])).factor == 1.0
    # ... the same after the manifest went through its dict form (a cut read back from disk)
    back = type(s).from_dict(s.perturb_speed(0.9).reverb_rir(rirs[2], rir_channels=[1]).to_dict())
    f, rv = speed_and_reverb(back)
    assert f == 0.9 and rv["rir_channels"] == [1]
    ref_rir = rirs[2].to_cut().with_channels([1]).load_audio()[0]
    assert np.array_equal(IS.load_reverb_rir(rv), ref_rir) and IS.load_reverb_rir(rv).dtype == np.float32
    early = IS.load_reverb_rir({**rv, "early_only": True})
    assert len(early) == 800 and np.array_equal(early, ref_rir[:800])
    # a pending Speed in front of a reverb the device serves counts; with the reverb route off such a cut is the reference's
    assert IS.parse_chain(s.perturb_speed(1.1).reverb_rir(rirs[0])).factor == 1.1 and IS.parse_chain(s.reverb_rir(rirs[0])).factor == 1.0
    assert speed_and_reverb(s.perturb_speed(1.1).reverb_rir(rirs[0]), gpu_reverb=False) is None
    # refused: the random generator, several rir_channels, a reverb in front of a Speed, other transforms, gpu_reverb off
    assert speed_and_reverb(s.reverb_rir()) is None
    two = fastcopy(s, recording=s.recording.reverb_rir(rirs[2], rir_channels=[0, 1]))
    assert speed_and_reverb(two) is None
    assert speed_and_reverb(s.reverb_rir(rirs[0]).perturb_speed(1.1)) is None
    assert speed_and_reverb(s.reverb_rir(rirs[0]).perturb_volume(2.0)) is None
    assert speed_and_reverb(s.perturb_volume(2.0).reverb_rir(rirs[0])) is None
    assert speed_and_reverb(s.reverb_rir(rirs[0]).reverb_rir(rirs[1])) is None
    assert speed_and_reverb(s.reverb_rir(rirs[0]), gpu_reverb=False) is None and speed_and_reverb(s.perturb_speed(1.1), gpu_reverb=False) == (1.1, None)
    # mixed cuts: a reverberated track is accepted (its chain carries the reverb), a reverb on the mixed cut itself (mix_first) is not
    tr = IS.deferred_mix(s.perturb_speed(1.1).reverb_rir(rirs[1]).mix(n, snr=15))
    assert [(t.chain.factor, t.chain.reverb is not None) for t in tr] == [(1.1, True), (1.0, False)] and tr[0].chain.reverb["rir"].id == "rir1"
    assert IS.deferred_mix(s.perturb_speed(1.1).reverb_rir(rirs[1]).mix(n, snr=15), gpu_reverb=False) is None
    assert IS.deferred_mix(s.mix(n.reverb_rir(), snr=15)) is None
    own = s.mix(n, snr=15).reverb_rir(rirs[0], mix_first=True)
    assert type(own).__name__ == "MixedCut" and own.transforms and IS.deferred_mix(own) is None
    # the loaded tracks: a reverb where one is pending, the samples in front of every transform
    loaded, _, want = IS._read_tracks(s.reverb_rir(rirs[0]).mix(n, snr=15), IS.deferred_mix(s.reverb_rir(rirs[0]).mix(n, snr=15)))
    assert [t.reverb is not None for t in loaded] == [True, False] and np.array_equal(loaded[0].samples, s.load_audio()[0]) and loaded[0].reverb[1] is True
    assert all((t.cap, t.source_rate, t.levels) == (len(t.samples), None, None) for t in loaded)
    assert np.array_equal(loaded[0].reverb[0], rirs[0].load_audio()[0])
    one = IS._read_one(s.perturb_speed(1.1).reverb_rir(rirs[0]), gpu_speed=True, suppress_errors=False, gpu_mix=True, gpu_reverb=True)
    assert isinstance(one[0], list) and one[0][0].reverb is not None and one[0][0].factor == 1.1 and one[2] == s.perturb_speed(1.1).num_samples
    assert (one[0][0].source_rate, one[0][0].levels) == (None, None)
    assert np.array_equal(one[0][0].samples, IS.read_before_chain(s.perturb_speed(1.1)))
    # gpu_speed off: a [Speed, Reverb] cut takes the reference's path, a [Reverb] cut still goes to the device
    off = IS._read_one(s.perturb_speed(1.1).reverb_rir(rirs[0]), gpu_speed=False, suppress_errors=False, gpu_mix=True, gpu_reverb=True)
    assert isinstance(off[0], torch.Tensor) and off[1] == 1.0
    assert isinstance(IS._read_one(s.reverb_rir(rirs[0]), gpu_speed=False, suppress_errors=False, gpu_mix=False, gpu_reverb=True)[0], list)


@pytest.mark.reference
def test_transform_round_trips_through_the_reference_dict_form(env):
    from lhotse.augmentation import AudioTransform, ReverbWithImpulseResponse

    from lhotse_amd import _lib
    from lhotse_amd.augmentation import HipReverbWithImpulseResponse, load_rir

    _, _, rirs = env
    assert AudioTransform.KNOWN_TRANSFORMS["HipReverbWithImpulseResponse"] is HipReverbWithImpulseResponse
    tf = HipReverbWithImpulseResponse(rir=rirs[2], normalize_output=False, early_only=True, rir_channels=[1])
    d = tf.to_dict()
    assert d["name"] == "HipReverbWithImpulseResponse" and d["kwargs"]["rir"] == rirs[2].to_dict() and d["kwargs"]["rir_channels"] == [1]
    back = AudioTransform.from_dict(d)
    assert isinstance(back, HipReverbWithImpulseResponse) and back.rir == rirs[2] and (back.normalize_output, back.early_only, back.rir_channels) == (False, True, [1])
    assert back.to_dict() == d
    # the reference's own dict (its fields) builds the device transform, and the other way round
    ref = ReverbWithImpulseResponse(rir=rirs[1], early_only=True)
    mine = HipReverbWithImpulseResponse(**ref.to_dict()["kwargs"])
    assert mine.rir == rirs[1] and mine.early_only and mine.rir_channels == [0]
    kw = {k: v for k, v in mine.to_dict()["kwargs"].items() if k != "device"}
    assert ReverbWithImpulseResponse(**kw).to_dict() == ref.to_dict()
    assert np.array_equal(load_rir(mine.rir, mine.rir_channels, True)[0], rirs[1].to_cut().truncate(duration=0.05).load_audio()[0])
    with pytest.raises(_lib.HipFeatError) as e:
        HipReverbWithImpulseResponse(**ReverbWithImpulseResponse(rir_generator={"sr": 16000}).to_dict()["kwargs"])
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        HipReverbWithImpulseResponse(rir=rirs[0], rir_channels=[1])


@pytest.mark.reference
def test_strategy_with_cpu_stand_ins_equals_on_the_fly_features(env, monkeypatch):
    import lhotse_amd as LA
    import lhotse_amd.extractors as E
    import lhotse_amd.input_strategies as IS
    from _dropin_support import make_cpu_plan
    from _mix_ref import mix_in_arena_cpu
    from lhotse.augmentation import ReverbWithImpulseResponse as RefReverb
    from lhotse.cut import MixedCut
    from lhotse.dataset.cut_transforms import CutMix, PerturbSpeed, ReverbWithImpulseResponse
    from lhotse.dataset.input_strategies import OnTheFlyFeatures
    from lhotse.features.kaldi.extractors import Fbank
    from oracle import resample_ref

    from lhotse_amd.augmentation import perturbed_layout

    speech, noise, rirs = env
    monkeypatch.setattr(E, "_Plan", make_cpu_plan())
    count = {"reverb_cpu": 0, "reverb_items": 0}

    def cpu_perturb(arena, offsets, lengths, factors, sr, tail_start):
        po, pl, _ = perturbed_layout(offsets, lengths, factors, sr, tail_start)
        for i, f in enumerate(factors):
            if f != 1.0:
                y = resample_ref.resample(arena[int(offsets[i]) : int(offsets[i] + lengths[i])].numpy(), round(sr * f), sr).astype(np.float32)
                assert len(y) == pl[i]
                arena[int(po[i]) : int(po[i]) + len(y)] = torch.from_numpy(y)
        return po, pl

    def cpu_reverb(arena, so, sl, ro, rl, shifts, norm, tail_start):
        """hipfeat_reverb_plan's placement + the rule of tests/_reverb_ref.py"""
        assert tail_start % 4 == 0
        a, offs, tail = arena.numpy(), [], int(tail_start)
        for s, n, r, taps, sh, nm in zip(so, sl, ro, rl, shifts, norm):
            assert s + n <= tail_start and r + taps <= tail_start and int(np.argmax(a[r : r + taps])) == sh
            a[tail : tail + n] = R.chunked32(a[s : s + n], a[r : r + taps], int(sh), bool(nm))
            offs.append(tail)
            tail += (int(n) + 3) & ~3
            count["reverb_items"] += 1
        assert tail <= len(a)
        return np.asarray(offs, dtype=np.int64)

    monkeypatch.setattr(IS, "_perturb_in_arena", cpu_perturb)
    monkeypatch.setattr(IS, "_reverb_in_arena", cpu_reverb)
    monkeypatch.setattr(IS, "_mix_in_arena", mix_in_arena_cpu)
    real = RefReverb.__call__
    monkeypatch.setattr(RefReverb, "__call__", lambda self, *a, **k: (count.__setitem__("reverb_cpu", count["reverb_cpu"] + 1), real(self, *a, **k))[1])

    mono_rirs = rirs[:2]
    cuts = PerturbSpeed(factors=[0.9, 1.1], p=2 / 3, randgen=random.Random(23))(speech)
    cuts = ReverbWithImpulseResponse(mono_rirs, p=0.5, randgen=random.Random(24))(cuts)
    cuts = CutMix(noise, snr=(10, 20), p=0.5, pad_to_longest=False, random_mix_offset=True, seed=25)(cuts)

    def has_reverb(c):
        return any(IS._transform_name(t) == "ReverbWithImpulseResponse" for t in (c.recording.transforms or []))

    leaves = [t.cut for c in cuts if isinstance(c, MixedCut) for t in c.tracks] + [c for c in cuts if not isinstance(c, MixedCut)]
    n_rvb = sum(has_reverb(c) for c in leaves if type(c).__name__ != "PaddingCut")
    kinds = {("mixed" if isinstance(c, MixedCut) else "reverb" if has_reverb(c) else "speed" if c.recording.transforms else "plain") for c in cuts}
    assert kinds == {"mixed", "reverb", "speed", "plain"} and n_rvb >= 2
    assert any(isinstance(c, MixedCut) and has_reverb(c.tracks[0].cut) for c in cuts)  # a reverberated track under a noise
    ref_f, ref_l, ref_a, ref_al = OnTheFlyFeatures(Fbank(), return_audio=True)(cuts)
    assert count["reverb_cpu"] == n_rvb
    hip = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), return_audio=True, num_workers=2)
    f, l, a, al = hip(cuts)
    assert count["reverb_cpu"] == n_rvb and count["reverb_items"] == n_rvb  # ZERO reference-path reverbs of the eligible cuts
    assert torch.equal(l, ref_l) and torch.equal(al, ref_al) and f.shape == ref_f.shape and a.shape == ref_a.shape
    # the resampler's 1e-5 passes through the convolution times gain x sum|hs| (about 3 here); float32 rounding of both forms besides
    assert torch.allclose(a, ref_a, atol=1e-4)
    assert torch.allclose(f, ref_f, atol=5e-3)
    # switched off: the reference's own path, cut by cut
    f2, l2 = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), gpu_reverb=False)(cuts)
    assert count["reverb_cpu"] == 2 * n_rvb and count["reverb_items"] == n_rvb and torch.equal(l2, ref_l) and torch.allclose(f2, ref_f, atol=5e-3)
    # wave_transforms: by default the reverb stays where the reference does it; the explicit contradiction raises
    f3, l3 = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), wave_transforms=[lambda x: x])(cuts)
    assert count["reverb_cpu"] == 3 * n_rvb and count["reverb_items"] == n_rvb and torch.equal(l3, ref_l)
    with pytest.raises(ValueError, match="gpu_reverb=True was requested together with wave_transforms"):
        LA.HipOnTheFlyFeatures(LA.HipFbank(), wave_transforms=[lambda x: x], gpu_reverb=True, gpu_speed_perturb=False, gpu_mix=False)(cuts)
