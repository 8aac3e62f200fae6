"""CPU: the mixing rule and its lhotse binding against the REAL lhotse (authoring container; the golden reload runs anywhere).

  * tests/_mix_ref.py (the contract of hipfeat_mix_*) equals MixedCut.load_audio bit for bit when it takes the energies the way the
    reference does -- on the committed goldens and on freshly built cuts;
  * deferred_mix accepts / refuses each case of the fallback list;
  * HipOnTheFlyFeatures with CPU stand-ins for the device (plan, resampler, mixer) returns what OnTheFlyFeatures(Fbank()) returns on a
    mini-batch of mixed, speed-only and plain cuts, WITHOUT a MixedCut.load_audio call for the eligible cuts."""
import random

import numpy as np
import pytest
import torch

from _mix_golden import corpus_files, exact_mix, load_mix_goldens, ref_tracks_of
from _mix_ref import mix_in_arena_cpu, mix_tracks


@pytest.fixture(scope="module")
def goldens():
    return load_mix_goldens()


def test_goldens_reload_and_the_rule_reproduces_the_stored_audio(tmp_path, goldens):
    arrays, meta = goldens
    paths = corpus_files(tmp_path, meta)
    assert set(meta["groups"]) == {"cutmix", "speed_cutmix", "pad", "fixed", "k2"} and {"mixed", "speed", "plain"} <= set(meta["k2_kinds"])
    n_audio = n_exact = 0
    for group, entries in meta["groups"].items():
        for i, e in enumerate(entries):
            f = arrays[f"{group}/{i}/feats"]
            assert f.dtype == np.float32 and f.shape[1] == 80 and abs(f.shape[0] - e["want"] / 160) <= 1
            if e["audio"] and all(r["factor"] == 1.0 for r in e["tracks"]):
                tracks, ref = ref_tracks_of(e, paths)
                audio = arrays[f"{group}/{i}/audio"]
                assert np.array_equal(mix_tracks(tracks, ref, e["want"], energy="float32"), audio), (group, i)  # bit for bit
                n_audio += 1
                if e["exact"]:
                    m64 = exact_mix(arrays, group, i)
                    assert np.allclose(m64, mix_tracks(tracks, ref, e["want"], accumulate=np.float64), rtol=0, atol=1e-12)
                    d = np.linalg.norm(audio - m64) / np.linalg.norm(m64)
                    assert abs(d - e["reference_rel_l2"]) <= 1e-12
                    # what the device computes (float64 energies, float32 gains and sums) keeps the bar of the GPU test
                    dev = np.linalg.norm(mix_tracks(tracks, ref, e["want"]) - m64) / np.linalg.norm(m64)
                    assert dev <= 2 * e["reference_rel_l2"] + 2.0 ** -24
                    n_exact += 1
    assert n_audio >= 8 and n_exact >= 8


# ---- under the real lhotse ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from _dropin_support import import_lhotse, install_wave_backend, write_cutset

    import_lhotse()
    from lhotse.audio.backend import set_current_audio_backend

    prev = install_wave_backend()
    d = tmp_path_factory.mktemp("mixwav")
    (d / "s").mkdir(), (d / "n").mkdir()
    speech = write_cutset(d / "s", [16000, 12345, 8000, 5000, 20480, 9999], seed=1)
    noise = write_cutset(d / "n", [24000, 7000], seed=2)
    yield speech, noise
    set_current_audio_backend(prev)


def _tracks_for_rule(cut, IS):
    tracks = IS.deferred_mix(cut)
    assert tracks is not None
    loaded, _, want = IS._read_tracks(cut, tracks)
    return [(t.samples, t.offset, t.snr) for t in loaded], next((k for k, t in enumerate(loaded) if t.is_ref), -1), want


@pytest.mark.reference
def test_rule_equals_load_audio_on_fresh_cuts(env):
    import lhotse_amd.input_strategies as IS
    from lhotse.dataset.cut_transforms import CutMix

    speech, noise = env
    cuts = list(CutMix(noise, snr=(10, 20), p=1.0, pad_to_longest=True, random_mix_offset=True, seed=3)(speech))
    cuts += [c.pad(duration=1.6, direction=d) for c in list(speech)[:3] for d in ("left", "right", "both")]
    cuts += [c.pad(duration=1.4, direction="both").mix(list(noise)[1], snr=15) for c in list(speech)[1:4]]
    cuts += [list(speech)[0].mix(list(noise)[1], snr=None, offset_other_by=0.0301875)]
    for cut in cuts:
        tracks, ref, want = _tracks_for_rule(cut, IS)
        assert np.array_equal(mix_tracks(tracks, ref, want, energy="float32"), cut.load_audio()[0]), cut


@pytest.mark.reference
def test_deferred_mix_accepts_and_refuses(env):
    import lhotse_amd.input_strategies as IS
    from lhotse import MultiCut
    from lhotse.cut import MixedCut, MixTrack
    from lhotse.utils import fastcopy

    speech, noise = env
    s, n = list(speech)[0], list(noise)[1]
    ok = s.mix(n, snr=15)
    tr = IS.deferred_mix(ok)
    assert [(t.chain.factor, t.offset, t.snr, t.is_ref) for t in tr] == [(1.0, 0, None, True), (1.0, 0, 15, False)]
    assert [t.chain and t.chain.factor for t in IS.deferred_mix(s.pad(duration=1.5))] == [1.0, None]  # a PaddingCut track
    assert [t.chain.factor for t in IS.deferred_mix(s.perturb_speed(1.1).mix(n, snr=15))] == [1.1, 1.0]  # exactly one Speed
    assert IS.deferred_mix(s) is None  # not a mixed cut
    assert IS.deferred_mix(s.perturb_volume(2.0).mix(n, snr=15)) is None  # a transform other than Speed
    assert IS.deferred_mix(s.perturb_speed(1.1).perturb_volume(2.0).mix(n, snr=15)) is None  # several transforms
    assert IS.deferred_mix(ok.perturb_volume(2.0)) is None  # (the volume lands on the tracks' recordings)
    assert IS.deferred_mix(s.mix(ok, snr=10)) is not None and all(type(t.cut).__name__ == "MonoCut" for t in IS.deferred_mix(s.mix(ok, snr=10)))  # mix() flattens
    assert IS.deferred_mix(MixedCut(id="nest", tracks=[MixTrack(cut=s, type="MonoCut"), MixTrack(cut=ok, type="MixedCut", snr=10)])) is None  # a nested mixed cut
    assert IS.deferred_mix(fastcopy(ok, transforms=[{"name": "Volume", "kwargs": {"factor": 2.0}}])) is None  # transforms of its own
    multi = MultiCut(id="m", start=0, duration=s.duration, channel=[0], recording=s.recording)
    assert IS.deferred_mix(MixedCut(id="x", tracks=[MixTrack(cut=multi, type="MultiCut"), MixTrack(cut=n, type="MonoCut", snr=15)])) is None  # MultiCut track
    # a first track with an SNR while the reference track is another one
    assert IS.deferred_mix(MixedCut(id="y", tracks=[MixTrack(cut=n, type="MonoCut", snr=10), MixTrack(cut=s, type="MonoCut")])) is None
    # a muted reference track / muted tracks are dropped
    muted = MixedCut(id="z", tracks=[MixTrack(cut=s, type="MonoCut"), MixTrack(cut=n, type="MonoCut", snr=15, mute=True)])
    assert len(IS.deferred_mix(muted)) == 1
    assert IS.deferred_mix(MixedCut(id="w", tracks=[MixTrack(cut=s, type="MonoCut", mute=True), MixTrack(cut=n, type="MonoCut", snr=15)])) is None
    # an explicit SNR reference flag on a padding track (E_ref = 0 in the reference: all gains 1)
    from lhotse.cut import PaddingCut

    pad = PaddingCut(id="p", duration=0.1, sampling_rate=16000, feat_value=0, num_samples=1600)
    assert IS.deferred_mix(MixedCut(id="pr", tracks=[MixTrack(cut=pad, type="PaddingCut", is_snr_reference=True), MixTrack(cut=s, type="MonoCut", snr=10, offset=0.1)])) is None
    # video, on the first track and on a later one
    from lhotse.audio import AudioSource
    from lhotse.audio.recording import VideoInfo

    def with_video(c):
        src = c.recording.sources[0]
        v = AudioSource(type=src.type, channels=src.channels, source=src.source, video=VideoInfo(fps=25.0, num_frames=25, height=8, width=8))
        return fastcopy(c, recording=fastcopy(c.recording, sources=[v]))

    assert with_video(s).has_video
    assert IS.deferred_mix(MixedCut(id="vid0", tracks=[MixTrack(cut=with_video(s), type="MonoCut"), MixTrack(cut=n, type="MonoCut", snr=15)])) is None
    assert IS.deferred_mix(MixedCut(id="vid1", tracks=[MixTrack(cut=s, type="MonoCut"), MixTrack(cut=with_video(n), type="MonoCut", snr=15)])) is None
    # a mix that comes out SHORTER than cut.num_samples (0.4 + 100.4 samples round to 0 + 100, their sum to 101): the reference reflect-pads
    sr = 16000
    short = MixedCut(id="short", tracks=[MixTrack(cut=fastcopy(s, duration=50 / sr), type="MonoCut"),
                                         MixTrack(cut=fastcopy(n, duration=100.4 / sr), type="MonoCut", offset=0.4 / sr, snr=10)])
    assert short.num_samples == 101 and short.load_audio().shape == (1, 101) and IS.deferred_mix(short) is None
    # one sample LONGER (0.5 + 100.5 -> 1 + 101 against 101) is truncated on the device ...
    longer = MixedCut(id="long", tracks=[MixTrack(cut=fastcopy(s, duration=50 / sr), type="MonoCut"),
                                         MixTrack(cut=fastcopy(n, duration=100.5 / sr), type="MonoCut", offset=0.5 / sr, snr=10)])
    assert longer.num_samples == 101 and [t.offset for t in IS.deferred_mix(longer)] == [0, 1]
    tracks, ref, want = _tracks_for_rule(longer, IS)
    assert want == 101 and np.array_equal(mix_tracks(tracks, ref, want, energy="float32"), longer.load_audio()[0])
    # ... unless that is lhotse's tolerance or more (the reference then refuses the cut itself)
    from lhotse.audio.utils import get_audio_duration_mismatch_tolerance, set_audio_duration_mismatch_tolerance

    tol = get_audio_duration_mismatch_tolerance()
    set_audio_duration_mismatch_tolerance(1 / sr)
    try:
        assert IS.deferred_mix(longer) is None
        with pytest.raises(AssertionError):
            longer.load_audio()
    finally:
        set_audio_duration_mismatch_tolerance(tol)
    assert IS.deferred_mix(longer) is not None
    # another sampling rate in a track
    assert IS.deferred_mix(MixedCut(id="v", tracks=[MixTrack(cut=s, type="MonoCut"), MixTrack(cut=n.resample(8000), type="MonoCut", snr=15)])) is None


@pytest.mark.reference
def test_strategy_with_cpu_stand_ins_equals_on_the_fly_features(env, monkeypatch):
    import lhotse_amd as LA
    import lhotse_amd.extractors as E
    import lhotse_amd.input_strategies as IS
    from _dropin_support import make_cpu_plan
    from lhotse import CutSet
    from lhotse.cut import MixedCut
    from lhotse.dataset.cut_transforms import CutMix, PerturbSpeed
    from lhotse.dataset.input_strategies import OnTheFlyFeatures
    from lhotse.features.kaldi.extractors import Fbank
    from oracle import resample_ref

    speech, noise = env
    monkeypatch.setattr(E, "_Plan", make_cpu_plan())

    def cpu_perturb(arena, offsets, lengths, factors, sr, tail_start):
        offsets, lengths = np.asarray(offsets, dtype=np.int64).copy(), np.asarray(lengths, dtype=np.int64).copy()
        tail = (int(tail_start) + 3) & ~3
        for i, f in enumerate(factors):
            if f == 1.0:
                continue
            x = arena[int(offsets[i]) : int(offsets[i] + lengths[i])].numpy()
            y = resample_ref.resample(x, round(sr * f), sr).astype(np.float32)
            arena[tail : tail + len(y)] = torch.from_numpy(y)
            offsets[i], lengths[i] = tail, len(y)
            tail = (tail + len(y) + 3) & ~3
        return offsets, lengths

    monkeypatch.setattr(IS, "_perturb_in_arena", cpu_perturb)
    monkeypatch.setattr(IS, "_mix_in_arena", mix_in_arena_cpu)
    loads = {"mixed": 0}
    real = MixedCut.load_audio
    monkeypatch.setattr(MixedCut, "load_audio", lambda self, *a, **k: (loads.__setitem__("mixed", loads["mixed"] + 1), real(self, *a, **k))[1])

    cuts = PerturbSpeed(factors=[0.9, 1.1], p=2 / 3, randgen=random.Random(1))(speech)
    cuts = CutMix(noise, snr=(10, 20), p=0.5, pad_to_longest=False, random_mix_offset=True, seed=13)(cuts)
    kinds = {("mixed" if isinstance(c, MixedCut) else "speed" if c.recording.transforms else "plain") for c in cuts}
    assert kinds == {"mixed", "speed", "plain"}
    n_mixed = sum(isinstance(c, MixedCut) for c in cuts)
    ref_f, ref_l, ref_a, ref_al = OnTheFlyFeatures(Fbank(), return_audio=True)(cuts)
    assert loads["mixed"] == n_mixed
    hip = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), return_audio=True, num_workers=2)
    f, l, a, al = hip(cuts)
    assert loads["mixed"] == n_mixed  # ZERO reference-path loads of the eligible mixed cuts
    assert torch.equal(l, ref_l) and torch.equal(al, ref_al) and f.shape == ref_f.shape and a.shape == ref_a.shape
    assert torch.allclose(a, ref_a, atol=1e-5)  # the resampler's summation order and the float64 energies
    assert torch.allclose(f, ref_f, atol=5e-3)
    # switched off: the reference's own path, cut by cut
    f2, l2 = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), gpu_mix=False)(cuts)
    assert loads["mixed"] == 2 * n_mixed and torch.equal(l2, ref_l) and torch.allclose(f2, ref_f, atol=5e-3)
    # wave_transforms: by default the mix stays where the reference does it; the explicit contradiction raises
    f3, l3 = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), wave_transforms=[lambda x: x])(cuts)
    assert loads["mixed"] == 3 * n_mixed and torch.equal(l3, ref_l)
    with pytest.raises(ValueError, match="gpu_mix=True was requested together with wave_transforms"):
        LA.HipOnTheFlyFeatures(LA.HipFbank(), wave_transforms=[lambda x: x], gpu_mix=True, gpu_speed_perturb=False)(cuts)
    # fault_tolerant: a mixed cut with a track that cannot be read is dropped, the tuple carries the surviving cuts
    from lhotse.audio import AudioSource
    from lhotse.audio.backend import get_current_audio_backend
    from lhotse.audio.utils import AudioLoadingError
    from lhotse.utils import fastcopy

    backend = get_current_audio_backend()
    inner = backend.read_audio

    def failing_read(path_or_fd, *a, **k):  # (what lhotse's own backends raise for a file they cannot decode)
        if "nonexistent" in str(path_or_fd):
            raise AudioLoadingError(f"cannot read {path_or_fd}")
        return inner(path_or_fd, *a, **k)

    monkeypatch.setattr(backend, "read_audio", failing_read, raising=False)
    broken = list(noise)[0]
    broken = fastcopy(broken, recording=fastcopy(broken.recording, sources=[AudioSource(type="file", channels=[0], source="/nonexistent/x.wav")]))
    bad = list(speech)[0].mix(broken, snr=10)
    with_bad = CutSet.from_cuts(list(cuts) + [bad])
    out = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), fault_tolerant=True)(with_bad)
    assert len(out) == 3 and [c.id for c in out[2]] == [c.id for c in cuts] and torch.equal(out[1], ref_l)


@pytest.mark.reference
def test_quiet_fallbacks_and_single_track_mixed_cuts_take_the_right_route(env, monkeypatch, tmp_path):
    """The decisions nobody sees from the outside, each on one cut, each with an assertion on the ROUTE: a counted MixedCut.load_audio
    (the reference's path) or a counted device mix."""
    import wave

    import lhotse_amd as LA
    import lhotse_amd.extractors as E
    import lhotse_amd.input_strategies as IS
    from _dropin_support import make_cpu_plan
    from lhotse import CutSet, MonoCut, Recording
    from lhotse.audio import AudioSource
    from lhotse.cut import MixedCut, MixTrack
    from lhotse.dataset.input_strategies import OnTheFlyFeatures
    from lhotse.features.kaldi.extractors import Fbank
    from lhotse.utils import fastcopy
    from oracle import resample_ref

    speech, noise = env
    s, s2, n = list(speech)[0], list(speech)[2], list(noise)[1]
    monkeypatch.setattr(E, "_Plan", make_cpu_plan())
    count = {"load": 0, "mix": 0, "cuts_mixed": 0}

    def cpu_perturb(arena, offsets, lengths, factors, sr, tail_start):
        from lhotse_amd.augmentation import perturbed_layout

        po, pl, _ = perturbed_layout(offsets, lengths, factors, sr, tail_start)
        for i, f in enumerate(factors):
            if f != 1.0:
                y = resample_ref.resample(arena[int(offsets[i]) : int(offsets[i] + lengths[i])].numpy(), round(sr * f), sr).astype(np.float32)
                assert len(y) == pl[i]
                arena[int(po[i]) : int(po[i]) + len(y)] = torch.from_numpy(y)
        return po, pl

    def counted_mix(arena, first, *a):
        count["mix"] += 1
        count["cuts_mixed"] += len(first) - 1
        return mix_in_arena_cpu(arena, first, *a)

    monkeypatch.setattr(IS, "_perturb_in_arena", cpu_perturb)
    monkeypatch.setattr(IS, "_mix_in_arena", counted_mix)
    real = MixedCut.load_audio
    monkeypatch.setattr(MixedCut, "load_audio", lambda self, *a, **k: (count.__setitem__("load", count["load"] + 1), real(self, *a, **k))[1])

    def hip(**kw):
        return LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), **kw)

    def run(cuts, **kw):
        """-> (MixedCut.load_audio calls, device mix calls, cuts mixed there) of ONE strategy call; the result equals the reference's."""
        cuts = CutSet.from_cuts(cuts)
        ref_f, ref_l = OnTheFlyFeatures(Fbank())(cuts, **kw)
        before = dict(count)
        f, l = hip()(cuts, **kw)
        assert torch.equal(l, ref_l) and torch.allclose(f, ref_f, atol=5e-3)
        return tuple(count[k] - before[k] for k in ("load", "mix", "cuts_mixed"))

    ok = s.mix(n, snr=15)
    assert run([ok, s2]) == (0, 1, 1)  # the yardstick: an eligible cut is mixed on the device, no reference-path load

    # (1) a mixed cut with ONE audible, unscaled track at offset 0 (its noise track muted) and nothing else to mix: no mix call at all
    muted = MixedCut(id="muted", tracks=[MixTrack(cut=s, type="MonoCut"), MixTrack(cut=fastcopy(n, duration=0.3), type="MonoCut", snr=15, mute=True)])
    assert len(IS.deferred_mix(muted)) == 1
    assert run([muted, s2]) == (0, 0, 0)
    assert run([muted.perturb_speed(1.1), s2]) == (0, 0, 0)  # ... also behind a device Speed
    assert run([muted, ok, s2]) == (0, 1, 1)  # ... and next to a really mixed cut only that one is mixed

    # (2) a perturbed TRACK that would need reflect-padding (its file is five samples shorter than the manifest states): deferred_mix
    # accepts the cut, the reader finds the short track, the cut takes cut.load_audio()
    N = 16000
    path = tmp_path / "shortfile.wav"
    with wave.open(str(path), "wb") as fh:
        fh.setnchannels(1), fh.setsampwidth(2), fh.setframerate(16000)
        fh.writeframes(((np.random.RandomState(3).rand(N - 5) - 0.5) * 32767).astype(np.int16).tobytes())
    rec = Recording(id="recshort", sources=[AudioSource(type="file", channels=[0], source=str(path))], sampling_rate=16000, num_samples=N, duration=N / 16000)
    reflect = MonoCut(id="cshort", start=0, duration=rec.duration, channel=0, recording=rec).perturb_speed(1.1).mix(fastcopy(n, duration=0.3), snr=10)
    tracks = IS.deferred_mix(reflect)
    assert tracks is not None and IS._read_tracks(reflect, tracks) is None
    assert run([reflect, ok, s2]) == (1, 1, 1)

    # (3) a mix shorter than cut.num_samples (reflect-padded by the reference): refused before anything is read
    short = MixedCut(id="short", tracks=[MixTrack(cut=fastcopy(s, duration=0.5), type="MonoCut"),
                                         MixTrack(cut=fastcopy(n, duration=4000.4 / 16000), type="MonoCut", offset=4000.4 / 16000, snr=10)])
    assert short.num_samples == 8001 and IS.deferred_mix(short) is None
    assert run([short, ok]) == (1, 1, 1)

    # (4) recording_field is not None: every cut, mixed ones included, is read the reference's way (a custom recording has no tracks)
    custom = fastcopy(s, custom={"target_recording": n.recording}).pad(duration=1.5)
    assert isinstance(custom, MixedCut) and IS.deferred_mix(custom) is not None
    assert run([custom, fastcopy(s2, custom={"target_recording": n.recording})], recording_field="target_recording")[1:] == (0, 0)
    assert run([custom, s2]) == (0, 1, 1)  # (the same padded cut without the field goes to the device)
