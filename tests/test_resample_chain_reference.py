"""CPU: a ``Resample`` at the front of a recording's transforms taken over by the fused route.

Anywhere (no lhotse):
  * the goldens of tools/make_golden_resample_chain.py reload, the source files regenerate (CRC), and the float32 numpy statement of the
    device's order over the stored track tables stays within 2 x the reference's own distance + 2^-24 of the float64 chain (a single
    stage also within 1e-5 of ``load_audio()``);
  * ``resample_layout`` equals ``perturbed_layout`` bit for bit on speed ratios, and places ratio by ratio in ascending order;
  * ``FusedMiniBatch.features_of_tracks`` with CPU stand-ins for the device reproduces the reference's features over the tables.
Under the real lhotse (authoring container):
  * ``parse_chain`` accepts / refuses each case of the list, and nothing with a ``Resample`` when the resampling route is off;
  * ``read_before_chain`` reads the very file segments ``load_audio()`` reads (logging backend);
  * ``HipOnTheFlyFeatures`` with the stand-ins equals the reference's K2 batch, without one ``load_audio()`` of an eligible cut;
  * the default of ``gpu_resample`` with and without a pretended torchaudio."""
import random
from pathlib import Path

import numpy as np
import pytest
import torch

import _resample_chain as RC
from _mix_ref import mix_in_arena_cpu, mix_tracks

SR = 16000
REL_TOL, ABS_TOL = 1e-4, 2e-3  # the suite's bar for driver goldens (tests/test_gpu_reference_drivers.py)
AUDIO_GROUPS = ["resample", "resample_speed", "resample_cutmix"]


@pytest.fixture(scope="module")
def goldens():
    return RC.load_goldens()


@pytest.fixture(scope="module")
def paths(tmp_path_factory, goldens):
    return RC.source_files(tmp_path_factory.mktemp("srcwav"), goldens[1])


@pytest.fixture(scope="module")
def models(goldens, paths):
    """The float32 model of every cut of groups 1-3, computed once."""
    _, meta = goldens
    out = {}
    for group in AUDIO_GROUPS:
        for i, e in enumerate(meta["groups"][group]):
            tracks, ref = RC.chain_tracks(e, paths, RC.model_track)
            out[(group, i)] = tracks[0][0][: e["want"]] if len(tracks) == 1 else mix_tracks(tracks, ref, e["want"])
    return out


def test_goldens_reload_and_the_model_of_the_device_order_meets_the_audio_bar(goldens, models):
    arrays, meta = goldens
    assert set(meta["groups"]) == {"resample", "resample_speed", "resample_cutmix", "resample_speed_reverb", "k2"}
    ratios = {(r["source_rate"], r["factor"]) for g in meta["groups"].values() for e in g for r in e["tracks"]}
    assert {(44100, 1.0), (22050, 1.0), (8000, 1.0), (44100, 0.9), (44100, 1.1)} <= ratios
    assert {"mixed", "resample", "resample+speed"} <= set(meta["k2_kinds"])
    assert all(r.get("reverb") and r["source_rate"] for e in meta["groups"]["resample_speed_reverb"] for r in e["tracks"])
    for group, entries in meta["groups"].items():
        for i, e in enumerate(entries):
            f = arrays[f"{group}/{i}/feats"]
            assert f.dtype == np.float32 and f.shape[1] == 80 and abs(f.shape[0] - e["want"] / 160) <= 1 and e["want"] <= 16000
            assert e["audio"] == (group in AUDIO_GROUPS)
    for (group, i), model in models.items():
        e = meta["groups"][group][i]
        audio, truth = arrays[f"{group}/{i}/audio"], RC.exact_audio(arrays, group, i)
        assert len(model) == len(audio) == e["want"]
        assert abs(float(np.abs(audio - truth).max()) - e["reference_max_abs"]) <= 2.0 ** -24  # (the stored difference is float32)
        d = float(np.abs(model.astype(np.float64) - truth).max())
        assert d <= 2.0 * e["reference_max_abs"] + 2.0 ** -24, (group, i, d, e["reference_max_abs"])
        rows = e["tracks"]
        if len(rows) == 1 and len(RC.stages(rows[0]["source_rate"], rows[0]["factor"])) == 1:
            assert float(np.abs(model - audio).max()) <= 1e-5, (group, i)  # ABS_TOL of tests/test_gpu_resample.py


def test_resample_layout_generalises_perturbed_layout_bit_for_bit():
    from lhotse_amd.augmentation import perturbed_layout, perturbed_tail_floats, resample_layout, resampled_tail_floats

    rng = np.random.RandomState(0)
    for sr in (16000, 8000, 22050):
        for _ in range(20):
            n = int(rng.randint(1, 12))
            lens = rng.randint(0, 200000, size=n)
            offs = np.cumsum(np.r_[0, (lens + 3) & ~3])[:n]
            fac = rng.choice([0.9, 1.0, 1.1] if sr == 22050 else [0.9, 1.0, 1.1, 0.95, 1.05], size=n)  # (ratios with small banks)
            tail = int(offs[-1] + lens[-1])
            ratios = [None if f == 1.0 else (round(sr * f), sr) for f in fac]
            a, b = perturbed_layout(offs, lens, fac, sr, tail), resample_layout(offs, lens, ratios, tail)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
            assert a[0].dtype == b[0].dtype == np.int64 and np.all(b[0][fac != 1.0] % 4 == 0)
            assert resampled_tail_floats(lens, ratios) == perturbed_tail_floats(lens, fac, sr)
    # ratio by ratio in ascending order of (source, target), cuts of one ratio in their own order, every output on a 16-byte boundary
    lens = np.array([441, 1000, 882, 300, 4410], dtype=np.int64)
    offs = np.array([0, 444, 1444, 2328, 2628], dtype=np.int64)
    ratios = [(44100, 16000), None, (22050, 16000), (44100, 16000), (22050, 16000)]
    o, l, end = resample_layout(offs, lens, ratios, 7040)
    assert l.tolist() == [160, 1000, 640, 109, 3200]
    assert o.tolist() == [7040 + 640 + 3200, 444, 7040, 7040 + 640 + 3200 + 160, 7040 + 640] and end == 7040 + 640 + 3200 + 160 + 112
    assert resampled_tail_floats(lens, ratios) == end - 7040


# ---- CPU stand-ins for the device ----------------------------------------------------------------------------------------------
def cpu_resample(arena, offsets, lengths, ratios, tail_start):
    from lhotse_amd.augmentation import resample_layout

    po, pl, _ = resample_layout(offsets, lengths, ratios, tail_start)
    for i, r in enumerate(ratios):
        if r is not None:
            y = RC.fma_resample(arena[int(offsets[i]) : int(offsets[i] + lengths[i])].numpy(), r[0], r[1])
            assert len(y) == pl[i] and po[i] >= tail_start
            arena[int(po[i]) : int(po[i]) + len(y)] = torch.from_numpy(y)
    return po, pl


def cpu_perturb(arena, offsets, lengths, factors, sr, tail_start):
    return cpu_resample(arena, offsets, lengths, [None if f == 1.0 else (round(sr * f), sr) for f in factors], tail_start)


def cpu_reverb(arena, so, sl, ro, rl, shifts, norm, tail_start):
    import _reverb_ref as RV

    a = arena.numpy()
    tail = (int(tail_start) + 3) & ~3
    offs = []
    for s, n, r, taps, shift, nm in zip(so, sl, ro, rl, shifts, norm):
        y = RV.chunked32(a[int(s) : int(s) + int(n)].copy(), a[int(r) : int(r) + int(taps)].copy(), int(shift), bool(nm))
        a[tail : tail + len(y)] = y
        offs.append(tail)
        tail = (tail + len(y) + 3) & ~3
    return np.array(offs, dtype=np.int64)


@pytest.fixture
def stand_ins(monkeypatch):
    import lhotse_amd.extractors as E
    import lhotse_amd.input_strategies as IS
    from _dropin_support import make_cpu_plan

    calls = {"resample": 0, "perturb": 0}

    def counted(name, fn):
        def run(*a):
            calls[name] += 1
            return fn(*a)

        return run

    monkeypatch.setattr(E, "_Plan", make_cpu_plan())
    monkeypatch.setattr(IS, "_resample_in_arena", counted("resample", cpu_resample))
    monkeypatch.setattr(IS, "_perturb_in_arena", counted("perturb", cpu_perturb))
    monkeypatch.setattr(IS, "_mix_in_arena", mix_in_arena_cpu)
    monkeypatch.setattr(IS, "_reverb_in_arena", cpu_reverb)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    return calls


def _cpu_fbank(**kw):
    import lhotse_amd as LA

    return LA.HipFbank(LA.HipFbankConfig(**kw))


@pytest.mark.parametrize("group", ["resample", "resample_speed", "resample_cutmix", "resample_speed_reverb", "k2"])
def test_features_of_tracks_with_stand_ins_equals_the_reference_features(goldens, paths, models, stand_ins, group):
    from lhotse_amd.input_strategies import FusedMiniBatch

    arrays, meta = goldens
    entries = meta["groups"][group]
    ex = _cpu_fbank(edge_rule="batch_zero_pad") if group == "k2" else _cpu_fbank()
    rirs = {}
    tracks = [RC.tracks_of(e, paths, arrays, rirs) for e in entries]
    feats, lens, audio = FusedMiniBatch(ex, return_audio=True).features_of_tracks(tracks, [e["want"] for e in entries], SR)
    assert stand_ins["resample"] == 1  # ONE first pass for all source rates of the mini-batch
    assert stand_ins["perturb"] == int(any(r["factor"] != 1.0 for e in entries for r in e["tracks"]))
    want = [arrays[f"{group}/{i}/feats"] for i in range(len(entries))]
    assert [int(x) for x in lens] == [len(w) for w in want]
    for i, (e, w) in enumerate(zip(entries, want)):
        assert len(audio[i]) == e["want"]
        if (group, i) in models:  # the route places and truncates what the numpy statement states
            assert np.array_equal(audio[i].numpy(), models[(group, i)]), (group, i)
        got = feats[i, : len(w)].numpy().astype(np.float64)
        rel, mx = float(np.linalg.norm(got - w) / np.linalg.norm(w)), float(np.abs(got - w).max())
        assert rel <= REL_TOL and mx <= ABS_TOL, (group, i, rel, mx)


def test_a_mini_batch_without_a_source_rate_takes_the_route_it_took(goldens, paths, stand_ins):
    """8-element tracks whose source rate is None or the mini-batch's own: no first pass, and plain cuts are not even packed as tracks."""
    from lhotse_amd.input_strategies import FusedMiniBatch

    x = np.ascontiguousarray(RC.read_wav(paths["s16a"])[0])
    fm = FusedMiniBatch(_cpu_fbank(), return_audio=True)
    f0, l0, a0 = fm.features_of_tracks([[(x, 1.0, 0, None, True)], [(x[:4000], 1.1, 0, None, True, 3636)]], [len(x), 3636], SR)
    f1, l1, a1 = fm.features_of_tracks([[(x, 1.0, 0, None, True, len(x), None, None)], [(x[:4000], 1.1, 0, None, True, 3636, None, SR)]], [len(x), 3636], SR)
    assert stand_ins["resample"] == 0 and stand_ins["perturb"] == 2
    assert torch.equal(f0, f1) and torch.equal(l0, l1) and all(torch.equal(p, q) for p, q in zip(a0, a1))


# ---- under the real lhotse -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from _dropin_support import import_lhotse, install_wave_backend

    import_lhotse()
    import lhotse.augmentation.torchaudio as ref_ta
    from lhotse import CutSet, MonoCut, Recording, SupervisionSegment
    from lhotse.audio import AudioSource
    from lhotse.audio.backend import set_current_audio_backend

    was = ref_ta.is_torchaudio_available
    ref_ta.is_torchaudio_available = lambda: True  # the reference's sinc branch, as in the generator of the goldens
    prev = install_wave_backend()
    cuts = {}
    for f in RC.write_sources(tmp_path_factory.mktemp("chainwav")):
        dur = f["n"] / f["rate"]
        rec = Recording(id=f"rec-{f['id']}", sources=[AudioSource(type="file", channels=[0], source=f["path"])], sampling_rate=f["rate"], num_samples=f["n"],
                        duration=dur)
        sup = SupervisionSegment(id=f"sup-{f['id']}", recording_id=rec.id, start=0.0, duration=dur, channel=0, text=f["id"])
        cuts[f["id"]] = MonoCut(id=f["id"], start=0, duration=dur, channel=0, recording=rec, supervisions=[sup])
    yield cuts, CutSet
    set_current_audio_backend(prev)
    ref_ta.is_torchaudio_available = was


@pytest.mark.reference
def test_pending_chain_accepts_and_refuses(env, monkeypatch):
    import lhotse_amd.input_strategies as IS
    from lhotse import MultiCut, Recording
    from lhotse.audio import AudioSource
    from lhotse.audio import resampling_backend as RB
    from lhotse.utils import fastcopy

    cuts, _ = env
    c44, c22, c8, c16 = cuts["s44a"], cuts["s22a"], cuts["n8a"], cuts["s16a"]
    rir = Recording(id="rir", sources=[AudioSource(type="file", channels=[0], source=c16.recording.sources[0].source)], sampling_rate=SR, num_samples=7000,
                    duration=7000 / SR)
    def pending_chain(cut, **kw):  # the rule with the level route off: [Resample]? [Speed]? [Reverb]? is all it serves
        ch = IS.parse_chain(cut, gpu_level=False, **kw)
        assert ch is None or (isinstance(ch, IS.Chain) and ch.levels is None)
        return None if ch is None else (ch.source_rate, ch.factor, ch.reverb)

    # accepted: [Resample]? [Speed]? [Reverb]?
    assert pending_chain(c16) == (None, 1.0, None) and pending_chain(c16.perturb_speed(1.1)) == (None, 1.1, None)
    assert pending_chain(c44.resample(SR)) == (44100, 1.0, None)
    assert pending_chain(c22.resample(SR).perturb_speed(0.9)) == (22050, 0.9, None)
    assert pending_chain(c8.resample(SR)) == (8000, 1.0, None)
    ch = pending_chain(c44.resample(SR).perturb_speed(1.1).reverb_rir(rir))
    assert ch[:2] == (44100, 1.1) and ch[2]["normalize_output"] is True and ch[2]["rir_channels"] == [0]
    assert pending_chain(c44.resample(SR).reverb_rir(rir))[:2] == (44100, 1.0)
    assert pending_chain(c44.resample(24000)) == (44100, 1.0, None)
    # refused
    assert pending_chain(c44.perturb_speed(1.1).resample(SR)) is None  # a Resample that is not first
    assert pending_chain(c44.resample(22050).resample(SR)) is None  # more than one
    low = fastcopy(c16, recording=fastcopy(c16.recording, transforms=[{"name": "Resample", "kwargs": {"source_sampling_rate": SR, "target_sampling_rate": 8000}},
                                                                      {"name": "Resample", "kwargs": {"source_sampling_rate": 8000, "target_sampling_rate": SR}}]))
    assert pending_chain(low) is None  # (what LowpassUsingResampling appends)
    assert pending_chain(c44.resample(SR).perturb_volume(2.0)) is None and pending_chain(c44.resample(SR).reverb_rir()) is None
    assert pending_chain(c44.resample(SR), gpu_resample=False) is None
    assert pending_chain(c44.resample(SR).reverb_rir(rir), gpu_reverb=False) is None
    assert pending_chain(MultiCut(id="m", start=0, duration=c44.duration, channel=[0], recording=c44.resample(SR).recording)) is None
    wrong = fastcopy(c44.resample(SR), recording=fastcopy(c44.resample(SR).recording, sampling_rate=22050))
    assert pending_chain(wrong) is None  # a Resample to another rate than the cut's
    monkeypatch.setattr(RB, "CURRENT_RESAMPLING_BACKEND", "sox")
    assert pending_chain(c44.resample(SR)) is None and pending_chain(c16.perturb_speed(1.1)) == (None, 1.1, None)
    monkeypatch.setattr(RB, "CURRENT_RESAMPLING_BACKEND", "default")
    # the size of the reduced bank: every pair among the common rates -> 16 / 24 kHz is below 0.3 x 2^20 floats, the largest 441:640
    sizes = {(a, b): IS._sinc_bank_floats(a, b) for a in (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000) for b in (16000, 24000) if a != b}
    assert max(sizes, key=sizes.get) == (11025, 16000) and max(sizes.values()) < 0.3 * 2 ** 20
    from lhotse_amd.constants import sinc_resample_kernel

    assert sizes[(44100, 16000)] == sinc_resample_kernel(44100, 16000)[0].size == 76000
    big = fastcopy(c16, recording=fastcopy(c16.recording, sampling_rate=16001, transforms=[{"name": "Resample", "kwargs": {"source_sampling_rate": SR, "target_sampling_rate": 16001}}]))
    assert IS._sinc_bank_floats(SR, 16001) > 2 ** 20 and pending_chain(big) is None
    # with the resampling route off a Resample is nothing the rule knows, whatever follows it
    r = c44.resample(SR)
    assert pending_chain(r, gpu_resample=False) is None and pending_chain(r.reverb_rir(rir), gpu_resample=False) is None
    assert pending_chain(r.perturb_speed(1.1), gpu_resample=False) is None
    mixed = c16.mix(c8.resample(SR), snr=10)
    assert IS.deferred_mix(mixed) is None and IS.deferred_mix(mixed, True) is None
    tr = IS.deferred_mix(mixed, gpu_resample=True)
    assert tr[0].chain == IS.Chain() and tr[1][1:] == (0, 10, False, IS.Chain(source_rate=8000))
    assert IS.deferred_mix(c16.mix(c8.perturb_speed(0.9).resample(SR), snr=10), gpu_resample=True) is None


@pytest.mark.reference
def test_the_reader_reads_the_file_segments_the_reference_reads(env, monkeypatch):
    import lhotse_amd.input_strategies as IS
    from lhotse.audio.backend import get_current_audio_backend

    cuts, _ = env
    backend = get_current_audio_backend()
    reads, inner = [], backend.read_audio

    def logging_read(path_or_fd, offset=0.0, duration=None, force_opus_sampling_rate=None):
        audio, sr = inner(path_or_fd, offset=offset, duration=duration, force_opus_sampling_rate=force_opus_sampling_rate)
        reads.append((Path(str(path_or_fd)).stem, int(round(offset * sr)), int(audio.shape[1]), sr))
        return audio, sr

    monkeypatch.setattr(backend, "read_audio", logging_read, raising=False)
    c44, c22, c8 = cuts["s44a"], cuts["s22b"], cuts["n8a"]
    cases = [c44.resample(SR), c44.truncate(offset=0.0731, duration=0.2517).resample(SR), c22.resample(SR).perturb_speed(0.9),
             c22.truncate(offset=0.11, duration=0.3).resample(SR).perturb_speed(1.1), c8.resample(SR).truncate(offset=0.05, duration=0.4),
             c44.resample(SR).perturb_speed(1.1).truncate(offset=0.1, duration=0.2)]
    for cut in cases:
        del reads[:]
        ref = cut.load_audio()[0]
        ref_reads = list(reads)
        del reads[:]
        chain = IS.parse_chain(cut)
        ch = (chain.source_rate, chain.factor)
        assert chain == IS.Chain(*ch)
        raw = IS.read_before_chain(cut)
        assert reads == ref_reads and len(reads) == 1 and reads[0][2] == len(raw) and reads[0][3] == ch[0], cut
        want = int(cut.num_samples)
        assert IS.chain_num_samples(len(raw), ch[0], ch[1], SR) >= want
        model = RC.model_track(raw, ch[0], ch[1])[:want]
        assert len(model) == len(ref) and float(np.abs(model - ref).max()) <= 1e-5 * len(RC.stages(ch[0], ch[1]))
        track = IS._read_track(cut, chain)
        assert np.array_equal(track.samples, raw) and track[1:] == (ch[1], 0, None, True, want, None, ch[0], None)
    # a chain whose output is shorter than the cut (its file is shorter than the manifest states) takes the reference's path
    import wave

    from lhotse import MonoCut, Recording
    from lhotse.audio import AudioSource

    path = Path(cuts["s44a"].recording.sources[0].source).parent / "short44.wav"
    with wave.open(str(path), "wb") as fh:
        fh.setnchannels(1), fh.setsampwidth(2), fh.setframerate(44100)
        fh.writeframes(((np.random.RandomState(3).rand(22050 - 40) - 0.5) * 32767).astype(np.int16).tobytes())
    rec = Recording(id="short44", sources=[AudioSource(type="file", channels=[0], source=str(path))], sampling_rate=44100, num_samples=22050, duration=0.5)
    short = MonoCut(id="short44", start=0, duration=0.5, channel=0, recording=rec).resample(SR)
    assert IS.parse_chain(short) == IS.Chain(source_rate=44100) and IS._read_track(short, IS.parse_chain(short)) is None
    assert IS._read_one(short, True, False, True, True, True)[1:] == (1.0, 8000)  # (load_audio reflect-pads it)


@pytest.mark.reference
def test_strategy_with_stand_ins_equals_the_reference_k2_batch_without_a_load_audio(env, stand_ins, monkeypatch):
    import lhotse_amd as LA
    from lhotse.cut import MixedCut, MonoCut
    from lhotse.dataset import K2SpeechRecognitionDataset
    from lhotse.dataset.cut_transforms import CutMix, PerturbSpeed
    from lhotse.dataset.input_strategies import OnTheFlyFeatures
    from lhotse.features.kaldi.extractors import Fbank
    from lhotse.utils import fastcopy

    cuts, CutSet = env
    recipe = CutSet.from_cuts([cuts[k] for k in ("s44a", "s44b", "s22a", "s22b", "n8a")]).resample(SR)
    noise = CutSet.from_cuts([fastcopy(cuts[k], supervisions=[]) for k in ("n8a", "n8b")]).resample(SR)

    def transforms():
        return [PerturbSpeed(factors=[0.9, 1.1], p=2 / 3, randgen=random.Random(1)),
                CutMix(noise, snr=(10, 20), p=0.5, pad_to_longest=False, random_mix_offset=True, seed=13)]

    ref = K2SpeechRecognitionDataset(input_strategy=OnTheFlyFeatures(Fbank()), cut_transforms=transforms(), return_cuts=True)[recipe]
    batch_cuts = ref["supervisions"]["cut"]
    assert any(isinstance(c, MixedCut) for c in batch_cuts) and any(not isinstance(c, MixedCut) for c in batch_cuts)
    loads = {"n": 0}
    for cls in (MonoCut, MixedCut):
        real = cls.load_audio
        monkeypatch.setattr(cls, "load_audio", lambda self, *a, _real=real, **k: (loads.__setitem__("n", loads["n"] + 1), _real(self, *a, **k))[1])
    hip = LA.HipOnTheFlyFeatures(_cpu_fbank(edge_rule="batch_zero_pad"), gpu_resample=True, num_workers=2)
    got = K2SpeechRecognitionDataset(input_strategy=hip, cut_transforms=transforms(), return_cuts=True)[recipe]
    assert loads["n"] == 0  # every cut of the recipe is eligible: not one cut.load_audio()
    assert stand_ins["resample"] == 1 and stand_ins["perturb"] == 1
    assert torch.equal(got["supervisions"]["num_frames"], ref["supervisions"]["num_frames"]) and got["inputs"].shape == ref["inputs"].shape
    f, w = got["inputs"].numpy().astype(np.float64), ref["inputs"].numpy().astype(np.float64)
    for i, n in enumerate(ref["supervisions"]["num_frames"].tolist()):
        rel, mx = float(np.linalg.norm(f[i, :n] - w[i, :n]) / np.linalg.norm(w[i, :n])), float(np.abs(f[i, :n] - w[i, :n]).max())
        assert rel <= REL_TOL and mx <= ABS_TOL, (i, rel, mx)
    # switched off: the reference's own path, cut by cut
    off = LA.HipOnTheFlyFeatures(_cpu_fbank(edge_rule="batch_zero_pad"), gpu_resample=False)
    f2, l2 = off(CutSet.from_cuts(batch_cuts))
    assert loads["n"] >= len(batch_cuts) and stand_ins["resample"] == 1 and torch.equal(l2, ref["supervisions"]["num_frames"].to(l2.dtype))
    # the explicit contradiction raises when such a cut is met; the default with wave_transforms stays on the reference's path
    with pytest.raises(ValueError, match="gpu_resample=True was requested together with wave_transforms"):
        LA.HipOnTheFlyFeatures(_cpu_fbank(), wave_transforms=[lambda x: x], gpu_resample=True, gpu_mix=False, gpu_speed_perturb=False)(recipe)
    assert LA.HipOnTheFlyFeatures(_cpu_fbank(), wave_transforms=[lambda x: x]).gpu_resample is False


@pytest.mark.reference
def test_default_of_gpu_resample_follows_what_the_reference_would_run(env, monkeypatch):
    import lhotse.augmentation.torchaudio as ref_ta
    import lhotse_amd as LA
    from lhotse.audio import resampling_backend as RB

    monkeypatch.setattr(ref_ta, "is_torchaudio_available", lambda: True)
    assert LA.HipOnTheFlyFeatures(_cpu_fbank()).gpu_resample is True
    assert LA.HipOnTheFlyFeatures(_cpu_fbank(), gpu_resample=False).gpu_resample is False
    monkeypatch.setattr(RB, "CURRENT_RESAMPLING_BACKEND", "sox")
    assert LA.HipOnTheFlyFeatures(_cpu_fbank()).gpu_resample is False
    monkeypatch.setattr(RB, "CURRENT_RESAMPLING_BACKEND", "default")
    monkeypatch.setattr(ref_ta, "is_torchaudio_available", lambda: False)  # the reference would substitute scipy's resample_poly: another filter
    assert LA.HipOnTheFlyFeatures(_cpu_fbank()).gpu_resample is False
    assert LA.HipOnTheFlyFeatures(_cpu_fbank(), gpu_resample=True).gpu_resample is True
