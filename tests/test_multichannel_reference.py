"""CPU, under the real lhotse (authoring container only): ``HipAudioSamples`` with multi-channel cuts against the reference's own
``AudioSamples`` (lhotse/dataset/input_strategies.py:208-299, ``collate_audio``: lhotse/dataset/collation.py:148-247) -- multi-channel int16
WAVs through the stdlib backend, ``MultiCut``s of 2, 3 and 8 channels and of unequal lengths with mono cuts among them, the CPU stand-ins of
tests/test_audio_samples_reference.py for the chain and ``collate_sources_ref`` (tests/_multichannel_ref.py) for the new launch.

Bars: shape, dtype and ``audio_lens`` are the parent's in all three ``mono_downmix`` modes; the ``(B, C, T)`` form is ``array_equal``; the
downmix is ``array_equal`` for the cuts of one and of two channels, and for every C its largest error against the float64 mean of the row
is no larger than the parent's own (a correctly rounded value cannot lose); a ``[Resample, Speed]`` cut is within the 1e-5 of
tests/test_mix_reference.py.  A spy asserts that the parent's ``__call__`` is not entered for the batches the device serves, and that it is
for every remaining fall-back case, whose result is then the parent's.  (The reference collates ``(B, C, T)`` only where all multi-channel
cuts of a batch have the same C -- it raises otherwise -- so that form is compared per C; the device writes zero rows for the channels
a cut does not have.)"""
import wave

import numpy as np
import pytest
import torch

import _multichannel_golden as MG
from _collate_ref import collate_ref
from _multichannel_ref import collate_sources_ref
from test_audio_samples_reference import bound_to_lhotse  # noqa: F401  (the module-scoped binding to the real lhotse)
from test_level_reference import cpu_level
from test_resample_chain_reference import cpu_perturb, cpu_resample, cpu_reverb

SR = 16000
pytestmark = pytest.mark.reference


@pytest.fixture(scope="module")
def env(bound_to_lhotse, tmp_path_factory):  # noqa: F811
    from _dropin_support import install_wave_backend, write_cutset

    import lhotse.augmentation.torchaudio as ref_ta
    from lhotse.audio.backend import set_current_audio_backend

    was = ref_ta.is_torchaudio_available
    ref_ta.is_torchaudio_available = lambda: True  # the reference's sinc branch, as in the generator of the goldens
    prev = install_wave_backend()
    d = tmp_path_factory.mktemp("multichannelwav")
    multi = MG.write_cuts(d, MG.make_inputs())  # 2, 3, 1, 8 and 3 channels
    mono = list(write_cutset(d, [2600, 1850], seed=5))
    yield {"multi": multi, "mono": mono, "dir": d}
    set_current_audio_backend(prev)
    ref_ta.is_torchaudio_available = was


@pytest.fixture
def stand_ins(monkeypatch):
    import lhotse_amd.input_strategies as IS
    from _mix_ref import mix_in_arena_cpu

    calls = {"collate": 0, "sources": 0, "level": 0, "perturb": 0, "resample": 0}

    def counted(name, fn):
        def run(*a):
            calls[name] += 1
            return fn(*a)

        return run

    def cpu_collate(arena, offsets, lengths, row_len, dtype):
        assert not arena.is_cuda
        return collate_ref(arena, offsets, lengths, row_len, None, dtype)

    def cpu_sources(arena, first, src_offsets, lengths, row_len, dst_offsets, dtype):
        assert not arena.is_cuda
        return collate_sources_ref(arena, first, src_offsets, lengths, row_len, dst_offsets, dtype)

    monkeypatch.setattr(IS, "_collate_in_arena", counted("collate", cpu_collate))
    monkeypatch.setattr(IS, "_collate_sources_in_arena", counted("sources", cpu_sources))
    monkeypatch.setattr(IS, "_level_in_arena", counted("level", cpu_level))
    monkeypatch.setattr(IS, "_resample_in_arena", counted("resample", cpu_resample))
    monkeypatch.setattr(IS, "_perturb_in_arena", counted("perturb", cpu_perturb))
    monkeypatch.setattr(IS, "_mix_in_arena", mix_in_arena_cpu)
    monkeypatch.setattr(IS, "_reverb_in_arena", cpu_reverb)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    return calls


@pytest.fixture
def spy(monkeypatch, bound_to_lhotse):  # noqa: F811
    """Counts the entries into the parent's own ``__call__``."""
    from lhotse.dataset.input_strategies import AudioSamples

    entered = {"n": 0}
    real = AudioSamples.__call__

    def counting(self, *a, **k):
        entered["n"] += 1
        return real(self, *a, **k)

    monkeypatch.setattr(AudioSamples, "__call__", counting)
    return entered


def _ours(**kw):
    import lhotse_amd as LA

    return LA.HipAudioSamples(device="cpu", return_device="cpu", gpu_channels=True, **kw)


def _same_frame(got, want):
    assert len(got) == len(want)
    assert got[0].shape == want[0].shape and got[0].dtype == want[0].dtype == torch.float32
    assert got[1].dtype == want[1].dtype == torch.int32 and torch.equal(got[1], want[1])


def _f64_mean(cut):
    return cut.load_audio().astype(np.float64).mean(axis=0)


def test_the_downmix_has_the_parents_frame_and_cannot_lose_to_it(env, stand_ins, spy):
    from lhotse import CutSet
    from lhotse.dataset.input_strategies import AudioSamples

    c2, c3, c1, c8, c3b = env["multi"]
    m0, m1 = env["mono"]
    cuts = [c2, m0.perturb_volume(0.5), c3, c1, c8, m1, c3b]
    batch = CutSet.from_cuts(cuts)
    assert len({c.num_samples for c in batch}) == len(cuts)  # unequal lengths
    for mode in (None, True):
        want = AudioSamples(mono_downmix=mode)(batch)
        assert want[0].ndim == 2
        spy["n"], stand_ins["sources"], stand_ins["collate"] = 0, 0, 0
        got = _ours(mono_downmix=mode)(batch)
        assert spy["n"] == 0 and stand_ins["sources"] == 1 and stand_ins["collate"] == 0 and stand_ins["level"] > 0  # ONE launch, no fall-back
        _same_frame(got, want)
        g, w = got[0].numpy(), want[0].numpy()
        for i, cut in enumerate(cuts):
            n = cut.num_samples
            assert int(want[1][i]) == n and not g[i, n:].view(np.uint32).any()  # all padding is exactly (+)zero
            if cut.num_channels <= 2:
                assert np.array_equal(g[i, :n], w[i, :n]), (mode, i, cut.id)
            else:
                t = _f64_mean(cut)
                ours, theirs = np.abs(g[i, :n] - t).max(), np.abs(w[i, :n] - t).max()
                print(f"mode={mode} cut {cut.id} C={cut.num_channels}: max |row - float64 mean| ours {ours:.3e} parent {theirs:.3e}")
                assert ours <= theirs, (mode, i, cut.id, ours, theirs)
    # 2-byte samples: one rounding of the float32 batch
    half = _ours(mono_downmix=True, dtype=torch.bfloat16)(batch)[0]
    assert half.dtype == torch.bfloat16 and torch.equal(half, got[0].to(torch.bfloat16))


def test_the_channel_form_equals_the_parents(env, stand_ins, spy):
    from lhotse import CutSet
    from lhotse.dataset.input_strategies import AudioSamples

    m0, m1 = env["mono"]
    for c, ids in MG.FALSE_BATCHES.items():
        cuts = [env["multi"][i] for i in ids] + [m0.perturb_speed(1.1)]
        batch = CutSet.from_cuts(cuts)
        want = AudioSamples(mono_downmix=False)(batch)
        assert want[0].shape[:2] == (len(cuts), c)
        spy["n"], stand_ins["sources"], stand_ins["perturb"] = 0, 0, 0
        got = _ours(mono_downmix=False)(batch)
        assert spy["n"] == 0 and stand_ins["sources"] == 1 and stand_ins["perturb"] == 1  # (the mono cut keeps its device chain)
        _same_frame(got, want)
        g, w = got[0].numpy(), want[0].numpy()
        assert np.array_equal(g[:-1], w[:-1]) and not g[-1, 1:].view(np.uint32).any()
        d = np.abs(g[-1, 0] - w[-1, 0]).max()
        assert d <= 1e-5, d  # the speed-perturbed mono cut in channel 0 (tests/test_mix_reference.py)
    # mono_downmix=None where every cut has more than one channel: (B, C, T)
    multi = CutSet.from_cuts([env["multi"][i] for i in MG.NONE_MULTI])
    want = AudioSamples()(multi)
    assert want[0].ndim == 3
    spy["n"] = 0
    got = _ours()(multi)
    assert spy["n"] == 0
    _same_frame(got, want)
    assert np.array_equal(got[0].numpy(), want[0].numpy())
    # mono cuts alone with mono_downmix=False: (B, 1, T)
    monos = CutSet.from_cuts([m0, m1.perturb_volume(2.0)])
    want = AudioSamples(mono_downmix=False)(monos)
    spy["n"] = 0
    got = _ours(mono_downmix=False)(monos)
    assert spy["n"] == 0 and want[0].shape[1] == 1
    _same_frame(got, want)
    assert np.array_equal(got[0].numpy(), want[0].numpy())
    # cuts of 2, 3 and 8 channels in one (B, C, T) batch, which the reference refuses: zero rows for the channels a cut does not have
    mixed_c = [env["multi"][i] for i in (0, 1, 3)]
    with pytest.raises(RuntimeError):
        AudioSamples(mono_downmix=False)(CutSet.from_cuts(mixed_c))
    spy["n"] = 0
    a, lens = _ours(mono_downmix=False)(CutSet.from_cuts(mixed_c))
    assert a.shape == (3, 8, 2100) and lens.tolist() == [2100, 1700, 1500]
    for i, cut in enumerate(mixed_c):
        n, c = cut.num_samples, cut.num_channels
        assert np.array_equal(a[i, :c, :n].numpy(), cut.load_audio()) and not a[i, c:].numpy().view(np.uint32).any() and not a[i, :, n:].numpy().view(np.uint32).any()


def test_the_golden_is_what_the_live_reference_returns(env):
    from lhotse import CutSet
    from lhotse.dataset.collation import collate_audio

    g = MG.load()
    assert all(np.array_equal(a, b) for a, b in zip(g["inputs"], MG.make_inputs()))
    batch = CutSet.from_cuts(env["multi"])
    for name, mode in (("true", True), ("none", None)):
        audio, lens = collate_audio(batch, mono_downmix=mode)
        assert np.array_equal(audio.numpy(), g[name]) and np.array_equal(lens.numpy(), g["lens"])
    for c, ids in MG.FALSE_BATCHES.items():
        assert np.array_equal(collate_audio(CutSet.from_cuts([env["multi"][i] for i in ids]), mono_downmix=False)[0].numpy(), g[f"false/{c}"])
    assert np.array_equal(collate_audio(CutSet.from_cuts([env["multi"][i] for i in MG.NONE_MULTI]))[0].numpy(), g["none_multi"])


def test_padded_cuts_left_and_right(env, stand_ins, spy):
    from lhotse import CutSet
    from lhotse.dataset.input_strategies import AudioSamples

    import lhotse_amd.input_strategies as IS

    c2, c3, c1, c8, c3b = env["multi"]
    left = c3.pad(duration=c3.duration + 0.03, direction="left")
    right = c8.pad(duration=c8.duration + 0.021, direction="right")
    assert type(left).__name__ == type(right).__name__ == "MixedCut"
    chain = IS.pending_channel_chain(left)
    assert chain[0] is not None and chain[1:] == (None, 1.0, 480, c3.num_samples + 480)
    assert IS.pending_channel_chain(right)[1:] == (None, 1.0, 0, c8.num_samples + 336)
    for mode in (True, False):
        cuts = [left, right] if mode else [left, c3b, env["mono"][0]]  # (one C per (B, C, T) batch of the reference)
        batch = CutSet.from_cuts(cuts)
        want = AudioSamples(mono_downmix=mode)(batch)
        spy["n"] = 0
        got = _ours(mono_downmix=mode)(batch)
        assert spy["n"] == 0
        _same_frame(got, want)
        if mode:
            g, w = got[0].numpy(), want[0].numpy()
            assert not g[0, :480].view(np.uint32).any()  # the padding in front
            for i, (cut, inner) in enumerate(((left, c3), (right, c8))):
                t = np.zeros(want[0].shape[1])
                off = 480 if i == 0 else 0
                t[off : off + inner.num_samples] = _f64_mean(inner)
                assert np.abs(g[i] - t).max() <= np.abs(w[i] - t).max(), i
        else:
            assert np.array_equal(got[0].numpy(), want[0].numpy())


def test_fault_tolerant_drops_the_unreadable_cut(env, stand_ins, spy, monkeypatch):
    from lhotse import CutSet
    from lhotse.audio import AudioSource
    from lhotse.audio.backend import get_current_audio_backend
    from lhotse.audio.utils import AudioLoadingError
    from lhotse.dataset.input_strategies import AudioSamples
    from lhotse.utils import fastcopy

    backend = get_current_audio_backend()
    inner = backend.read_audio

    def failing_read(path_or_fd, *a, **k):  # (what lhotse's own backends raise for a file they cannot decode)
        if "nonexistent" in str(path_or_fd):
            raise AudioLoadingError(f"cannot read {path_or_fd}")
        return inner(path_or_fd, *a, **k)

    monkeypatch.setattr(backend, "read_audio", failing_read, raising=False)
    c2, c3, c1, c8, c3b = env["multi"]
    broken = fastcopy(c3b, id="broken", recording=fastcopy(c3b.recording, sources=[AudioSource(type="file", channels=[0, 1, 2], source="/nonexistent/x.wav")]))
    batch = CutSet.from_cuts([c2, broken, c8, env["mono"][1]])
    want = AudioSamples(mono_downmix=True, fault_tolerant=True)(batch)
    spy["n"] = 0
    got = _ours(mono_downmix=True, fault_tolerant=True)(batch)
    assert spy["n"] == 0 and len(got) == 3
    assert [c.id for c in got[2]] == [c.id for c in want[2]] == [c2.id, c8.id, env["mono"][1].id]
    _same_frame(got[:2], want[:2])
    g, w = got[0].numpy(), want[0].numpy()
    assert np.array_equal(g[0], w[0]) and np.array_equal(g[2], w[2])
    t = np.zeros(g.shape[1])
    t[: c8.num_samples] = _f64_mean(c8)
    assert np.abs(g[1] - t).max() <= np.abs(w[1] - t).max()
    with pytest.raises(AudioLoadingError):
        _ours(mono_downmix=True)(batch)


def _rate_cut(d, rate, n, channels, seed):
    from lhotse import MultiCut, Recording
    from lhotse.audio import AudioSource

    pcm = ((np.random.RandomState(seed).rand(n, channels) - 0.5) * 30000).astype(np.int16)
    p = str(d / f"rate{rate}_{channels}_{seed}.wav")
    with wave.open(p, "wb") as f:
        f.setnchannels(channels), f.setsampwidth(2), f.setframerate(rate)
        f.writeframes(pcm.tobytes())
    rec = Recording(id=f"rate{rate}_{seed}", sources=[AudioSource(type="file", channels=list(range(channels)), source=p)], sampling_rate=rate,
                    num_samples=n, duration=n / rate)
    return MultiCut(id=f"rate{rate}_{seed}", start=0, duration=rec.duration, channel=list(range(channels)), recording=rec)


def test_a_resampled_and_speed_perturbed_cut_runs_its_chain_per_channel(env, stand_ins, spy):
    from lhotse import CutSet
    from lhotse.dataset.input_strategies import AudioSamples

    import lhotse_amd.input_strategies as IS

    c22 = _rate_cut(env["dir"], 22050, 6000, 3, 31).resample(SR).perturb_speed(0.9)
    c3 = env["multi"][1].perturb_speed(1.1)
    assert IS.pending_channel_chain(c22)[1:] == (22050, 0.9, 0, None) and IS.pending_channel_chain(c3)[1:] == (None, 1.1, 0, None)
    batch = CutSet.from_cuts([c22, c3, env["multi"][4]])
    for mode in (True, False):
        want = AudioSamples(mono_downmix=mode)(batch)
        spy["n"], stand_ins["resample"], stand_ins["perturb"] = 0, 0, 0
        got = _ours(mono_downmix=mode)(batch)
        assert spy["n"] == 0 and stand_ins["resample"] == 1 and stand_ins["perturb"] == 1
        _same_frame(got, want)
        d = float((got[0] - want[0]).abs().max())
        print(f"mono_downmix={mode}: max |ours - parent| = {d:.3e}")
        assert d <= 1e-5, d
        if not mode:
            assert np.array_equal(got[0][2].numpy(), want[0][2].numpy())  # the cut without a chain
    # the switches are those of the mono route
    off = _ours(mono_downmix=True, gpu_speed_perturb=False, gpu_resample=False)
    spy["n"] = 0
    assert torch.equal(off(batch)[0], AudioSamples(mono_downmix=True)(batch)[0]) and spy["n"] == 2  # (ours fell back, and the parent itself)


def test_every_remaining_fall_back_case_returns_what_the_parent_returns(env, stand_ins, spy, tmp_path):
    from lhotse import CutSet
    from lhotse.cut import MixedCut, MixTrack
    from lhotse.dataset.input_strategies import AudioSamples
    from lhotse.utils import fastcopy

    import lhotse_amd.input_strategies as IS

    c2, c3, c1, c8, c3b = env["multi"]
    m0, m1 = env["mono"]

    def falls_back(batch, ours_kw=None, call_kw=None, ref=None, mine=None):
        ref = AudioSamples(**(ours_kw or {})) if ref is None else ref
        mine = _ours(**(ours_kw or {})) if mine is None else mine
        want = ref(batch, **(call_kw or {}))
        spy["n"], stand_ins["sources"], stand_ins["collate"] = 0, 0, 0
        got = mine(batch, **(call_kw or {}))
        assert spy["n"] == 1 and stand_ins["sources"] == 0 and stand_ins["collate"] == 0
        _same_frame(got, want)
        assert torch.equal(got[0], want[0])

    # a multi-channel cut with a transform other than [Resample]? [Speed]?
    for bad in (c2.perturb_volume(0.5), c2.clip_amplitude(hard=True, gain_db=6.0, oversampling=None), c3.perturb_speed(1.1).perturb_volume(2.0),
                c2.perturb_speed(0.9).resample(8000).resample(SR)):
        assert IS.pending_channel_chain(bad) is None
        falls_back(CutSet.from_cuts([bad, m0]))
    # a Resample that is not first
    c22 = _rate_cut(tmp_path, 22050, 5000, 2, 7)
    late = c22.perturb_speed(1.1).resample(SR)
    assert IS.pending_channel_chain(late) is None
    falls_back(CutSet.from_cuts([late, m0]))
    # a multi-channel track that is mixed with audio
    mixed = c2.mix(m1, snr=10)
    assert type(mixed).__name__ == "MixedCut" and IS.pending_channel_chain(mixed) is None
    falls_back(CutSet.from_cuts([mixed, m0]))
    # more than 32 channels
    wide = MG.write_cuts(tmp_path, MG.make_inputs([(33, 300)], seed=9), prefix="wide")[0]
    assert wide.num_channels == 33 and IS.pending_channel_chain(wide) is None
    assert IS.pending_channel_chain(MG.write_cuts(tmp_path, MG.make_inputs([(32, 300)], seed=9), prefix="w32")[0]) is not None
    falls_back(CutSet.from_cuts([wide]))
    # recording_field
    with_field = CutSet.from_cuts([fastcopy(c, custom={"target_recording": c.recording}) for c in (c2, m0)])
    falls_back(with_field, call_kw={"recording_field": "target_recording"})
    # use_batch_loader (a stand-in that hands the cuts through)
    class Loader:
        def __call__(self, cuts):
            return cuts

    ref, mine = AudioSamples(), _ours()
    ref.use_batch_loader, ref.ais_batch_loader = True, Loader()
    mine.use_batch_loader, mine.ais_batch_loader = True, Loader()
    falls_back(CutSet.from_cuts([c2, m0]), ref=ref, mine=mine)
    # gpu_channels=False: the switch; and its default on a device without a GPU
    import lhotse_amd as LA

    for strat in (LA.HipAudioSamples(device="cpu", return_device="cpu", gpu_channels=False), LA.HipAudioSamples(device="cpu", return_device="cpu")):
        assert strat.gpu_channels is False
        falls_back(CutSet.from_cuts([c2, m0]), ref=AudioSamples(), mine=strat)
    assert LA.HipAudioSamples(device="cuda:0").gpu_channels is True


def test_the_rule_on_single_cuts(env):
    import lhotse_amd.input_strategies as IS

    c2, c3, c1, c8, c3b = env["multi"]
    assert IS.pending_channel_chain(c2) == (c2, None, 1.0, 0, None)
    assert IS.pending_channel_chain(c1) is None and IS.pending_channel_chain(env["mono"][0]) is None  # a MonoCut: the mono route's
    assert IS.pending_channel_chain(c3.perturb_speed(0.9), gpu_speed=False) is None
    assert IS.pending_channel_chain(c3.perturb_speed(0.9))[1:3] == (None, 0.9)
    padded_twice = c2.pad(duration=c2.duration + 0.01).pad(duration=c2.duration + 0.02, direction="left")
    ch = IS.pending_channel_chain(padded_twice)
    assert ch is not None and ch[3] == 160 and ch[4] == c2.num_samples + 320
