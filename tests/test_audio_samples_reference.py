"""CPU, under the real lhotse (authoring container only): ``HipAudioSamples`` against the reference's own ``AudioSamples``
(lhotse/dataset/input_strategies.py:208-299) on one CutSet of unequal lengths that holds a plain cut, a speed-perturbed cut, a ``Volume`` +
hard ``Clipping`` cut, a reverberated cut, a ``CutMix``ed cut and a padded cut -- with CPU stand-ins for the device steps of the chain (the
ones tests/test_level_reference.py uses) and ``collate_ref`` (tests/_collate_ref.py) for the collate launch.

Bars: the shape and ``audio_lens`` are equal; the rows of the cuts whose chain is exact (plain, Volume, hard Clipping, pad) are
``array_equal``; the speed-perturbed and the mixed row are within 1e-5 (tests/test_mix_reference.py), the reverberated one within 1e-4
(tests/test_reverb_reference.py); all padding is exactly zero.  Each of the four fall-back cases returns what the parent returns."""
import numpy as np
import pytest
import torch

from _collate_ref import collate_ref
from test_level_reference import _rir, cpu_level
from test_resample_chain_reference import cpu_perturb, cpu_resample, cpu_reverb

SR = 16000
pytestmark = pytest.mark.reference


@pytest.fixture(scope="module")
def bound_to_lhotse():
    """``import_lhotse`` binds an already imported lhotse_amd to the real lhotse by reloading its modules IN PLACE, which the test modules that
    sort behind this one and hold classes of the unbound package (collected before anything ran) would not survive.  So this module works on
    a copy of its own: the unbound modules are set aside, a fresh lhotse_amd is imported under the real lhotse, and afterwards the
    interpreter is put back as it was -- path, lhotse and its stub dependencies included."""
    import sys

    import lhotse_amd.compat as compat

    if compat.HAVE_LHOTSE:  # (another module bound it already: nothing to protect)
        yield
        return
    from _dropin_support import import_lhotse

    path, before = list(sys.path), set(sys.modules)
    ours = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "lhotse_amd" or k.startswith("lhotse_amd.")}
    import_lhotse()
    yield
    foreign = ("lhotse", "soundfile", "intervaltree", "cytoolz")
    for k in list(sys.modules):
        if k == "lhotse_amd" or k.startswith("lhotse_amd.") or (k not in before and k.split(".")[0] in foreign):
            del sys.modules[k]
    sys.modules.update(ours)
    sys.path[:] = path


@pytest.fixture(scope="module")
def env(bound_to_lhotse, tmp_path_factory):
    from _dropin_support import install_wave_backend, write_cutset

    import lhotse.augmentation.torchaudio as ref_ta
    from lhotse.audio.backend import set_current_audio_backend

    was = ref_ta.is_torchaudio_available
    ref_ta.is_torchaudio_available = lambda: True  # the reference's sinc branch, as in the generator of the goldens
    prev = install_wave_backend()
    cuts = list(write_cutset(tmp_path_factory.mktemp("audiosampleswav"), [6000, 4800, 7200, 5000, 8000, 3000, 5600], seed=7))
    yield cuts
    set_current_audio_backend(prev)
    ref_ta.is_torchaudio_available = was


@pytest.fixture
def stand_ins(monkeypatch):
    import lhotse_amd.input_strategies as IS
    from _mix_ref import mix_in_arena_cpu

    calls = {"collate": 0, "level": 0, "reverb": 0, "mix": 0, "perturb": 0}

    def counted(name, fn):
        def run(*a):
            calls[name] += 1
            return fn(*a)

        return run

    def cpu_collate(arena, offsets, lengths, row_len, dtype):
        assert not arena.is_cuda
        return collate_ref(arena, offsets, lengths, row_len, None, dtype)

    monkeypatch.setattr(IS, "_collate_in_arena", counted("collate", cpu_collate))
    monkeypatch.setattr(IS, "_level_in_arena", counted("level", cpu_level))
    monkeypatch.setattr(IS, "_resample_in_arena", cpu_resample)
    monkeypatch.setattr(IS, "_perturb_in_arena", counted("perturb", cpu_perturb))
    monkeypatch.setattr(IS, "_mix_in_arena", counted("mix", mix_in_arena_cpu))
    monkeypatch.setattr(IS, "_reverb_in_arena", counted("reverb", cpu_reverb))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    return calls


def _batch(env, tmp_path):
    from lhotse import CutSet
    from lhotse.dataset.cut_transforms import CutMix

    c0, c1, c2, c3, c4, c5, c6 = env
    rir = _rir(tmp_path)
    mixed = list(CutMix(CutSet.from_cuts([c4]), snr=15, p=1.0, pad_to_longest=False, random_mix_offset=False, seed=3)(CutSet.from_cuts([c3])))[0]
    assert type(mixed).__name__ == "MixedCut"
    cuts = [c0,  # 0 plain
            c1.perturb_speed(1.1),  # 1 speed
            c2.perturb_volume(1.7).clip_amplitude(hard=True, gain_db=12.0, oversampling=None),  # 2 Volume + hard Clipping
            c5.reverb_rir(rir),  # 3 reverb
            mixed,  # 4 CutMix
            c6.pad(duration=c6.duration + 0.05)]  # 5 padded
    kinds = ["exact", 1e-5, "exact", 1e-4, 1e-5, "exact"]
    return CutSet.from_cuts(cuts), kinds


def test_hip_audio_samples_equals_the_reference(env, tmp_path, stand_ins, monkeypatch):
    from lhotse.dataset.input_strategies import AudioSamples

    import lhotse_amd as LA

    batch, kinds = _batch(env, tmp_path)
    assert len({c.num_samples for c in batch}) == len(batch)  # unequal lengths
    want_a, want_l = AudioSamples()(batch)
    loads = {"n": 0}
    for cls in {type(c) for c in batch}:
        real = cls.load_audio
        monkeypatch.setattr(cls, "load_audio", lambda self, *a, _real=real, **k: (loads.__setitem__("n", loads["n"] + 1), _real(self, *a, **k))[1])
    strat = LA.HipAudioSamples(device="cpu", return_device="cpu")
    assert (strat.gpu_speed_perturb, strat.gpu_mix, strat.gpu_reverb, strat.gpu_resample, strat.gpu_level) == (True,) * 5
    got_a, got_l = strat(batch)
    assert stand_ins["collate"] == 1 and stand_ins["level"] > 0 and stand_ins["reverb"] == 1 and stand_ins["mix"] == 1 and stand_ins["perturb"] == 1
    assert got_a.shape == want_a.shape and got_a.dtype == want_a.dtype == torch.float32
    assert got_l.dtype == want_l.dtype == torch.int32 and torch.equal(got_l, want_l)
    got, want = got_a.numpy(), want_a.numpy()
    for i, (cut, kind) in enumerate(zip(batch, kinds)):
        n = int(want_l[i])
        assert n == cut.num_samples
        if kind == "exact":
            assert np.array_equal(got[i, :n], want[i, :n]), (i, cut.id)
        else:
            d = float(np.abs(got[i, :n] - want[i, :n]).max())
            assert 0 < d <= kind or d == 0, (i, cut.id, d)
        assert not got[i, n:].view(np.uint32).any() and not want[i, n:].any(), (i, cut.id)  # all padding is exactly (+)zero
    # 2-byte samples: one rounding of the same values
    half = LA.HipAudioSamples(device="cpu", return_device="cpu", dtype=torch.bfloat16)(batch)[0]
    assert half.dtype == torch.bfloat16 and torch.equal(half, got_a.to(torch.bfloat16))
    # fault_tolerant: the third result is the CutSet that was read
    out = LA.HipAudioSamples(device="cpu", return_device="cpu", fault_tolerant=True)(batch)
    assert len(out) == 3 and [c.id for c in out[2]] == [c.id for c in batch] and torch.equal(out[0], got_a) and torch.equal(out[1], got_l)
    # with every switch off each cut is loaded the reference's way, and the rows are the reference's
    stand_ins.update(level=0, reverb=0, mix=0, perturb=0)
    off = LA.HipAudioSamples(device="cpu", return_device="cpu", gpu_speed_perturb=False, gpu_mix=False, gpu_reverb=False, gpu_resample=False, gpu_level=False)
    a_off, l_off = off(batch)
    assert (stand_ins["level"], stand_ins["reverb"], stand_ins["mix"], stand_ins["perturb"]) == (0, 0, 0, 0)
    assert torch.equal(l_off, want_l) and torch.equal(a_off, want_a)


def test_a_batch_of_plain_cuts_is_packed_and_collated_with_nothing_in_between(env, stand_ins):
    from lhotse import CutSet
    from lhotse.dataset.input_strategies import AudioSamples

    import lhotse_amd as LA

    batch = CutSet.from_cuts(env[:4])
    want_a, want_l = AudioSamples()(batch)
    got_a, got_l = LA.HipAudioSamples(device="cpu", return_device="cpu", num_workers=2)(batch)
    assert stand_ins == {"collate": 1, "level": 0, "reverb": 0, "mix": 0, "perturb": 0}
    assert torch.equal(got_a, want_a) and torch.equal(got_l, want_l) and got_l.dtype == torch.int32


def test_the_fall_back_cases_return_what_the_parent_returns(env, tmp_path, stand_ins):
    """``recording_field``, ``use_batch_loader``, ``mono_downmix=False`` and a batch with a multi-channel cut: the parent's own ``__call__``."""
    import wave

    from lhotse import CutSet, MultiCut, Recording
    from lhotse.audio import AudioSource
    from lhotse.dataset.input_strategies import AudioSamples

    import lhotse_amd as LA

    def same(got, want):
        assert len(got) == len(want) and stand_ins["collate"] == 0
        assert got[0].shape == want[0].shape and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[1].dtype == want[1].dtype

    batch = CutSet.from_cuts([env[0].perturb_volume(0.5), env[1], env[2].perturb_speed(0.9)])
    # mono_downmix=False: (B, C, T)
    want = AudioSamples(mono_downmix=False)(batch)
    assert want[0].ndim == 3
    same(LA.HipAudioSamples(device="cpu", return_device="cpu", mono_downmix=False)(batch), want)
    # recording_field: a custom recording attached to every cut
    from lhotse.utils import fastcopy

    with_field = CutSet.from_cuts([fastcopy(c, custom={"target_recording": c.recording}) for c in env[:3]])
    want = AudioSamples()(with_field, recording_field="target_recording")
    same(LA.HipAudioSamples(device="cpu", return_device="cpu")(with_field, recording_field="target_recording"), want)
    # use_batch_loader: the parent's batch loader runs (a stand-in that hands the cuts through)
    class Loader:
        calls = 0

        def __call__(self, cuts):
            Loader.calls += 1
            return cuts

    ref = AudioSamples()
    ref.use_batch_loader, ref.ais_batch_loader = True, Loader()
    ours = LA.HipAudioSamples(device="cpu", return_device="cpu")
    ours.use_batch_loader, ours.ais_batch_loader = True, Loader()
    same(ours(batch), ref(batch))
    assert Loader.calls == 2
    # a batch in which one cut has two channels
    n = 4000
    pcm = (np.random.RandomState(11).rand(n, 2) * 2.0 - 1.0) * np.array([3000.0, 20000.0])
    path = tmp_path / "stereo.wav"
    with wave.open(str(path), "wb") as f:
        f.setnchannels(2), f.setsampwidth(2), f.setframerate(SR)
        f.writeframes(pcm.astype(np.int16).tobytes())
    rec = Recording(id="stereo", sources=[AudioSource(type="file", channels=[0, 1], source=str(path))], sampling_rate=SR, num_samples=n, duration=n / SR)
    multi = MultiCut(id="multi", start=0, duration=rec.duration, channel=[0, 1], recording=rec)
    mixed_batch = CutSet.from_cuts([env[0], multi, env[1].perturb_volume(0.5)])
    same(LA.HipAudioSamples(device="cpu", return_device="cpu")(mixed_batch), AudioSamples()(mixed_batch))
    only_multi = CutSet.from_cuts([multi])
    want = AudioSamples()(only_multi)
    assert want[0].ndim == 3  # (every cut is multi-channel: the parent collates (B, C, T))
    same(LA.HipAudioSamples(device="cpu", return_device="cpu")(only_multi), want)
