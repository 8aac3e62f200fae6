"""
Drop-in check against the REAL lhotse package (authoring container only: needs /root/reference).

The Hip* extractors must be usable, unchanged, by lhotse's own drivers:
  CutSet.compute_and_store_features_batch   lhotse/cut/set.py:2197-2408
  CutSet.compute_and_store_features         lhotse/cut/set.py:1981-2195
  OnTheFlyFeatures                          lhotse/dataset/input_strategies.py:351-476
There is no GPU here, so the DEVICE side (one class, extractors._Plan) is replaced by a CPU
stand-in built on the oracle; everything above it -- input normalisation, packing, return
conventions, registry, YAML, manifests, validate_features -- is the product code under test.
GPU numerics are covered by tests/test_gpu_parity.py.
"""
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.reference


@pytest.fixture(scope="module")
def lhotse_mod():
    from _dropin_support import import_lhotse

    return import_lhotse()


@pytest.fixture()
def cpu_device(monkeypatch, lhotse_mod):
    """Replace the device plan by an oracle-backed stand-in (same interface)."""
    import lhotse_amd.extractors as E
    from oracle.kaldi_ref import RefConfig, RefExtractor

    kinds = {0: "spectrogram", 1: "log-spectrogram", 2: "fbank", 3: "mfcc"}

    class CpuPlan:
        def __init__(self, cfg, kind, device, mel_floor=None):
            fields = {k: getattr(cfg, k) for k in RefConfig.__dataclass_fields__ if hasattr(cfg, k)}
            self.ref = RefExtractor(RefConfig(kind=kinds[kind], **fields), np.float32)
            self.device = torch.device("cpu")
            self.feature_dim = self.ref.feature_dim
            self.kernel_name = "cpu-stand-in"
            self.n, self.shift, self.snip_edges = self.ref.n, self.ref.shift, int(cfg.snip_edges)

        def run(self, wave, offsets, lengths, padded):
            outs = []
            for i, (o, l) in enumerate(zip(offsets, lengths)):
                f = self.ref.extract(wave[o : o + l].numpy(), padded_len=None if padded is None else int(padded[i]))
                if padded is not None:
                    f = f[: (int(l) + self.shift // 2) // self.shift]
                outs.append(torch.from_numpy(np.ascontiguousarray(f)))
            return torch.cat(outs), np.array([len(o) for o in outs], dtype=np.int64)

        def run_collated(self, wave, offsets, lengths, padded, pad_value):
            packed, frames = self.run(wave, offsets, lengths, padded)
            out = torch.full((len(frames), int(frames.max()), self.feature_dim), pad_value, dtype=torch.float32)
            for i, f in enumerate(packed.split(frames.tolist())):
                out[i, : len(f)] = f
            return out, frames

        def close(self):
            pass

    monkeypatch.setattr(E, "_Plan", CpuPlan)
    return CpuPlan


@pytest.fixture()
def cutset(tmp_path, lhotse_mod):
    from lhotse import CutSet, MonoCut, Recording
    from lhotse.audio import AudioSource
    from lhotse.audio.backend import AudioBackend, get_current_audio_backend, set_current_audio_backend

    class StdlibWaveBackend(AudioBackend):  # soundfile is not installed here; int16 WAV via the stdlib
        def read_audio(self, path_or_fd, offset=0.0, duration=None, force_opus_sampling_rate=None):
            with wave.open(str(path_or_fd), "rb") as f:
                sr, n, ch = f.getframerate(), f.getnframes(), f.getnchannels()
                start = int(round(offset * sr))
                f.setpos(start)
                raw = f.readframes(n - start if duration is None else int(round(duration * sr)))
            return np.frombuffer(raw, dtype=np.int16).reshape(-1, ch).T.astype(np.float32) / 32768.0, sr

        def is_applicable(self, p):
            return str(p).endswith(".wav")

        handles_special_case = is_applicable

    prev = get_current_audio_backend()
    set_current_audio_backend(StdlibWaveBackend())
    rs = np.random.RandomState(0)
    cuts = []
    for i, n in enumerate([16000, 24000, 12345, 32000, 8000]):
        x = rs.rand(n) - 0.5
        p = tmp_path / f"r{i}.wav"
        with wave.open(str(p), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes((x * 32767).astype(np.int16).tobytes())
        rec = Recording(id=f"rec{i}", sources=[AudioSource(type="file", channels=[0], source=str(p))], sampling_rate=16000,
                        num_samples=n, duration=n / 16000)
        cuts.append(MonoCut(id=f"cut{i}", start=0, duration=rec.duration, channel=0, recording=rec))
    yield CutSet.from_cuts(cuts)
    set_current_audio_backend(prev)


def test_plugin_registration(lhotse_mod):
    import lhotse_amd as LA
    from lhotse.features.base import FEATURE_EXTRACTORS, FeatureExtractor, create_default_feature_extractor

    for cls in (LA.HipFbank, LA.HipMfcc, LA.HipSpectrogram, LA.HipLogSpectrogram):
        assert issubclass(cls, FeatureExtractor)
        assert FEATURE_EXTRACTORS[cls.name] is cls  # -> shows up in `lhotse feat extract -f` (bin/modes/features.py:40)
        assert isinstance(create_default_feature_extractor(cls.name), cls)  # no GPU needed (cut/mixed.py:1252)


def test_yaml_through_lhotse(tmp_path, lhotse_mod):
    import lhotse_amd as LA
    from lhotse.features.base import FeatureExtractor
    from lhotse.features.kaldi.extractors import Fbank

    ex = LA.HipFbank(LA.HipFbankConfig(num_filters=40))
    ex.to_yaml(tmp_path / "f.yml")
    back = FeatureExtractor.from_yaml(tmp_path / "f.yml")
    assert type(back) is LA.HipFbank and back.config == ex.config
    # a kaldi-fbank config becomes a hip-fbank config by changing only feature_type
    d = Fbank().to_dict()
    d["feature_type"] = "hip-fbank"
    assert type(FeatureExtractor.from_dict(d)) is LA.HipFbank


@pytest.mark.parametrize("collate", [False, True])
def test_compute_and_store_features_batch(tmp_path, cutset, cpu_device, collate):
    import lhotse_amd as LA
    from lhotse.features.io import NumpyFilesWriter
    from lhotse.features.kaldi.extractors import Fbank

    ex = LA.HipFbank(LA.HipFbankConfig(device="cpu", edge_rule="batch_zero_pad"))
    out = cutset.compute_and_store_features_batch(
        extractor=ex, storage_path=tmp_path / "feats", manifest_path=tmp_path / "cuts.jsonl.gz", batch_duration=3.0,
        num_workers=0, collate=collate, storage_type=NumpyFilesWriter,
    )
    ref = Fbank()
    assert len(out) == len(cutset)
    for c in out:
        f = c.load_features()
        assert c.features.type == "hip-fbank" and f.dtype == np.float32
        assert f.shape == (c.features.num_frames, 80) == ((c.num_samples + 80) // 160, 80)  # validate_features contract
    # the collated path zero pads like the reference's batch path, so it can be compared with it item by item
    batch = [c.load_audio() for c in cutset]
    want = ref.extract_batch([torch.from_numpy(b) for b in batch], 16000)
    got = LA.HipFbank(LA.HipFbankConfig(device="cpu", edge_rule="batch_zero_pad")).extract_batch([torch.from_numpy(b) for b in batch], 16000)
    for g, w in zip(got, want):
        np.testing.assert_allclose(g.numpy(), w.numpy(), atol=2e-3, rtol=1e-4)


def test_batch_driver_resume(tmp_path, cutset, cpu_device):
    import lhotse_amd as LA
    from lhotse.features.io import NumpyFilesWriter

    ex = LA.HipFbank(LA.HipFbankConfig(device="cpu"))
    kw = dict(extractor=ex, storage_path=tmp_path / "feats", manifest_path=tmp_path / "cuts.jsonl.gz", batch_duration=3.0,
              num_workers=0, storage_type=NumpyFilesWriter)
    first = cutset.subset(first=2).compute_and_store_features_batch(**kw)
    assert len(first) == 2
    allc = cutset.compute_and_store_features_batch(**kw, overwrite=False)  # resumes: only the missing cuts are computed
    assert sorted(c.id for c in allc) == sorted(c.id for c in cutset)


def test_per_cut_driver_and_on_the_fly(tmp_path, cutset, cpu_device):
    import lhotse_amd as LA
    from lhotse.dataset.input_strategies import OnTheFlyFeatures
    from lhotse.features.io import NumpyFilesWriter
    from lhotse.utils import LOG_EPSILON

    ex = LA.HipFbank(LA.HipFbankConfig(device="cpu"))
    out = cutset.compute_and_store_features(extractor=ex, storage_path=tmp_path / "f1", num_jobs=1, storage_type=NumpyFilesWriter)
    per_cut = {c.id: c.load_features() for c in out}
    assert all(v.shape[1] == 80 for v in per_cut.values())
    # OnTheFlyFeatures: list of 1-D tensors -> extract_batch -> padded with LOG_EPSILON
    feats, lens = OnTheFlyFeatures(ex)(cutset)
    assert feats.shape[0] == len(cutset) and feats.shape[2] == 80
    for i, c in enumerate(cutset):
        t = int(lens[i])
        assert t == per_cut[c.id].shape[0]
        np.testing.assert_allclose(feats[i, :t].numpy(), per_cut[c.id], atol=1e-5)  # per-item reflect == extract()
        if t < feats.shape[1]:
            assert torch.all(feats[i, t:] == LOG_EPSILON)


def test_speed_perturbation_through_recording_transforms(cutset, lhotse_mod, monkeypatch):
    """Recording.load_audio applies AudioTransforms lazily (lhotse/audio/recording.py:431-475): HipSpeed must be
    accepted there (registry, reverse_timestamps, output length bookkeeping) and reproduce Speed's samples.
    The device object (HipResampleTensor) is replaced by an oracle-backed stand-in; GPU numerics are covered by
    tests/test_gpu_resample.py."""
    import lhotse_amd.augmentation as A
    from lhotse.augmentation import AudioTransform, Speed
    from lhotse.utils import fastcopy
    from oracle import resample_ref as R

    assert issubclass(A.HipSpeed, AudioTransform) and AudioTransform.KNOWN_TRANSFORMS["HipSpeed"] is A.HipSpeed

    class CpuResampler:
        def __init__(self, orig_freq, new_freq, device=None):
            self.o, self.n = orig_freq, new_freq

        def __call__(self, t):
            return torch.from_numpy(np.stack([R.resample(row, self.o, self.n) for row in t.numpy().reshape(-1, t.shape[-1])]))

    monkeypatch.setattr(A, "HipResampleTensor", CpuResampler)
    monkeypatch.setattr(A, "_precompiled_resamplers", {})
    for factor in (0.9, 1.1):
        for cut in cutset:
            sp = cut.perturb_speed(factor)
            want = sp.load_audio()
            assert isinstance(sp.recording.transforms[0], (Speed, dict))
            hip_rec = fastcopy(sp.recording, transforms=[A.HipSpeed(factor).to_dict()])  # as read back from a manifest
            hip = fastcopy(sp, recording=hip_rec)
            got = hip.load_audio()
            assert got.shape == want.shape == (1, sp.num_samples)
            assert np.abs(got - want).max() <= 5e-6
            # a sub-span of the perturbed cut goes through reverse_timestamps
            part_w = sp.truncate(offset=0.25, duration=0.5).load_audio()
            part_g = hip.truncate(offset=0.25, duration=0.5).load_audio()
            assert part_g.shape == part_w.shape and np.abs(part_g - part_w).max() <= 5e-6


def test_kaldifeat_shaped_configs_equal_the_reference_dict_layout(lhotse_mod):
    """HipKaldifeat*Config must (de)serialise exactly like lhotse/features/kaldifeat.py:148-246 (device aside)."""
    import lhotse_amd as LA
    from lhotse.features.kaldifeat import KaldifeatFbankConfig, KaldifeatFrameOptions, KaldifeatMelOptions, KaldifeatMfccConfig

    for ours, theirs in [(LA.HipKaldifeatFbankConfig(), KaldifeatFbankConfig()), (LA.HipKaldifeatMfccConfig(), KaldifeatMfccConfig())]:
        a, b = ours.to_dict(), theirs.to_dict()
        assert a.pop("device") == "cuda" and b.pop("device") == "cpu"
        assert a == b
        # a manifest written by the reference loads into ours and back
        d = theirs.to_dict()
        assert type(ours).from_dict(d).to_dict() == theirs.to_dict()
    fo = KaldifeatFrameOptions(sampling_rate=8000, frame_shift=0.0125, snip_edges=True)
    assert LA.HipKaldifeatFrameOptions.from_dict(fo.to_dict()).to_dict() == fo.to_dict()
    mo = KaldifeatMelOptions(num_bins=64, high_freq=0.0)
    assert LA.HipKaldifeatMelOptions.from_dict(mo.to_dict()).to_dict() == mo.to_dict()
    from lhotse.features import FeatureExtractor

    ex = FeatureExtractor.from_dict({**LA.HipKaldifeatFbankConfig().to_dict(), "feature_type": "hip-kaldifeat-fbank"})
    assert isinstance(ex, LA.HipKaldifeatFbank)


def test_fused_on_the_fly_features_equal_the_reference_strategy(cutset, cpu_device):
    """HipOnTheFlyFeatures (extract + collate fused) vs lhotse's OnTheFlyFeatures(Fbank()): same padded tensor
    (LOG_EPSILON padding), same lengths, same optional outputs."""
    import lhotse_amd as LA
    from lhotse import Fbank
    from lhotse.dataset.input_strategies import OnTheFlyFeatures
    from lhotse.utils import LOG_EPSILON

    assert LA.compat.LOG_EPSILON == LOG_EPSILON
    assert issubclass(LA.HipOnTheFlyFeatures, OnTheFlyFeatures)
    ref_f, ref_l = OnTheFlyFeatures(Fbank())(cutset)
    ours = LA.HipOnTheFlyFeatures(LA.HipFbank(), num_workers=2)
    f, l = ours(cutset)
    assert f.shape == ref_f.shape and f.dtype == torch.float32 and torch.equal(l, ref_l) and l.dtype == ref_l.dtype
    for i, n in enumerate(l.tolist()):
        assert torch.all(f[i, n:] == LOG_EPSILON) and torch.equal(f[i, n:], ref_f[i, n:])
        # valid rows: the reference zero-pads the batch before framing, we reflect per cut -> last rows differ
        assert torch.allclose(f[i, : n - 2], ref_f[i, : n - 2], atol=2e-3)
    # with the reference's edge rule the whole tensor agrees
    f2, _ = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")))(cutset)
    assert torch.allclose(f2, ref_f, atol=2e-3)
    # optional outputs
    f3, l3, a3, al3, c3 = LA.HipOnTheFlyFeatures(LA.HipFbank(), return_audio=True, fault_tolerant=True, return_device="cpu")(cutset)
    assert torch.equal(f3, f) and a3.shape == (5, 32000) and al3.tolist() == [16000, 24000, 12345, 32000, 8000] and len(c3) == 5
    assert ours.supervision_intervals is not None
    with pytest.raises(TypeError):
        LA.HipOnTheFlyFeatures(Fbank())


def test_bulk_save_driver_equals_the_reference_driver(tmp_path, cutset, cpu_device):
    """lhotse_amd.compute_and_store_features_batch (packed archive backend, template manifests, one flush per batch) must
    describe and store what CutSet.compute_and_store_features_batch does: same cuts in the same order, the same Features
    fields (up to where the bytes live), the same arrays through cut.load_features() -- and it must resume like the reference."""
    import lhotse_amd as LA
    from lhotse import CutSet, NumpyFilesWriter
    from lhotse.features.io import get_reader, get_writer

    assert get_writer("hip_archive") is LA.HipArchiveWriter and get_reader("hip_archive") is LA.HipArchiveReader
    ex = LA.HipFbank()
    ref = cutset.compute_and_store_features_batch(extractor=ex, storage_path=tmp_path / "ref", manifest_path=tmp_path / "ref.jsonl.gz",
                                                  batch_duration=3.0, num_workers=0, storage_type=NumpyFilesWriter)
    ours = LA.compute_and_store_features_batch(cutset, extractor=ex, storage_path=tmp_path / "ours", manifest_path=tmp_path / "ours.jsonl.gz",
                                               batch_duration=3.0, num_workers=0)
    ref, ours = list(ref), list(ours)
    assert [c.id for c in ours] == [c.id for c in ref] and len(ours) == 5
    for a, b in zip(ours, ref):
        fa, fb = a.features, b.features
        assert fa.storage_type == "hip_archive" and fa.storage_path.endswith(".hfa")
        assert (fa.type, fa.num_frames, fa.num_features, fa.frame_shift, fa.sampling_rate, fa.start, fa.duration, fa.recording_id, fa.channels) == (
            fb.type, fb.num_frames, fb.num_features, fb.frame_shift, fb.sampling_rate, fb.start, fb.duration, fb.recording_id, fb.channels)
        assert np.array_equal(a.load_features(), b.load_features())
        # the template-built manifest is the dict lhotse's own objects serialise to
        da, db = a.to_dict(), b.to_dict()
        for k in ("storage_type", "storage_path", "storage_key"):
            da["features"].pop(k), db["features"].pop(k)
        assert da == db
        # partial reads (left / right frame offsets) read only their own rows
        full = a.load_features()
        part = a.features.load(start=a.start + 0.2, duration=0.3)
        assert np.array_equal(part, full[20:50])
    # resume: everything is already in the manifest -> nothing is recomputed, same manifest comes back, archive untouched
    size = os.path.getsize(ours[0].features.storage_path)
    again = LA.compute_and_store_features_batch(cutset, extractor=ex, storage_path=tmp_path / "ours", manifest_path=tmp_path / "ours.jsonl.gz",
                                                batch_duration=3.0, num_workers=0)
    assert [c.id for c in again] == [c.id for c in ours] and os.path.getsize(ours[0].features.storage_path) == size
    # any registered writer still works (per-cut writes), in-memory manifests, collated batches
    mem = LA.compute_and_store_features_batch(cutset, extractor=ex, storage_path=tmp_path / "mem", batch_duration=100.0, num_workers=0,
                                              collate=True, storage_type=NumpyFilesWriter, overwrite=True)
    mem = list(mem)
    assert len(mem) == 5 and all(c.has_features for c in mem)
    for a, b in zip(mem, ref):
        assert a.features.storage_type == "numpy_files" and np.allclose(a.load_features(), b.load_features(), atol=2e-3)


def test_a_failing_or_slow_save_thread_stops_or_throttles_the_extractor(tmp_path, cutset, cpu_device, monkeypatch):
    """The save thread runs behind the extractor (as in lhotse/cut/set.py:2365-2404).  A write that fails must stop the run at the next
    batch, not after the whole corpus, and a slow writer must not let finished (page-locked) batches pile up without bound."""
    import threading
    import time

    import lhotse_amd as LA
    import lhotse_amd.storage as S

    calls = {"extracted": 0, "in_flight_max": 0, "written": 0}
    real = S._batch_features_on_host

    def counting(*a, **kw):
        calls["extracted"] += 1
        calls["in_flight_max"] = max(calls["in_flight_max"], calls["extracted"] - calls["written"])
        return real(*a, **kw)

    monkeypatch.setattr(S, "_batch_features_on_host", counting)

    class FailingWriter(LA.HipArchiveWriter):
        name = "hip_archive"

        def write_packed(self, matrix, frames):
            calls["written"] += 1
            raise OSError("No space left on device")

    ex = LA.HipFbank()
    many = cutset + cutset.modify_ids(lambda i: i + "_b") + cutset.modify_ids(lambda i: i + "_c")  # 15 cuts, one per batch below
    with pytest.raises(OSError, match="No space left"):
        LA.compute_and_store_features_batch(many, extractor=ex, storage_path=tmp_path / "full", manifest_path=tmp_path / "full.jsonl.gz",
                                            batch_duration=0.4, num_workers=0, storage_type=FailingWriter)
    assert calls["extracted"] < 15  # stopped early

    calls.update(extracted=0, in_flight_max=0, written=0)
    monkeypatch.setattr(S, "_SAVE_BACKLOG", 2)

    class SlowWriter(LA.HipArchiveWriter):
        name = "hip_archive"

        def write_packed(self, matrix, frames):
            time.sleep(0.05)
            keys = super().write_packed(matrix, frames)
            calls["written"] += 1
            return keys

    out = LA.compute_and_store_features_batch(many, extractor=ex, storage_path=tmp_path / "slow", manifest_path=tmp_path / "slow.jsonl.gz",
                                              batch_duration=0.4, num_workers=0, storage_type=SlowWriter)
    assert len(list(out)) == 15 and calls["written"] == 15
    assert calls["in_flight_max"] <= 2 + 2  # backlog + the batch being written + the one being extracted


def test_template_manifests_behind_lazy_cuts_and_loader_workers(tmp_path, cutset, cpu_device):
    """with lazily loaded cuts (fresh Recording objects per batch, addresses reused by CPython) and DataLoader workers the
    per-recording cache of the template path must never hand one cut another cut's recording, and the template path must be the one
    that runs behind lhotse's sampler (which attaches a `dataloading_info` custom field to every cut)."""
    import lhotse_amd as LA
    from lhotse import CutSet, NumpyFilesWriter

    many = CutSet.from_cuts(c.with_id(f"{c.id}-{k}") for k in range(8) for c in cutset)  # 40 cuts over 5 recordings
    many.to_file(tmp_path / "in.jsonl.gz")
    lazy = CutSet.from_jsonl_lazy(tmp_path / "in.jsonl.gz")
    ex = LA.HipFbank()
    ref = list(lazy.compute_and_store_features_batch(extractor=ex, storage_path=tmp_path / "ref", manifest_path=tmp_path / "ref.jsonl.gz",
                                                     batch_duration=2.0, num_workers=1, storage_type=NumpyFilesWriter))
    before = dict(LA.storage.TEMPLATE_STATS)
    ours = list(LA.compute_and_store_features_batch(lazy, extractor=ex, storage_path=tmp_path / "ours", manifest_path=tmp_path / "ours.jsonl.gz",
                                                    batch_duration=2.0, num_workers=1))
    assert LA.storage.TEMPLATE_STATS["template"] - before["template"] == 40 and LA.storage.TEMPLATE_STATS["fallback"] == before["fallback"]
    assert [c.id for c in ours] == [c.id for c in ref] and len(ours) == 40
    for a, b in zip(ours, ref):
        da, db = a.to_dict(), b.to_dict()
        for k in ("storage_type", "storage_path", "storage_key"):
            da["features"].pop(k), db["features"].pop(k)
        assert da == db and da["recording"]["id"] == a.id.split("-")[0].replace("cut", "rec")
        assert da["custom"]["dataloading_info"]["world_size"] == 1
        assert np.array_equal(a.load_features(), b.load_features())
    # a custom field that is itself a manifest goes through lhotse's own serialiser
    c0 = many[0]
    c0.custom = {"other_recording": c0.recording}
    LA.compute_and_store_features_batch(CutSet.from_cuts([c0]), extractor=ex, storage_path=tmp_path / "c", manifest_path=tmp_path / "c.jsonl.gz",
                                        num_workers=0)
    assert LA.storage.TEMPLATE_STATS["fallback"] == before["fallback"] + 1
    back = list(CutSet.from_file(tmp_path / "c.jsonl.gz"))[0]
    assert back.custom["other_recording"].id == c0.recording.id and back.has_features


def test_archive_backend_round_trip_without_lhotse_objects(tmp_path):
    """The archive itself: packed batch appends, self-describing keys, positioned partial reads, append mode."""
    import lhotse_amd as LA

    rs = np.random.RandomState(0)
    mats = [rs.rand(t, 7).astype(np.float32) for t in (5, 1, 40, 13)]
    with LA.HipArchiveWriter(tmp_path / "feats") as w:
        k0 = w.write("a", mats[0])
        ks = w.write_packed(np.concatenate(mats[1:]), [m.shape[0] for m in mats[1:]])
        path = w.storage_path
    assert path.endswith(".hfa") and os.path.getsize(path) == sum(m.nbytes for m in mats)
    r = LA.HipArchiveReader(tmp_path / "feats")
    for k, m in zip([k0] + ks, mats):
        assert np.array_equal(r.read(k), m)
    assert np.array_equal(r.read(ks[1], left_offset_frames=3, right_offset_frames=11), mats[2][3:11])
    assert r.read(ks[1], left_offset_frames=50).shape == (0, 7)
    with LA.HipArchiveWriter(tmp_path / "feats", mode="a") as w:  # resume appends behind what is there
        k4 = w.write("e", mats[0] * 2)
    assert k4.startswith(str(sum(m.nbytes for m in mats)) + ":") and np.array_equal(LA.HipArchiveReader(path).read(k4), mats[0] * 2)


def test_half_precision_archive(tmp_path, cutset, cpu_device):
    """`hip_archive_f16`: binary16 rows (the reference's default storage, lilcom, is lossy too: its shipped fixture is exact to 2^-6);
    written through the same driver, read back as float32 by lhotse's own `Features.load` -- whole and partial reads."""
    import lhotse_amd as LA
    from lhotse.features.io import get_reader, get_writer

    assert get_writer("hip_archive_f16") is LA.HipArchiveF16Writer and get_reader("hip_archive_f16").name == "hip_archive_f16"
    ex = LA.HipFbank()
    full = list(LA.compute_and_store_features_batch(cutset, extractor=ex, storage_path=tmp_path / "f32", manifest_path=tmp_path / "f32.jsonl.gz",
                                                    batch_duration=3.0, num_workers=0))
    half = list(LA.compute_and_store_features_batch(cutset, extractor=ex, storage_path=tmp_path / "f16", manifest_path=tmp_path / "f16.jsonl.gz",
                                                    batch_duration=3.0, num_workers=0, storage_type=LA.HipArchiveF16Writer))
    assert [c.id for c in half] == [c.id for c in full]
    for a, b in zip(half, full):
        assert a.features.storage_type == "hip_archive_f16" and a.features.storage_key.endswith(":f16")
        x, y = a.load_features(), b.load_features()
        assert x.dtype == np.float32 and x.shape == y.shape
        assert np.array_equal(x, y.astype(np.float16).astype(np.float32))  # exactly the binary16 rounding of the float32 features
        assert np.abs(x - y).max() <= 2.0 ** -6
        assert np.array_equal(a.features.load(start=a.start + 0.2, duration=0.3), x[20:50])
    assert os.path.getsize(half[0].features.storage_path) * 2 == os.path.getsize(full[0].features.storage_path)
    # binary16 holds log-domain features only -- a linear-domain extractor is refused up front, and values that are not finite
    # in binary16 (|x| > 65504) never reach the file
    with pytest.raises(ValueError, match="linear-domain output of 'hip-spectrogram'"):
        LA.compute_and_store_features_batch(cutset, extractor=LA.HipSpectrogram(), storage_path=tmp_path / "bad", manifest_path=tmp_path / "bad.jsonl.gz",
                                            batch_duration=3.0, num_workers=0, storage_type=LA.HipArchiveF16Writer)
    with LA.HipArchiveF16Writer(tmp_path / "range") as w:
        ok = w.write("a", np.float32([[65504.0, -65504.0, 1e-9]]))
        with pytest.raises(ValueError, match="not finite in binary16"):
            w.write("b", np.float32([[1.0, 7e4, 0.0]]))
        with pytest.raises(ValueError, match="not finite in binary16"):
            w.write_packed(np.float16([[np.inf, 0.0]]), [1])
        assert w.write("c", np.float32([[2.0, 3.0, 4.0]])) == "6:1:3:f16"  # the refused batches left nothing behind
    assert ok == "0:1:3:f16"


LAYER_PAIRS = [("HipWav2Spec", "Wav2Spec"), ("HipWav2LogSpec", "Wav2LogSpec"), ("HipWav2LogFilterBank", "Wav2LogFilterBank"), ("HipWav2MFCC", "Wav2MFCC")]


@pytest.mark.parametrize("ours,theirs", LAYER_PAIRS)
def test_layer_modules_have_the_reference_constructors(lhotse_mod, ours, theirs):
    import inspect

    import lhotse.features.kaldi.layers as RL
    import lhotse_amd.layers as HL

    a, b = inspect.signature(getattr(HL, ours).__init__), inspect.signature(getattr(RL, theirs).__init__)
    assert [(p.name, p.default) for p in a.parameters.values()] == [(p.name, p.default) for p in b.parameters.values()]
    m = getattr(HL, ours)()
    r = getattr(RL, theirs)()
    for attr in ("sampling_rate", "frame_length", "frame_shift", "remove_dc_offset", "preemph_coeff", "window_type", "dither", "snip_edges",
                 "energy_floor", "raw_energy", "use_energy", "fft_length"):
        if hasattr(r, attr):
            assert getattr(m, attr) == getattr(r, attr), attr


@pytest.mark.parametrize("ours,theirs,kw", [
    ("HipWav2LogFilterBank", "Wav2LogFilterBank", {}),
    ("HipWav2LogFilterBank", "Wav2LogFilterBank", {"use_energy": True, "num_filters": 40, "snip_edges": True}),
    ("HipWav2MFCC", "Wav2MFCC", {}),
    ("HipWav2Spec", "Wav2Spec", {}),
    ("HipWav2LogSpec", "Wav2LogSpec", {"use_energy": False, "sampling_rate": 8000}),
])
def test_layer_forward_equals_the_reference_layer(lhotse_mod, cpu_device, ours, theirs, kw):
    import lhotse.features.kaldi.layers as RL
    import lhotse_amd.layers as HL

    x = torch.from_numpy((np.random.RandomState(5).rand(3, 4000).astype(np.float32) - 0.5))
    with torch.no_grad():
        want = getattr(RL, theirs)(**kw)(x).numpy()
    layer = getattr(HL, ours)(**kw)
    got = layer(x).numpy()
    assert got.shape == want.shape
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 2e-4 * max(1.0, scale)
    assert layer(x[0]).shape == want.shape[1:]  # (T,) in -> (frames, F) out
    with pytest.raises(NotImplementedError, match="inference-only"):
        layer(x.clone().requires_grad_(True))
    with pytest.raises(TypeError):
        layer(x.double())


def test_on_the_fly_features_with_speed_perturbed_cuts(cutset, cpu_device, monkeypatch):
    """PerturbSpeed-ed cuts through HipOnTheFlyFeatures: the Speed transform of eligible cuts is applied to the packed batch (on the
    device; here: an oracle-backed stand-in of the resampler) instead of inside Recording.load_audio -- same features, same lengths,
    same padded audio as the reference strategy over lhotse's own CPU Speed (lhotse/audio/recording.py:431-490)."""
    import lhotse_amd as LA
    import lhotse_amd.input_strategies as IS
    from lhotse import CutSet
    from lhotse.dataset import OnTheFlyFeatures
    from lhotse.features import Fbank
    from lhotse.utils import LOG_EPSILON
    from oracle import resample_ref as R

    def cpu_perturb(arena, offsets, lengths, factors, sampling_rate, tail_start):  # perturb_speed_in_arena on the host
        offsets, lengths = np.asarray(offsets, dtype=np.int64).copy(), np.asarray(lengths, dtype=np.int64).copy()
        tail = (int(tail_start) + 3) & ~3
        for i, f in enumerate(factors):
            if f == 1.0:
                continue
            y = R.speed(arena[int(offsets[i]) : int(offsets[i]) + int(lengths[i])].numpy(), sampling_rate, float(f))
            arena[tail : tail + len(y)] = torch.from_numpy(y)
            offsets[i], lengths[i] = tail, len(y)
            tail = (tail + len(y) + 3) & ~3
        return offsets, lengths

    monkeypatch.setattr(IS, "_perturb_in_arena", cpu_perturb)
    calls = {"raw": 0}
    real_read = IS.read_before_chain
    monkeypatch.setattr(IS, "read_before_chain", lambda cut: (calls.__setitem__("raw", calls["raw"] + 1), real_read(cut))[1])

    mixed = CutSet.from_cuts(list(cutset.perturb_speed(1.1)) + list(cutset) + list(cutset.perturb_speed(0.9))
                             + [c.truncate(offset=0.13, duration=0.41) for c in cutset.perturb_speed(0.9)][:2])
    ref_f, ref_l, ref_a, ref_al = OnTheFlyFeatures(Fbank(), return_audio=True)(mixed)
    f, l, a, al = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), return_audio=True, num_workers=2)(mixed)
    assert calls["raw"] == 12  # every speed-perturbed cut was read WITHOUT its transform
    assert torch.equal(l, ref_l) and torch.equal(al, ref_al) and f.shape == ref_f.shape and a.shape == ref_a.shape
    assert torch.allclose(a, ref_a, atol=1e-5)  # the resampler's summation order only
    assert torch.allclose(f, ref_f, atol=5e-3)
    for i, n in enumerate(l.tolist()):
        assert torch.all(f[i, n:] == LOG_EPSILON)
    # switched off, or with wave transforms, the reference's own loading path is taken
    f2, l2 = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), gpu_speed_perturb=False)(mixed)
    assert calls["raw"] == 12 and torch.equal(l2, ref_l) and torch.allclose(f2, ref_f, atol=2e-3)
    # wave_transforms run on the LOADED samples: by default (gpu_speed_perturb=None) the strategy then behaves like the reference one
    # (CPU Speed inside load_audio, then the transforms) -- what worked with OnTheFlyFeatures keeps working
    f3, l3 = LA.HipOnTheFlyFeatures(LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")), wave_transforms=[lambda x: x])(mixed)
    assert calls["raw"] == 12 and torch.equal(l3, ref_l) and torch.allclose(f3, ref_f, atol=2e-3)
    with pytest.raises(ValueError, match="gpu_speed_perturb=True was requested together with wave_transforms"):  # only the explicit contradiction
        LA.HipOnTheFlyFeatures(LA.HipFbank(), wave_transforms=[lambda x: x], gpu_speed_perturb=True)(mixed)
    # cuts whose recording carries anything but exactly one Speed are not touched
    speed_only = lambda cut: IS.parse_chain(cut, gpu_reverb=False, gpu_resample=False, gpu_level=False)  # noqa: E731  (the other routes off)
    assert not speed_only(list(cutset)[0]).pending
    assert speed_only(list(cutset.perturb_speed(1.1).perturb_volume(2.0))[0]) is None
    assert speed_only(list(cutset.perturb_speed(1.1))[0]) == IS.Chain(factor=1.1)


def _lines(path):
    import gzip

    with gzip.open(path, "rt", encoding="utf-8") as f:
        return [ln.rstrip("\n") for ln in f]


def test_native_manifest_lines_equal_the_per_cut_path_byte_for_byte(tmp_path, cutset, cpu_device):
    """Round 5 (VERDICT r4 task 4): the manifest of the native path -- line halves made where the cuts are loaded, keys spliced in by
    libhipfeat's hipfeat_manifest_lines -- is the per-cut Python path's manifest character for character (storage_path apart), with
    and without loader workers, with supervisions that hold non-ASCII text and with lhotse's own `dataloading_info` custom field;
    the archive bytes are the same bytes; stripes spread them over several files that lhotse's readers follow per cut."""
    import lhotse_amd as LA
    from lhotse import CutSet, SupervisionSegment

    cuts = []
    for k in range(4):
        for c in cutset:
            c = c.with_id(f"{c.id}-{k}")
            c.supervisions = [SupervisionSegment(id=c.id, recording_id=c.recording_id, start=0.0, duration=c.duration, text=f"zażółć gęślą jaźń \"{k}\" \\ ü",
                                                 speaker=f"spk{k}", language="pl")]
            cuts.append(c)
    many = CutSet.from_cuts(cuts)  # 20 cuts
    ex = LA.HipFbank()

    class PerCut(LA.HipArchiveWriter):  # a subclass is served through the generic per-cut path (its own write_packed)
        name = "hip_archive"

    plain = list(LA.compute_and_store_features_batch(many, ex, tmp_path / "plain", manifest_path=tmp_path / "plain.jsonl.gz", batch_duration=4.0,
                                                     num_workers=0, storage_type=PerCut))
    want = _lines(tmp_path / "plain.jsonl.gz")
    assert len(want) == 20
    for tag, workers, stripes in (("w0", 0, 1), ("w2", 2, 1), ("s3", 1, 3)):
        before = dict(LA.storage.TEMPLATE_STATS)
        got_cuts = list(LA.compute_and_store_features_batch(many, ex, tmp_path / tag, manifest_path=tmp_path / f"{tag}.jsonl.gz", batch_duration=4.0,
                                                            num_workers=workers, archive_stripes=stripes))
        assert LA.storage.TEMPLATE_STATS.get("native", 0) - before.get("native", 0) == 20, tag  # every line came out of the C splice
        got = _lines(tmp_path / f"{tag}.jsonl.gz")
        if stripes == 1:
            assert [ln.replace(str(tmp_path / tag) + ".hfa", str(tmp_path / "plain") + ".hfa") for ln in got] == want, tag
            assert (tmp_path / f"{tag}.hfa").read_bytes() == (tmp_path / "plain.hfa").read_bytes()
        else:
            files = {c.features.storage_path for c in got_cuts}
            assert files == {str(tmp_path / "s3.hfa"), str(tmp_path / "s3.1.hfa"), str(tmp_path / "s3.2.hfa")}
            assert sum(os.path.getsize(f) for f in files) == os.path.getsize(tmp_path / "plain.hfa")
        for a, b in zip(got_cuts, plain):
            assert a.id == b.id and a.supervisions[0].text == b.supervisions[0].text and np.array_equal(a.load_features(), b.load_features())
    # the loader-side dataset is a module-level class: an instance survives pickling (spawned DataLoader workers)
    import pickle

    import lhotse_amd.storage as S

    ds = S.FragmentingWaveformDataset(False, {"type": "hip-fbank", "num_features": 80, "frame_shift": 0.01, "sampling_rate": 16000, "storage_type": "hip_archive",
                                              "storage_path": "x"}, 0.01)
    back = pickle.loads(pickle.dumps(ds))
    got = back[CutSet.from_cuts(cuts[:3])]
    assert len(got["hipfeat_fragments"]) == 3 and all(f is not None and f[2] == S.expected_num_frames(c.duration, 0.01, 16000) for f, c in zip(got["hipfeat_fragments"], cuts[:3]))
    # resume into a striped archive: nothing is extracted twice, the files do not move
    sizes = {f: os.path.getsize(f) for f in (tmp_path / "s3.hfa", tmp_path / "s3.1.hfa", tmp_path / "s3.2.hfa")}
    again = list(LA.compute_and_store_features_batch(many, ex, tmp_path / "s3", manifest_path=tmp_path / "s3.jsonl.gz", batch_duration=4.0, num_workers=0,
                                                     archive_stripes=3))
    assert [c.id for c in again] == [c.id for c in plain] and sizes == {f: os.path.getsize(f) for f in sizes}


def test_native_path_enforces_the_frame_count_contract_and_stops_on_write_errors(tmp_path, cutset, cpu_device, monkeypatch):
    """validate_features' contract (lhotse/qa.py:286-301) is checked inside hipfeat_manifest_lines on the extractor's ACTUAL frame counts;
    a failing archive append stops the run at the next batch."""
    import lhotse_amd as LA
    import lhotse_amd.storage as S

    ex = LA.HipFbank()
    real = S.expected_num_frames
    monkeypatch.setattr(S, "expected_num_frames", lambda d, fs, sr: real(d, fs, sr) + (1 if abs(d - 2.0) < 1e-9 else 0))  # the 32000-sample cut
    with pytest.raises(AssertionError, match="frame-count contract"):
        LA.compute_and_store_features_batch(cutset, ex, tmp_path / "bad", manifest_path=tmp_path / "bad.jsonl.gz", batch_duration=10.0, num_workers=0)
    monkeypatch.setattr(S, "expected_num_frames", real)
    calls = {"n": 0}

    def full(self, matrix, frames):
        calls["n"] += 1
        raise OSError("No space left on device")

    monkeypatch.setattr(S.NativeArchive, "append", full)
    many = cutset + cutset.modify_ids(lambda i: i + "_b") + cutset.modify_ids(lambda i: i + "_c")
    with pytest.raises(OSError, match="No space left"):
        LA.compute_and_store_features_batch(many, ex, tmp_path / "full", manifest_path=tmp_path / "full.jsonl.gz", batch_duration=0.4, num_workers=0)
    assert calls["n"] < 15


def test_loader_workers_hand_over_one_packed_tensor_per_batch(tmp_path, cutset, cpu_device):
    """Round 6: the product's waveform dataset packs an un-collated batch into ONE float32 tensor inside the DataLoader worker (one
    shared-memory segment per batch instead of one per cut: the transport, not decoding, bounded the batch driver); the main process
    extracts from 1-D views of it.  Same features, same manifests as the per-cut arrays -- and an augment_fn keeps the per-cut arrays."""
    import lhotse_amd as LA
    from lhotse_amd import storage as S

    ds = S.FragmentingWaveformDataset(False, None, 0.01)
    batch = ds[cutset]
    assert isinstance(batch["audio"], torch.Tensor) and batch["audio"].ndim == 1 and batch["audio"].dtype == torch.float32
    lens = batch["hipfeat_lens"].tolist()
    assert lens == [c.num_samples for c in cutset]
    views = S.unpack_batch_audio(batch)
    for v, c in zip(views, cutset):
        assert v.data_ptr() % 16 == 0 and np.array_equal(v.numpy(), c.load_audio()[0])
    plain = S.FragmentingWaveformDataset(False, None, 0.01, pack=False)[cutset]
    assert isinstance(plain["audio"], list) and "hipfeat_lens" not in plain and S.unpack_batch_audio(plain) is plain["audio"]
    ex = LA.HipFbank(LA.HipFbankConfig(device="cpu"))
    a = S.compute_and_store_features_batch(cutset, ex, tmp_path / "a", manifest_path=tmp_path / "a.jsonl.gz", batch_duration=3.0, num_workers=2,
                                           loader="dataloader")
    b = S.compute_and_store_features_batch(cutset, ex, tmp_path / "b", manifest_path=tmp_path / "b.jsonl.gz", batch_duration=3.0, num_workers=2,
                                           augment_fn=lambda w, sr: w)
    fa, fb = {c.id: c.load_features() for c in a}, {c.id: c.load_features() for c in b}
    assert sorted(fa) == sorted(fb) == sorted(c.id for c in cutset)
    for k in fa:
        assert np.array_equal(fa[k], fb[k]) and np.array_equal(fa[k], ex.extract(cutset[k].load_audio(), 16000))


def test_the_batch_driver_starts_its_workers_through_a_fork_server_when_the_gpu_is_already_in_use(tmp_path, cutset, cpu_device, monkeypatch):
    """Round 6 (profiles/r06_loader_pipeline_probe.txt): DataLoader workers FORKED off a process with a live HIP context slow that process's
    device round trips by ~30 ms each.  The product's driver therefore asks for a fork server when `_lib.hip_live()`, says so, and keeps
    torch's default otherwise / on request."""
    import torch.utils.data as tud

    import lhotse_amd as LA
    from lhotse_amd import _lib
    from lhotse_amd import storage as S

    seen = []
    real = tud.DataLoader

    class Spy(real):
        def __init__(self, *a, **k):
            seen.append({x: k[x] for x in ("multiprocessing_context", "worker_init_fn") if x in k})
            k.pop("multiprocessing_context", None)  # (the stub modules this container needs to import lhotse do not exist in a fork server's children)
            super().__init__(*a, **k)

    monkeypatch.setattr(tud, "DataLoader", Spy)
    ex = LA.HipFbank(LA.HipFbankConfig(device="cpu"))
    kw = dict(batch_duration=3.0, num_workers=2, loader="dataloader")
    monkeypatch.setattr(_lib, "hip_live", lambda: False)
    S.compute_and_store_features_batch(cutset, ex, tmp_path / "a", manifest_path=tmp_path / "a.jsonl.gz", **kw)
    assert seen[-1] == {}
    monkeypatch.setattr(_lib, "hip_live", lambda: True)
    init = lambda wid: None  # noqa: E731
    with pytest.warns(RuntimeWarning, match="fork server"):
        S.compute_and_store_features_batch(cutset, ex, tmp_path / "b", manifest_path=tmp_path / "b.jsonl.gz", worker_init_fn=init, **kw)
    assert seen[-1] == {"multiprocessing_context": "forkserver", "worker_init_fn": init}
    S.compute_and_store_features_batch(cutset, ex, tmp_path / "c", manifest_path=tmp_path / "c.jsonl.gz", loader_start_method="fork", **kw)
    assert seen[-1] == {}
    S.compute_and_store_features_batch(cutset, ex, tmp_path / "d", manifest_path=tmp_path / "d.jsonl.gz", batch_duration=3.0, num_workers=0)
    assert seen[-1] == {}
    # the ring loader (the default where it applies) takes the same decision
    import lhotse_amd.ring_loader as R

    started = []
    real_ring = R.RingLoader

    class SpyRing(real_ring):
        def __init__(self, *a, **k):
            started.append((k.get("start_method"), k.get("worker_init_fn")))
            k["start_method"] = "fork"  # (as above: no stub modules behind a fork server in this container)
            super().__init__(*a, **k)

    monkeypatch.setattr(R, "RingLoader", SpyRing)
    with pytest.warns(RuntimeWarning, match="fork server"):
        S.compute_and_store_features_batch(cutset, ex, tmp_path / "e", manifest_path=tmp_path / "e.jsonl.gz", batch_duration=3.0, num_workers=2, worker_init_fn=init)
    assert started[-1] == ("forkserver", init)
    monkeypatch.setattr(_lib, "hip_live", lambda: False)
    S.compute_and_store_features_batch(cutset, ex, tmp_path / "f", manifest_path=tmp_path / "f.jsonl.gz", batch_duration=3.0, num_workers=2)
    assert started[-1] == (None, None) and len(seen) == 4  # (no DataLoader was built for the two ring runs)


def test_forking_with_a_live_context_warns_once(monkeypatch):
    import os

    from lhotse_amd import _lib

    monkeypatch.setattr(_lib, "hip_live", lambda: True)
    monkeypatch.setattr(_lib, "_FORK_WARNED", False)
    with pytest.warns(RuntimeWarning, match="live HIP context"):
        pid = os.fork()
        if pid == 0:
            os._exit(0)
        os.waitpid(pid, 0)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pid = os.fork()  # a second fork: silent
        if pid == 0:
            os._exit(0)
        os.waitpid(pid, 0)


def test_ring_loader_behind_the_batch_driver_equals_the_dataloader(tmp_path, cutset, cpu_device, monkeypatch):
    """Round 6: `loader="ring"` (the default where it applies) -- worker processes load every batch's audio straight into a slot of one
    shared-memory ring (lhotse_amd/ring_loader.py + storage.LoadCutsIntoSlot) -- gives the DataLoader route's manifest character for
    character and the same archive bytes; cuts whose audio fails to load are dropped with lhotse's warning as
    UnsupervisedWaveformDataset drops them (lhotse/dataset/unsupervised.py:72-78); a batch that does not fit a slot travels by pickle;
    where the ring does not apply the DataLoader is used, and asking for it there is an error."""
    import lhotse_amd as LA
    import lhotse_amd.ring_loader as R
    from lhotse import CutSet, MonoCut, Recording, SupervisionSegment
    from lhotse.audio import AudioSource
    from lhotse_amd import storage as S

    cuts = []
    for k in range(5):
        for c in cutset:
            c = c.with_id(f"{c.id}-{k}")
            c.supervisions = [SupervisionSegment(id=c.id, recording_id=c.recording_id, start=0.0, duration=c.duration, text=f"gęślą \"{k}\"", speaker=f"s{k}")]
            cuts.append(c)
    # one cut whose file holds half of what its manifest states: dropped by both loaders (DurationMismatchError is one of the errors
    # suppress_audio_loading_errors swallows, lhotse/audio/utils.py:126-138)
    ghost = Recording(id="ghost", sources=[AudioSource(type="file", channels=[0], source=str(tmp_path / "r0.wav"))], sampling_rate=16000, num_samples=32000, duration=2.0)
    cuts.insert(7, MonoCut(id="ghost-cut", start=0, duration=2.0, channel=0, recording=ghost))
    many = CutSet.from_cuts(cuts)
    ex = LA.HipFbank(LA.HipFbankConfig(device="cpu"))
    kw = dict(batch_duration=4.0, num_workers=2)
    want_cuts = list(S.compute_and_store_features_batch(many, ex, tmp_path / "dl", manifest_path=tmp_path / "dl.jsonl.gz", loader="dataloader", **kw))
    want = _lines(tmp_path / "dl.jsonl.gz")
    assert len(want) == 25 and "ghost-cut" not in {c.id for c in want_cuts}

    made = []
    real = R.RingLoader

    class Spy(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(R, "RingLoader", Spy)
    for tag, extra in (("ring", dict(loader="ring")), ("auto", {}), ("s2", dict(archive_stripes=2))):
        before = dict(S.TEMPLATE_STATS)
        got_cuts = list(S.compute_and_store_features_batch(many, ex, tmp_path / tag, manifest_path=tmp_path / f"{tag}.jsonl.gz", **kw, **extra))
        assert S.TEMPLATE_STATS.get("native", 0) - before.get("native", 0) == 25, tag
        assert len(made) > 0 and made[-1]._closed and not any(p.is_alive() for p in made[-1]._procs), tag
        got = _lines(tmp_path / f"{tag}.jsonl.gz")
        if "archive_stripes" not in extra:
            assert [ln.replace(str(tmp_path / tag) + ".hfa", str(tmp_path / "dl") + ".hfa") for ln in got] == want, tag
            assert (tmp_path / f"{tag}.hfa").read_bytes() == (tmp_path / "dl.hfa").read_bytes(), tag
        assert [c.id for c in got_cuts] == [c.id for c in want_cuts]
        for a, b in zip(got_cuts, want_cuts):
            assert np.array_equal(a.load_features(), b.load_features())
    assert len(made) == 3
    # resume through the ring: nothing is extracted twice
    size = os.path.getsize(tmp_path / "ring.hfa")
    again = list(S.compute_and_store_features_batch(many, ex, tmp_path / "ring", manifest_path=tmp_path / "ring.jsonl.gz", loader="ring", **kw))
    assert [c.id for c in again] == [c.id for c in want_cuts] and os.path.getsize(tmp_path / "ring.hfa") == size
    # a batch that does not fit its slot (here: every batch -- the slots are made tiny) still arrives, by pickle
    class Tiny(real):
        def __init__(self, load_batch, num_workers, slot_bytes, num_slots=None, **k):
            super().__init__(load_batch, num_workers, 4096, num_slots, **k)

    monkeypatch.setattr(R, "RingLoader", Tiny)
    S.compute_and_store_features_batch(many, ex, tmp_path / "tiny", manifest_path=tmp_path / "tiny.jsonl.gz", loader="ring", **kw)
    assert (tmp_path / "tiny.hfa").read_bytes() == (tmp_path / "dl.hfa").read_bytes()
    monkeypatch.setattr(R, "RingLoader", Spy)
    # where it does not apply
    n = len(made)
    S.compute_and_store_features_batch(many, ex, tmp_path / "aug", manifest_path=tmp_path / "aug.jsonl.gz", augment_fn=lambda w, sr: w, **kw)
    clean = CutSet.from_cuts(c for c in cuts if c.id != "ghost-cut")  # (collate_audio is not fault tolerant: lhotse/dataset/collation.py:207)
    S.compute_and_store_features_batch(clean, ex, tmp_path / "col", manifest_path=tmp_path / "col.jsonl.gz", collate=True, **kw)
    S.compute_and_store_features_batch(many, ex, tmp_path / "w0", manifest_path=tmp_path / "w0.jsonl.gz", batch_duration=4.0, num_workers=0)
    assert len(made) == n
    for bad in (dict(collate=True), dict(augment_fn=lambda w, sr: w), dict(num_workers=0)):
        with pytest.raises(ValueError, match="loader='ring' serves"):
            S.compute_and_store_features_batch(many, ex, tmp_path / "x", manifest_path=tmp_path / "x.jsonl.gz", loader="ring", **{**kw, **bad})
    with pytest.raises(ValueError, match="expected None"):
        S.compute_and_store_features_batch(many, ex, tmp_path / "x", manifest_path=tmp_path / "x.jsonl.gz", loader="queue", **kw)
    # /dev/shm too small: the default falls back to the DataLoader with a warning, an explicit request raises
    monkeypatch.setattr(S, "_shm_free_bytes", lambda: 1 << 20)
    with pytest.warns(RuntimeWarning, match="using the DataLoader"):
        S.compute_and_store_features_batch(many, ex, tmp_path / "small", manifest_path=tmp_path / "small.jsonl.gz", **kw)
    assert (tmp_path / "small.hfa").read_bytes() == (tmp_path / "dl.hfa").read_bytes()
    with pytest.raises(OSError, match="/dev/shm"):
        S.compute_and_store_features_batch(many, ex, tmp_path / "small2", manifest_path=tmp_path / "small2.jsonl.gz", loader="ring", **kw)


def test_ring_loader_serves_lhotse_s_own_storage_types_too(tmp_path, cutset, cpu_device, monkeypatch):
    """The ring is a transport: with lhotse's own writers (NumpyFilesWriter here: one .npy per cut, manifests through Python objects) the
    driver stores the same arrays under the same manifest lines as behind the DataLoader -- and really uses the ring."""
    import lhotse_amd as LA
    import lhotse_amd.ring_loader as R
    from lhotse import CutSet
    from lhotse.features.io import NumpyFilesWriter
    from lhotse_amd import storage as S

    cuts = [c.with_id(f"{c.id}-{k}") for k in range(3) for c in cutset]
    many = CutSet.from_cuts(cuts)
    ex = LA.HipFbank(LA.HipFbankConfig(device="cpu"))
    made = []
    real = R.RingLoader

    class Spy(real):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(R, "RingLoader", Spy)
    kw = dict(batch_duration=4.0, num_workers=2, storage_type=NumpyFilesWriter)
    a = list(S.compute_and_store_features_batch(many, ex, tmp_path / "dl", manifest_path=tmp_path / "dl.jsonl.gz", loader="dataloader", **kw))
    assert made == []
    b = list(S.compute_and_store_features_batch(many, ex, tmp_path / "ring", manifest_path=tmp_path / "ring.jsonl.gz", **kw))
    assert len(made) == 1 and made[0]._closed
    assert [c.id for c in a] == [c.id for c in b] == [c.id for c in cuts]
    for x, y in zip(a, b):
        assert x.features.storage_type == y.features.storage_type == "numpy_files" and x.features.storage_key == y.features.storage_key
        assert np.array_equal(x.load_features(), y.load_features())
    assert [ln.replace(str(tmp_path / "ring"), "@") for ln in _lines(tmp_path / "ring.jsonl.gz")] == [ln.replace(str(tmp_path / "dl"), "@") for ln in _lines(tmp_path / "dl.jsonl.gz")]
    # without a manifest path (an in-memory CutSet comes back), still through the ring
    c = S.compute_and_store_features_batch(many, ex, tmp_path / "mem", batch_duration=4.0, num_workers=2, storage_type=NumpyFilesWriter)
    assert len(made) == 2 and [x.id for x in c] == [x.id for x in cuts]


def test_pcm16_wav_route_of_the_ring_loader(tmp_path, cutset, cpu_device, lhotse_mod):
    """`wav_pcm16=True`: a batch whose cuts are all plain mono 16-bit PCM .wav segments is read as int16 straight into the ring slot (the device
    converts x / 32768, exact); `pcm16_wav_segment` gives exactly the samples of which `cut.load_audio()` returns x / 32768 -- whole
    recordings and sub-segments -- and declines everything lhotse would have to fix up, transform, mix or refuse; the driver then stores
    the same bytes under the same manifest lines as the float32 route."""
    import lhotse_amd as LA
    from lhotse import CutSet, MonoCut, Recording
    from lhotse.audio import AudioSource
    from lhotse_amd import storage as S

    cuts = list(cutset)
    for c in cuts:
        x = S.pcm16_wav_segment(c, MonoCut)
        assert x is not None and x.dtype == np.int16 and np.array_equal(x.astype(np.float32) / 32768.0, c.load_audio()[0])
    sub = cuts[3].truncate(offset=0.25, duration=1.0)  # a sub-segment of the 2 s recording
    x = S.pcm16_wav_segment(sub, MonoCut)
    assert x is not None and x.shape == (16000,) and np.array_equal(x.astype(np.float32) / 32768.0, sub.load_audio()[0])
    tail = cuts[2].truncate(offset=0.5)  # up to the (odd-length) end
    assert np.array_equal(S.pcm16_wav_segment(tail, MonoCut).astype(np.float32) / 32768.0, tail.load_audio()[0])
    # declined: a speed-perturbed cut (transforms), a recording whose manifest overstates the file, a padded cut (not a MonoCut)
    assert S.pcm16_wav_segment(cuts[0].perturb_speed(1.1), MonoCut) is None
    ghost = Recording(id="ghost", sources=[AudioSource(type="file", channels=[0], source=cuts[0].recording.sources[0].source)], sampling_rate=16000, num_samples=32000, duration=2.0)
    assert S.pcm16_wav_segment(MonoCut(id="g", start=0, duration=2.0, channel=0, recording=ghost), MonoCut) is None
    assert S.pcm16_wav_segment(cuts[0].pad(duration=3.0), MonoCut) is None
    # the worker side: an all-WAV batch arrives as int16, a batch with one declined cut takes lhotse's route (float32) as a whole
    out = np.zeros(1 << 20, dtype=np.uint8)
    load = S.LoadCutsIntoSlot(None, 0.01, pcm16=True)
    used, meta = load(cuts[:3], out)
    assert meta["pcm16"] is True and meta["kept"] == [0, 1, 2] and meta["lens"].tolist() == [c.num_samples for c in cuts[:3]]
    flat = out[:used].view(np.int16)
    for c, o, n in zip(cuts[:3], meta["offs"].tolist(), meta["lens"].tolist()):
        assert o % 8 == 0 and np.array_equal(flat[o : o + n].astype(np.float32) / 32768.0, c.load_audio()[0])
    used, meta = load([cuts[0], cuts[1].perturb_speed(0.9)], out)
    assert "pcm16" not in meta and np.array_equal(out[:used].view(np.float32)[: cuts[0].num_samples], cuts[0].load_audio()[0])
    # the driver: same manifests, same archive bytes
    many = CutSet.from_cuts([c.with_id(f"{c.id}-{k}") for k in range(3) for c in cuts] + [sub.with_id("sub")])
    ex = LA.HipFbank(LA.HipFbankConfig(device="cpu"))
    kw = dict(batch_duration=4.0, num_workers=2)
    a = list(S.compute_and_store_features_batch(many, ex, tmp_path / "f32", manifest_path=tmp_path / "f32.jsonl.gz", **kw))
    before = S.TEMPLATE_STATS.get("pcm16_batches", 0)
    b = list(S.compute_and_store_features_batch(many, ex, tmp_path / "i16", manifest_path=tmp_path / "i16.jsonl.gz", wav_pcm16=True, **kw))
    assert S.TEMPLATE_STATS.get("pcm16_batches", 0) - before >= 4  # (the batches really came as int16)
    assert [c.id for c in a] == [c.id for c in b] and len(a) == 16
    assert (tmp_path / "i16.hfa").read_bytes() == (tmp_path / "f32.hfa").read_bytes()
    assert [ln.replace(str(tmp_path / "i16"), "@") for ln in _lines(tmp_path / "i16.jsonl.gz")] == [ln.replace(str(tmp_path / "f32"), "@") for ln in _lines(tmp_path / "f32.jsonl.gz")]
