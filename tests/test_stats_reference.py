"""CPU, under the real lhotse (authoring container only): ``lhotse_amd.compute_global_feature_stats`` and
``HipGlobalMVN.from_cuts(device_stats=True)`` against ``CutSet.compute_global_feature_stats`` on a small CutSet on disk, with the
oracle-backed stand-in for the device plan and the numpy statement of the device's blocked order (tests/_stats_ref.py::DeviceStatement)
standing in for the handle.  The bar is the one of tests/test_gpu_stats.py: per statistic, the error against the longdouble truth stays
within max(2 x the reference's own, 1e-13)."""
import pickle

import numpy as np
import pytest
import torch

import _stats_ref as S

pytestmark = pytest.mark.reference
LENGTHS = [6000, 4800, 7200, 5000, 8000, 3000, 16000]


class CpuAccumulator(S.DeviceStatement):
    """The surface of HipStatsAccumulator over host tensors."""

    def __init__(self, feature_dim, device=None):
        super().__init__(feature_dim)
        self.feature_dim = feature_dim

    def update(self, features, num_frames=None, first_row=None):
        x = features.numpy()
        assert x.ndim == 2 and first_row is None and x.dtype in (np.float32, np.float16)
        bounds = np.concatenate([[0], np.cumsum([len(x)] if num_frames is None else num_frames)]).astype(int)
        for a, b in zip(bounds[:-1], bounds[1:]):
            super().update(x[a:b])


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from _dropin_support import import_lhotse, install_wave_backend, make_cpu_plan, write_cutset

    import_lhotse()
    from lhotse.audio.backend import set_current_audio_backend
    from lhotse.features.io import NumpyFilesWriter

    import lhotse_amd as LA
    import lhotse_amd.extractors as E
    import lhotse_amd.stats as ST

    prev = install_wave_backend()
    saved = (E._Plan, ST.HipStatsAccumulator, ST._DEFAULT_DEVICE)
    E._Plan, ST.HipStatsAccumulator, ST._DEFAULT_DEVICE = make_cpu_plan(), CpuAccumulator, "cpu"
    d = tmp_path_factory.mktemp("statswav")
    cuts = write_cutset(d, LENGTHS, seed=9)
    ex = LA.HipFbank(LA.HipFbankConfig(device="cpu"))
    stored = cuts.compute_and_store_features(extractor=ex, storage_path=str(d / "feats"), storage_type=NumpyFilesWriter)
    yield LA, ST, cuts, stored, ex, d, saved[1]
    E._Plan, ST.HipStatsAccumulator, ST._DEFAULT_DEVICE = saved
    set_current_audio_backend(prev)


def hold(got, want, mats):
    (dm, ds), (rm, rs) = S.errors(got["norm_means"], got["norm_stds"], mats), S.errors(want["norm_means"], want["norm_stds"], mats)
    print(f"[stats] device route {dm:.3g} / {ds:.3g}  (reference {rm:.3g} / {rs:.3g})")
    assert got["norm_means"].dtype == np.float64 and got["norm_means"].shape == want["norm_means"].shape
    assert dm <= max(2.0 * rm, 1e-13) and ds <= max(2.0 * rs, 1e-13), (dm, ds, rm, rs)


def test_with_an_extractor_the_batched_pass_agrees_with_the_reference(env, tmp_path):
    LA, ST, cuts, stored, ex, d, _ = env
    mats = [cut.compute_features(ex) for cut in cuts]
    want = cuts.compute_global_feature_stats(extractor=ex)
    for batch_duration in (600.0, 0.5):  # one batch; several batches in cut order
        hold(LA.compute_global_feature_stats(cuts, extractor=ex, batch_duration=batch_duration), want, mats)
    # max_cuts selects the same cuts, storage_path unpickles to the same dict
    want3 = cuts.compute_global_feature_stats(extractor=ex, max_cuts=3)
    got3 = LA.compute_global_feature_stats(cuts, extractor=ex, max_cuts=3, storage_path=tmp_path / "s.pkl")
    hold(got3, want3, mats[:3])
    assert not np.array_equal(want3["norm_means"], want["norm_means"])
    with open(tmp_path / "s.pkl", "rb") as f:
        back = pickle.load(f)
    assert sorted(back) == ["norm_means", "norm_stds"] and all(np.array_equal(back[k], got3[k]) for k in back)
    mvn = LA.HipGlobalMVN.from_cuts(cuts, extractor=ex, device_stats=True)
    ref = LA.HipGlobalMVN.from_cuts(cuts, extractor=ex)
    for k in ("norm_means", "norm_stds"):  # the float32 casts: at most 1 ulp apart
        a, b = getattr(mvn, k).numpy(), getattr(ref, k).numpy()
        assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b.astype(np.float32))).astype(np.float64)).all(), k


def test_on_stored_features_the_pass_agrees_with_the_reference(env, caplog):
    LA, ST, cuts, stored, ex, d, _ = env
    mats = [cut.load_features() for cut in stored]
    want = stored.compute_global_feature_stats()
    hold(LA.compute_global_feature_stats(stored), want, mats)
    hold(LA.compute_global_feature_stats(stored, batch_duration=0.5), want, mats)
    hold(LA.compute_global_feature_stats(stored, max_cuts=4), stored.compute_global_feature_stats(max_cuts=4), mats[:4])
    # a CutSet in which only some cuts have features: the reference's warning, and the same cuts
    from lhotse import CutSet

    some = CutSet.from_cuts(list(stored)[:2] + list(cuts)[2:4] + list(stored)[4:])
    with caplog.at_level("WARNING"):
        got = LA.compute_global_feature_stats(some)
    assert "only 5/7 cuts have features" in caplog.text
    hold(got, some.compute_global_feature_stats(), mats[:2] + mats[4:])
    with pytest.raises(ValueError, match="Could not find any features in this CutSet; did you forget to extract them"):
        LA.compute_global_feature_stats(cuts)


def test_a_foreign_extractor_and_the_default_keep_the_reference_path(env, monkeypatch):
    LA, ST, cuts, stored, ex, d, _ = env
    from lhotse import CutSet, Fbank

    calls = []
    real = CutSet.compute_global_feature_stats

    def spy(self, *args, **kwargs):
        calls.append(kwargs)
        return real(self, *args, **kwargs)

    monkeypatch.setattr(CutSet, "compute_global_feature_stats", spy)
    foreign = Fbank()
    got = LA.compute_global_feature_stats(cuts, extractor=foreign, max_cuts=2)
    assert len(calls) == 1 and calls[0]["extractor"] is foreign and calls[0]["max_cuts"] == 2
    assert got["norm_means"].shape == (80,)
    LA.HipGlobalMVN.from_cuts(cuts, max_cuts=2, extractor=ex)  # without the flag: the parent's method, as before
    assert len(calls) == 2 and calls[1] == {"max_cuts": 2, "extractor": ex}
    LA.HipGlobalMVN.from_cuts(cuts, max_cuts=2, extractor=ex, device_stats=True)  # with it: not
    assert len(calls) == 2
    # a CPU tensor is refused by the real accumulator's update before any device is touched
    real_cls = env[6]
    acc = object.__new__(real_cls)
    acc.feature_dim, acc.handle = 80, 0
    with pytest.raises(LA._lib.HipFeatError, match="there is no CPU fallback"):
        real_cls.update(acc, torch.zeros(3, 80))
