"""GPU: ``FusedFeatureBatch`` -- the lhotse-free half of ``HipPrecomputedFeatures`` (stored tracks -> pinned staging -> ONE byte arena -> the
two launches) -- on features this project's own archive writers stored (``hip_archive_f16`` and ``hip_archive``), read back with
``read_raw``.  The batch holds a plain cut, a right-padded cut (copy form), a cut with a noise track at an SNR and an offset, and a cut
padded on both sides (fold form), as ``pending_feature_mix`` tables them for ``CutMix`` / ``.pad``.  ``features_lens`` is int32 and equal
to the cuts' frame counts, copy-form rows are bit-equal to the stored values, fold-form rows are within the bound of
tests/test_gpu_featmix.py of the float64 truth (tests/_featmix_ref.py) over the very bytes that were uploaded.  (The class against the
reference's own ``PrecomputedFeatures`` on the same cuts: tests/test_featmix_reference.py, where lhotse is.)"""
import numpy as np
import pytest
import torch

import _featmix_ref as R

from lhotse_amd import FusedFeatureBatch
from lhotse_amd import input_strategies as IS
from lhotse_amd.augmentation import FEATMIX_COPY as COPY, FEATMIX_FOLD as FOLD
from lhotse_amd.storage import HipArchiveF16Reader, HipArchiveF16Writer, HipArchiveReader, HipArchiveWriter, _parse_key

pytestmark = pytest.mark.gpu
F = 80
FRAMES = [77, 60, 41, 33]


@pytest.mark.parametrize("kind", ["hip_archive_f16", "hip_archive"])
def test_a_batch_from_the_projects_own_archive(kind, tmp_path, monkeypatch):
    rs = np.random.RandomState(4)
    mats = [rs.uniform(-15.0, 5.0, (n, F)).astype(np.float32) for n in FRAMES]
    writer, reader = (HipArchiveF16Writer, HipArchiveF16Reader) if kind == "hip_archive_f16" else (HipArchiveWriter, HipArchiveReader)
    with writer(tmp_path / "feats") as w:
        keys = w.write_packed(np.concatenate(mats), FRAMES)
        path = w.storage_path
    if kind == "hip_archive_f16":
        mats = [m.astype(np.float16).astype(np.float32) for m in mats]
    rd = reader(path)

    def stored(i, lo=0, hi=None, **kw):
        rows = _parse_key(keys[i])[1]
        n = (rows if hi is None else min(rows, hi)) - lo
        return dict(frames=n, rows=n, f16=kind == "hip_archive_f16", read=lambda out: rd.read_raw(keys[i], lo, hi, out=out), **kw)

    pad = lambda n, first=0: dict(frames=n, first=first, value=R.LOG_EPSILON)  # noqa: E731
    cuts = [dict(form=COPY, num_frames=77, ref_track=-1, tracks=[stored(0)]),
            dict(form=COPY, num_frames=77, pad_value=R.LOG_EPSILON, ref_track=-1, tracks=[stored(1)]),
            dict(form=FOLD, num_frames=77, ref_track=0, tracks=[stored(0), stored(2, first=20, snr=12.0), pad(16, 61)]),  # CutMix: noise, then padding
            dict(form=FOLD, num_frames=77, ref_track=1, tracks=[pad(22), stored(3, 3, 33, first=22), pad(25, 52)])]  # a truncated cut, padded on both sides
    seen = []
    real = IS._featmix_in_arena

    def spy(arena, table, nf, rows, layout=None):
        seen.append((arena.cpu().numpy(), table))
        return real(arena, table, nf, rows, layout)

    monkeypatch.setattr(IS, "_featmix_in_arena", spy)
    batch = FusedFeatureBatch("cuda")
    feats, lens = batch.features_of(cuts, F)
    again, _ = batch.features_of(cuts, F)  # (the staging buffer is reused behind the first upload)
    torch.cuda.synchronize()
    assert feats.is_cuda and feats.dtype == torch.float32 and feats.shape == (4, 77, F) and lens.dtype == torch.int32 and lens.tolist() == [77] * 4
    assert torch.equal(feats, again)
    host, table = seen[0]
    item = 2 if kind == "hip_archive_f16" else 4
    assert len(host) == sum(-(-n * F * item // 16) * 16 for n in (77, 60, 77, 41, 30))  # the rows travel as they were stored
    got, truth = feats.cpu().numpy(), R.batch(host, table, F)
    assert np.array_equal(got[0], mats[0]) and np.array_equal(got[1][:60], mats[1]) and (got[1][60:] == np.float32(R.LOG_EPSILON)).all()
    for b in (2, 3):
        err = np.abs(got[b].astype(np.float64) - truth[b])
        bound = R.bar(truth[b]) + R.carried(table[b])[:, None]
        print(f"{kind} cut {b}: max |out - truth| = {err.max():.3e}")
        assert (err <= bound).all(), (kind, b, float((err - bound).max()))
    assert np.allclose(got[3][52:], np.log(2e-10), rtol=0, atol=4e-6)  # the tail two paddings cover
    # the truncated cut's own frames came from rows [3, 33) of its stored matrix
    e = np.exp(mats[3][3:33].astype(np.float64))
    assert np.allclose(got[3][22:52], np.log(np.maximum(1e-10, e + 0.0)), rtol=0, atol=4e-6)


def test_a_table_no_launch_could_serve_is_refused_before_anything_is_read():
    def boom(out):
        raise AssertionError("read before the layout was checked")

    cuts = [dict(form=COPY, num_frames=5, ref_track=-1, tracks=[dict(frames=9, rows=9, f16=False, read=boom)])]
    with pytest.raises(ValueError, match="does not fit"):
        FusedFeatureBatch("cuda").features_of(cuts, F)
    with pytest.raises(ValueError, match="float32 or float16"):
        FusedFeatureBatch("cuda").features_of([dict(form=COPY, num_frames=2, tracks=[dict(frames=2, array=np.zeros((2, F), dtype=np.float64))])], F)
