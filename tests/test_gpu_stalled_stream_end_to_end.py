"""GPU: the two on-the-fly input strategies behind a stalled stream: ``FusedMiniBatch.features_of_tracks`` and
``FusedAudioBatch.audio_of_tracks`` over the cuts of tests/golden/reverb.* (helpers: tests/_reverb_golden.py), two mini-batches back to
back on one stalled side stream.

Batch A holds the ``reverb`` group and the ``reverb_cutmix`` group (reverberated tracks behind a pending speed factor, mixed with a
second track), batch B the ``options`` and the ``speed_reverb`` group: mix, reverb and resample launches in one arena in either batch, with
different tables.  The tracks come from files, so there is no device input to poison; the uploads go through the two page-locked
ping-pong buffers of ``extractors._HostStaging``, and batch B packs its tracks into the second one while the copy out of the first is
still pending behind the stall.  The stream must still be stalled when batch B has been enqueued, and both batches then equal, bit for
bit, the same calls made on the default stream with a synchronise behind each (whose features are also held to the goldens with the bars
of tests/test_gpu_reverb.py)."""
import time

import numpy as np
import pytest
import torch

import _reverb_golden as RG
import test_gpu_reverb as TRV
from _golden import err_stats
from _stalled_stream import Stall, side_streams, stall_ms_for

import lhotse_amd as LA
from lhotse_amd.input_strategies import FusedAudioBatch, FusedMiniBatch

pytestmark = pytest.mark.gpu
SR = 16000
BATCHES = (("reverb", "reverb_cutmix"), ("options", "speed_reverb"))
WARM_ROUNDS = 8  # x 2 batches = the 16 slots of the shared arena handles


@pytest.fixture(scope="module")
def batches(tmp_path_factory):
    arrays, meta = RG.load_reverb_goldens()
    paths = RG.corpus_files(tmp_path_factory.mktemp("wav"), meta)
    out = []
    for groups in BATCHES:
        entries = [(g, i, e) for g in groups for i, e in enumerate(meta["groups"][g])]
        out.append(([RG.tracks_of(e, paths, arrays) for _, _, e in entries], [e["want"] for _, _, e in entries],
                    [arrays[f"{g}/{i}/feats"] for g, i, _ in entries]))
    for cuts, _, _ in out:  # every batch has a reverberated track, a pending speed and (batch A) a mixed cut
        assert any(len(t) > 6 for c in cuts for t in c) and any(t[1] != 1.0 for c in cuts for t in c)
    assert any(len(c) > 1 for c in out[0][0])
    return out


def _two_batches_behind_a_stall(name, call, batches):
    """call(cuts, wants) -> a tuple of tensors, on torch's current stream"""
    for _ in range(WARM_ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        alone = [call(cuts, wants) for cuts, wants, _ in batches]
        enqueue_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
    want = [[t.cpu() for t in res] for res in alone]
    torch.cuda.synchronize()
    S = side_streams()[0]
    ms = stall_ms_for(enqueue_ms)
    print(f"{name}: warm-up enqueue {enqueue_ms:.3f} ms, stall {ms:.0f} ms")
    stall = Stall(S, ms)
    with torch.cuda.stream(S):
        got = [call(cuts, wants) for cuts, wants, _ in batches]
    assert stall.still_stalled(), f"{name}: the host did not finish enqueuing both batches while the stream was stalled ({ms:.0f} ms)"
    S.synchronize()
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) and all(torch.equal(a.cpu(), b) for a, b in zip(g, w)), (name, "batch", k)
    return want


def test_features_of_tracks(batches):
    fm = FusedMiniBatch(LA.HipFbank(LA.HipFbankConfig(device="cuda:0")))
    alone = _two_batches_behind_a_stall("features_of_tracks", lambda cuts, wants: fm.features_of_tracks(cuts, wants, SR)[:2], batches)
    for (feats, lens), (_, _, golden) in zip(alone, batches):
        assert lens.tolist() == [len(w) for w in golden]
        for i, w in enumerate(golden):
            s = err_stats(feats[i, : len(w)].numpy(), w)
            assert s["rel_l2"] <= TRV.REL_TOL and s["max_abs"] <= TRV.ABS_TOL, (i, s)
            assert np.all(feats[i, len(w):].numpy() == np.float32(LA.compat.LOG_EPSILON))


def test_audio_of_tracks(batches):
    ab = FusedAudioBatch("cuda:0")
    alone = _two_batches_behind_a_stall("audio_of_tracks", lambda cuts, wants: ab.audio_of_tracks(cuts, wants, SR), batches)
    for (audio, lens), (_, wants, _) in zip(alone, batches):
        assert tuple(audio.shape) == (len(wants), max(wants)) and lens.tolist() == wants and bool(torch.isfinite(audio).all())
