"""GPU: ``FusedMiniBatch.features_of_tracks`` takes a track as a plain tuple of its first 5 to 9 values or as a ``Track``, and gives
the same mini-batch bit for bit either way."""
import numpy as np
import pytest
import torch

import lhotse_amd as LA
from lhotse_amd.input_strategies import FusedMiniBatch, Track

pytestmark = pytest.mark.gpu
SR = 16000


def test_bare_tuples_and_tracks_give_the_same_minibatch_bit_for_bit():
    rng = np.random.default_rng(20241021)
    plain, speech, noise, slow = (rng.standard_normal(n).astype(np.float32) * np.float32(0.1) for n in (2503, 3001, 1777, 2049))
    rir = (rng.standard_normal(301) * np.exp(-np.arange(301) / 40.0) * 0.1).astype(np.float32)
    rir[3] = 1.0
    bare = [[(plain, 1.0, 0, None, True)],  # a plain cut: the shortest legal tuple
            [(speech, 1.0, 0, None, True), (noise, 1.0, 701, 10.0, False), (1000, 1.0, 3001, None, False)],  # a mix, padded to 4001 samples
            [(slow, 1.0, 0, None, True, None, (rir, True), SR // 2)]]  # 8 kHz samples in front of a Resample and a reverb
    wants = [2503, 4001, 2 * 2049]
    typed = [[Track(*tr) for tr in tracks] for tracks in bare]
    assert [[len(tr) for tr in tracks] for tracks in bare] == [[5], [5, 5, 5], [8]] and all(len(tr) == 9 for tracks in typed for tr in tracks)
    assert typed[2][0].reverb[0] is rir and typed[2][0].source_rate == SR // 2 and typed[1][2].samples == 1000 and typed[0][0].levels is None
    fm = FusedMiniBatch(LA.HipFbank(LA.HipFbankConfig(device="cuda:0")), return_audio=True)
    f1, l1, a1 = fm.features_of_tracks(bare, wants, SR)
    f2, l2, a2 = fm.features_of_tracks(typed, wants, SR)
    assert f1.is_cuda and f1.shape[0] == 3 and [len(a) for a in a1] == wants and bool(torch.isfinite(f1[0, : int(l1[0])]).all())
    assert torch.equal(l1, l2) and torch.equal(f1, f2) and all(torch.equal(x, y) for x, y in zip(a1, a2))
