"""GPU: the fused narrowband kernel (hipfeat_narrowband_run behind narrowband_on_device / HipNarrowband) against its float64 statement
(tests/_narrowband_ref.py), row by row of a ragged batch whose lengths put the 8 kHz length L8 at 0, 1, M - 1, M, M + 1 and 2 M + 1 (M: the
tile the library reports), in a tensor whose row stride exceeds its width, NaN behind every length.

Bar: |device - f64| <= 4e-6 * max(1, peak of the row's result).  A float32 chain may land on the neighbouring mu-law code where the code
value u lies within EPS = 1e-3 of an integer: without restore such a sample may instead meet the bar against the decoded neighbour; with
restore an output whose 16-tap window holds such an 8 kHz sample is left out, at most 10 % of a row."""
import functools

import numpy as np
import pytest
import torch

import _narrowband_ref as R
import _sinc_ref as SR
import lhotse_amd as LA

pytestmark = pytest.mark.gpu
EPS, TOL, TAPS = 1e-3, 4e-6, 16
AMPLITUDES = (0.5, 0.05, 0.5, 1.5, 0.0, 0.05)  # 1.5: codes beyond 0 ... 255 and negative u; 0.0: the decoded silence inside, zeros outside


@functools.lru_cache(maxsize=None)
def filters(rate):
    return None if rate == 8000 else (SR.window(rate, 8000), SR.window(8000, rate))


def l8_of(n, rate):
    g = np.gcd(rate, 8000)
    return n if rate == 8000 else SR.resampled_length(n, rate // g, 8000 // g)


def shortest_row(l8, rate):
    n = max(0, (l8 - 1) * rate // 8000 - 2)
    while l8_of(n, rate) < l8:
        n += 1
    return n


@pytest.mark.parametrize("restore", (True, False))
@pytest.mark.parametrize("rate", (8000, 16000, 44100, 11025, 48000))
def test_ragged_batch_against_the_statement(rate, restore):
    M = LA.narrowband_geometry(rate)["tile"]
    l8s = [0, 1, M - 1, M, M + 1, 2 * M + 1]
    lengths = [shortest_row(l8, rate) for l8 in l8s]
    B, T = len(lengths), max(lengths) + 3
    rng = np.random.RandomState(rate)
    x = np.full((B, T + 5), np.nan, dtype=np.float32)
    for b, n in enumerate(lengths):
        x[b, :n] = AMPLITUDES[b] * rng.randn(n)
    dev = torch.from_numpy(x).cuda()[:, :T]  # row stride T + 5
    got = LA.HipNarrowband("mulaw", rate, restore)(dev, rate, lengths=lengths)
    if not restore and rate != 8000:
        got, out_lengths = got
        assert isinstance(out_lengths, torch.Tensor) and out_lengths.device.type == "cpu" and out_lengths.tolist() == l8s
    elif not restore:
        got, out_lengths = got
        assert out_lengths.tolist() == lengths
    up = restore and rate != 8000
    assert got.shape == (B, T if up or rate == 8000 else l8_of(T, rate))
    # purity: lengths on the device give the same bits; a row alone gives the bits it has inside the batch
    again = LA.narrowband_on_device(dev, rate, restore_orig_sr=restore, lengths=torch.tensor(lengths, device="cuda"))
    assert torch.equal(got, again[0] if isinstance(again, tuple) else again)
    alone = LA.narrowband_on_device(dev[3, : lengths[3]], rate, restore_orig_sr=restore)
    assert torch.equal(alone, got[3, : alone.shape[0]])
    got = got.cpu().numpy()
    first, _, width, orig, new = filters(rate)[1] if up else (None, None, 0, 1, 1)
    worst = 0.0
    for b, n in enumerate(lengths):
        want, u = R.narrowband(x[b, :n], rate, restore, filters(rate))
        m = len(want)
        assert m == (n if up else l8s[b]) and not got[b, m:].view(np.uint32).any()  # +0.0 behind the row, bit for bit
        if m == 0:
            continue
        bar = TOL * max(1.0, np.abs(want).max())
        err = np.abs(got[b, :m] - want)
        near = (np.abs(u - np.round(u)) < EPS) & (u != 128.0)  # (u == 128 exactly is d == 0: code 128 in any arithmetic, nothing is rounded)
        if up:
            o = np.arange(m)
            s0 = (o // new) * orig + first[o % new] - width
            hits = np.concatenate([[0], np.cumsum(near)])  # near-integer codes in front of each 8 kHz position
            lo, hi = np.clip(s0, 0, len(u)), np.clip(s0 + TAPS, 0, len(u))
            keep = hits[hi] == hits[lo]
            assert (~keep).mean() <= 0.10, f"row {b}: {(~keep).mean():.3f} of the samples left out"
            err = err[keep]
        else:
            for side in (-EPS, EPS):
                err = np.where(near, np.minimum(err, np.abs(got[b, :m] - R.decode(np.trunc(u + side)))), err)
        worst = max(worst, float(err.max() / bar) if err.size else 0.0)
        print(f"rate {rate} restore {restore} row {b} (n {n}, L8 {l8s[b]}, amplitude {AMPLITUDES[b]}): max err {err.max() if err.size else 0:.3e}, bar {bar:.3e}")
        assert (err <= bar).all(), f"row {b}: {err.max()} > {bar}"
    print(f"rate {rate} restore {restore}: worst err / bar {worst:.3f}")

