"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The banded float64 truth of the sinc resampler (``ResampleTensor``, lhotse/augmentation/resample.py:184-315) for ANY rate pair: the
reference's weight formula (:239-281) evaluated with numpy on the window of taps per phase that can carry weight, nothing else -- 8000:4673
costs kilobytes where the reference's dense bank takes 300 MB.  The weights are cast to float32 and back, as the reference caches them
(:280-281); the sums are float64.  ``test_sinc_tables.py`` pins it against ``oracle.resample_ref`` where the dense bank is small.

Nothing here shares code with lhotse_amd/csrc/sinc_tables.hpp: the window is found from the rates in numpy's own arithmetic.
"""
import math

import numpy as np


def geometry(source_rate: int, target_rate: int):
    """-> (orig, new, width): resample.py:219-222, :239"""
    g = math.gcd(int(source_rate), int(target_rate))
    orig, new = int(source_rate) // g, int(target_rate) // g
    return orig, new, math.ceil(6 * orig / (min(orig, new) * 0.99))


def _t(phase, taps, orig, width, base):
    return (phase + (taps - width).astype(np.float64) / orig) * base  # resample.py:246-258


def window(source_rate: int, target_rate: int):
    """-> (first[new] int64, weights[new][W] float64 with float32 values, width, orig, new), W = 2 width + 2: tap d of phase ph is the
    reference's kernel[ph][first[ph] + d]; first[ph] = one tap below the first tap with unclamped |t| < 6."""
    orig, new, width = geometry(source_rate, target_rate)
    base = min(orig, new) * 0.99
    W = 2 * width + 2
    # the phase term is float32 in the reference (torch.arange(0, -new, -1) / new: int64 / int -> float32), promoted by the sum
    phase = (np.arange(0, -new, -1, dtype=np.float32) / np.float32(new)).astype(np.float64)
    live = np.floor(orig * (np.arange(new) / new - 6 / base)).astype(np.int64) + width + 1  # an estimate of the first live tap, then exact:
    for _ in range(8):
        live = np.where(_t(phase, live - 1, orig, width, base) > -6, live - 1, live)
    for _ in range(8):
        live = np.where(_t(phase, live, orig, width, base) <= -6, live + 1, live)
    assert np.all(_t(phase, live, orig, width, base) > -6) and np.all(_t(phase, live - 1, orig, width, base) <= -6)
    first = live - 1
    t = _t(phase[:, None], first[:, None] + np.arange(W)[None, :], orig, width, base)
    t = np.clip(t, -6, 6)
    win = np.cos(t * math.pi / 6 / 2) ** 2
    t = t * math.pi
    scale = base / orig
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(t == 0, 1.0, np.sin(t) / t)
    k = k * (win * scale)  # resample.py:277-278
    return first, k.astype(np.float32).astype(np.float64), width, orig, new


def resampled_length(num_samples: int, orig: int, new: int) -> int:
    return int(np.ceil(np.float32(new * num_samples / orig)))  # resample.py:309


def resample(x, source_rate: int, target_rate: int, filt=None) -> np.ndarray:
    """resample.py:284-315 for one waveform (T,), float64 sums over the window.  ``filt``: a ``window(...)`` computed before."""
    first, w, width, orig, new = window(source_rate, target_rate) if filt is None else filt
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = len(x)
    out_len = resampled_length(n, orig, new)
    W = w.shape[1]
    xp = np.concatenate([x, np.zeros(1)])  # index n = "outside"
    y = np.zeros(out_len, dtype=np.float64)
    for a in range(0, out_len, 1 << 16):
        o = np.arange(a, min(a + (1 << 16), out_len))
        j, ph = o // new, o % new
        s = (j * orig + first[ph] - width)[:, None] + np.arange(W)[None, :]
        s = np.where((s >= 0) & (s < n), s, n)
        y[o] = (xp[s] * w[ph]).sum(axis=1)
    return y
