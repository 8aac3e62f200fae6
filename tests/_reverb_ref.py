"""
numpy statement of the reverberation rule of ABI v7 (include/hipfeat.h, lhotse_amd/csrc/kernel_reverb.hpp), written from the rule:

    hs = rir * 2^-15;  shift = first index of max(hs)
    y[n] = sum_k hs[k] * x[n + shift - k],  0 <= n < N, over the k with 0 <= n + shift - k < N
    normalise:  if sum(y^2) > 0:  y *= (float32) sqrt((sum(x^2) / N) / (sum(y^2) / N))

three ways: ``exact`` (float64 throughout: the truth both implementations are judged against), ``chunked32`` (the device's order: float32
partial sums of 256 consecutive taps -- each the ascending sum of its runs of 16 taps --, added in ascending order; ``chunk=None`` = one serial chain over all taps, the
form the accuracy bar rejects) and ``fft32`` (float32 FFTs of a 2-3-5-smooth size >= N + L - 1: the arithmetic of the CPU path, in the role
of the reference).  ``bars`` are the two audio bars of the suite.  ``integer_item`` / ``integer_expected``: items whose output under the rule
is the same float32 array in every summation order -- the yardstick of the batches that are too large for ``chunked32``.
"""
from __future__ import annotations

import numpy as np

SCALE = np.float32(0.5 ** 15)
EPS24 = 2.0 ** -24


def scale_and_shift(rir):
    hs = np.asarray(rir, dtype=np.float32).reshape(-1) * SCALE
    return hs, int(np.argmax(hs))


def _gain64(x, y):
    n = len(x)
    p_in, p_out = float(np.sum(np.asarray(x, np.float64) ** 2)) / n, float(np.sum(np.asarray(y, np.float64) ** 2)) / n
    return np.sqrt(p_in / p_out) if p_out > 0 else None


def exact(x, hs, shift, normalize=False):
    """float64 convolution of the float32 inputs, shifted; with ``normalize`` scaled by the float64 gain.  -> float64 (N,)"""
    x64, h64 = np.asarray(x, np.float64).reshape(-1), np.asarray(hs, np.float64).reshape(-1)
    y = np.convolve(x64, h64)[shift : shift + len(x64)]
    if normalize:
        g = _gain64(x64, y)
        if g is not None:
            y = y * g
    return y


def chunked32(x, hs, shift, normalize=False, chunk=256, run=16):
    """The device's summation order in float32: runs of ``run`` taps accumulated with a fused multiply-add in ascending order (the exact
    product plus the sum so far, rounded once -- formed here in float64, where the product of two float32 is exact), the runs of a chunk
    of ``chunk`` taps added in ascending order, the chunks added in ascending order.  ``chunk=None``: one serial chain over all taps."""
    x, hs = np.asarray(x, np.float32).reshape(-1), np.asarray(hs, np.float32).reshape(-1)
    n, taps = len(x), len(hs)
    if chunk is None:
        chunk = run = taps
    xp = np.concatenate([np.zeros(taps), x.astype(np.float64), np.zeros(taps)])  # xp[taps + i] = x[i]
    y = np.zeros(n, np.float32)
    idx = np.arange(n) + shift + taps
    for k0 in range(0, taps, chunk):
        p = np.zeros(n, np.float32)
        for k1 in range(k0, min(k0 + chunk, taps), run):
            q = np.zeros(n, np.float32)
            for k in range(k1, min(k1 + run, k0 + chunk, taps)):
                q = (float(hs[k]) * xp[idx - k] + q.astype(np.float64)).astype(np.float32)
            p = p + q
        y = y + p
    if normalize:
        g = _gain64(x, y)
        if g is not None:
            y = y * np.float32(g)
    return y


# ---- integer-valued items: a yardstick without a tolerance for batches too large to model tap by tap -----------------------------------
# x in {-15 ... 15}, rir in {-15 ... 15} with ONE tap of 16 (the unique maximum, so shift = its index): hs = rir * 2^-15, every product and
# every partial sum of them is a multiple of 2^-15 below 15 * 16 * L * 2^-15 -- exact in float32 while 15 * 16 * L < 2^24, in ANY summation
# order, fused or not.  Sx and Sy are sums of multiples of 2^-30 that stay below 2^53 such units: exact in float64 in any order.  What remains of
# the rule is the gain, (float32) sqrt((Sx / N) / (Sy / N)) in correctly rounded float64 operations, and one rounded float32 multiply.
INT_AMPLITUDE, INT_PEAK = 15, 16


def assert_integer_exact(n, taps):
    """The bounds the exactness argument rests on."""
    bound = INT_AMPLITUDE * INT_PEAK * int(taps)  # >= |y| in units of 2^-15
    assert bound < 2 ** 24, f"{taps} taps: partial sums of integer items would leave float32's exact range"
    assert int(n) * bound * bound < 2 ** 53, f"{n} samples x {taps} taps: sum(y^2) would leave float64's exact range"


def integer_item(rng, n, taps, shift, normalize):
    """-> (x, hs, shift, normalize) as the GPU tests' ``_run`` takes items; ``rng``: a numpy Generator."""
    assert_integer_exact(n, taps)
    assert 0 <= shift < taps
    x = rng.integers(-INT_AMPLITUDE, INT_AMPLITUDE + 1, size=n).astype(np.float32)
    rir = rng.integers(-INT_AMPLITUDE, INT_AMPLITUDE + 1, size=taps).astype(np.float32)
    rir[shift] = INT_PEAK
    hs, found = scale_and_shift(rir)
    assert found == shift
    return x, hs, int(shift), bool(normalize)


def integer_expected(x, hs, shift, normalize=False):
    """The float32 output of an integer-valued item under the rule, bit for bit, whatever the summation order -> float32 (N,)"""
    x, hs = np.asarray(x, np.float32).reshape(-1), np.asarray(hs, np.float32).reshape(-1)
    assert_integer_exact(len(x), len(hs))
    assert np.array_equal(x, np.rint(x)) and np.abs(x).max(initial=0) <= INT_AMPLITUDE
    units = hs.astype(np.float64) * 2.0 ** 15
    assert np.array_equal(units, np.rint(units)) and np.abs(units).max(initial=0) <= INT_PEAK
    y64 = exact(x, hs, shift)  # sums of integers x 2^-15 below 2^53: exact
    y = y64.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), y64)
    if normalize:
        g = _gain64(x, y64)  # Sx, Sy exact; /, /, /, sqrt correctly rounded, as on the device
        if g is not None:
            y = y * np.float32(g)  # one rounded float32 multiply
    return y


def _next_fast_len(n):
    while True:
        r = n
        for f in (2, 3, 5):
            while r % f == 0:
                r //= f
        if r == 1:
            return n
        n += 1


def fft32(x, hs, shift, normalize=False):
    """The CPU path's arithmetic: float32 rfft of both, product, irfft, shifted; float32 powers and gain."""
    import torch

    x, hs = np.asarray(x, np.float32).reshape(-1), np.asarray(hs, np.float32).reshape(-1)
    size = _next_fast_len(len(x) + len(hs) - 1)
    f = torch.fft.rfft(torch.from_numpy(x), n=size) * torch.fft.rfft(torch.from_numpy(hs), n=size)
    y = torch.fft.irfft(f, n=size).numpy()[shift : shift + len(x)].astype(np.float32)
    if normalize:
        p_in, p_out = np.sum(np.abs(x) ** 2) / len(x), np.sum(np.abs(y) ** 2) / len(x)
        if p_out > 0:
            y = y * np.sqrt(p_in / p_out)
    return y.astype(np.float32)


def distances(y, truth):
    """(rel-L2, max abs error) of y from the float64 truth."""
    d = np.asarray(y, np.float64) - truth
    den = float(np.sqrt(np.sum(truth ** 2)))
    return (float(np.sqrt(np.sum(d ** 2))) / den if den > 0 else float(np.sqrt(np.sum(d ** 2)))), float(np.max(np.abs(d), initial=0.0))


def bars(ref_rel, ref_max, truth):
    """The audio bars: rel-L2 <= 2 x the reference's own + 2^-24, max abs <= 2 x the reference's own + 2^-24 x peak."""
    return 2.0 * ref_rel + EPS24, 2.0 * ref_max + EPS24 * float(np.max(np.abs(truth), initial=0.0))
