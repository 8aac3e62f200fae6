"""CPU: the numpy statement of the mono downmix (tests/_multichannel_ref.py) against the truth and against torch.

* PCM-derived inputs (int16 / 32768: multiples of 2^-15, whose float64 sums are exact): with ``t = math.fsum(x_c) / C`` in float64,
  ``|y - t| <= 0.5 ulp32(t) (1 + 2^-20)`` -- the statement is the correctly rounded mean (the 2^-20 covers the one float64 rounding of
  ``t`` itself, 2^-29 ulp32, with room).
* C = 2: ``array_equal`` to ``torch.mean(dim=0)`` -- float32 ``(a + b) / 2`` rounds once, in the sum, and the halving is exact.
* ``collate_sources_ref`` places rows as ``collate_ref`` does; a row of one source is ``collate_ref``'s row bit for bit."""
import math

import numpy as np
import pytest
import torch

from _collate_ref import bits_of, collate_ref
from _multichannel_ref import collate_sources_ref, downmix_ref, ulp32


def _pcm(C, T, seed):
    return (np.random.RandomState(seed).randint(-32768, 32768, size=(C, T)).astype(np.float32) / np.float32(32768.0)).astype(np.float32)


@pytest.mark.parametrize("C", [2, 3, 5, 6, 7, 8, 16, 32])
@pytest.mark.parametrize("T", [5, 16, 1003])
def test_the_statement_is_the_correctly_rounded_mean_of_pcm_samples(C, T):
    x = _pcm(C, T, 100 * C + T)
    y = downmix_ref(x)
    assert y.dtype == np.float32 and y.shape == (T,)
    t = np.array([math.fsum(float(v) for v in x[:, i]) / C for i in range(T)], dtype=np.float64)
    err = np.abs(y.astype(np.float64) - t)
    bound = 0.5 * ulp32(t) * (1.0 + 2.0 ** -20)
    print(f"C={C} T={T}: max |y - t| / ulp32 = {float((err / ulp32(t)).max()):.6f}")
    assert (err <= bound).all(), float((err / ulp32(t)).max())


@pytest.mark.parametrize("T", [5, 16, 100003])
def test_two_channels_equal_torch_mean(T):
    for x in (_pcm(2, T, T), np.random.RandomState(T).randn(2, T).astype(np.float32) * np.float32(3.0)):
        assert np.array_equal(downmix_ref(x), torch.from_numpy(x).mean(dim=0).numpy())


def test_nan_inf_and_signed_zero_follow_ieee():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    x = np.array([[1.0, inf, inf, nan, -0.0, -0.0, 1.0], [2.0, 1.0, -inf, 1.0, -0.0, 0.0, -1.0]], dtype=np.float32)
    y = downmix_ref(x)
    assert y[0] == 1.5 and y[1] == inf and np.isnan(y[2]) and np.isnan(y[3]) and y[6] == 0.0
    assert bits_of(torch.from_numpy(y[4:7].copy())).tolist() == [0, 0, 0]  # the sum starts from +0.0: a zero mean is +0
    one = np.array([[-0.0, nan, 3.0]], dtype=np.float32)
    assert np.array_equal(downmix_ref(one).view(np.uint32), one[0].view(np.uint32))  # one channel: the bits


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_rows_are_placed_as_collate_ref_places_them(dtype):
    rs = np.random.RandomState(3)
    arena = rs.randn(400).astype(np.float32)
    first, src, lens, dst = [0, 1, 1, 3, 4], [7, 100, 201, 300], [50, 9, 60, 0], [0, 3, 10, 70]
    got = collate_sources_ref(arena, first, src, lens, 70, dst, dtype)
    assert got.shape == (4, 70) and got.dtype == dtype
    # k = 1 rows are collate_ref's rows; the k = 0 row and the row of no samples are zeros
    want = collate_ref(arena, [7, 0, 0, 300], [50, 0, 0, 0], 70, dst, dtype)
    assert np.array_equal(bits_of(got[[0, 1, 3]]), bits_of(want[[0, 1, 3]]))
    mean = torch.from_numpy(downmix_ref([arena[100:160], arena[201:261]])).to(dtype)
    assert np.array_equal(bits_of(got[2, 10:70]), bits_of(mean)) and not bits_of(got[2, :10]).any()
    assert collate_sources_ref(arena, [0], [], [], None, None, dtype).shape == (0, 0)
