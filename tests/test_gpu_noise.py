"""GPU: the noise kernel (hipfeat_noise_run behind noise_on_device / HipRandomizedSmoothing) against its float64 statement
(tests/_noise_ref.py).  Bar, per case: max|device - f64| <= max(2 * max|ref32 - f64|, FLOOR * max|n|) with ref32 the same formulae in
numpy float32 and the floor four float32 roundings at the largest normal of the case.  cols 1 ... 9 walk the head, one and two whole
16-byte groups and the tail of a float32 row (3 rows of an odd length start at three phases of the 16 bytes); 259 makes more than one
wave of groups.  Keys and seed are beyond 2^32, so all six key and counter words of the generator matter."""
import numpy as np
import pytest
import torch

import _noise_ref as R
import lhotse_amd as LA

pytestmark = pytest.mark.gpu
FLOOR = 4 * 2.0**-24
SEED = (1 << 32) + 12345
KEYS = [7, (1 << 32) + 3, (1 << 62) + 11]
COLS = (1, 3, 4, 5, 8, 9, 259)
EPS = {torch.float32: 2.0**-24, torch.float16: 2.0**-11, torch.bfloat16: 2.0**-8}  # half an ulp, relative


def _bar(truth, cols, rows):
    e32 = np.abs(R.batch(SEED, KEYS[:rows], cols, np.float32) - truth).max()
    return max(2 * e32, FLOOR * np.abs(truth).max())


@pytest.mark.parametrize("rows", (1, 3))
@pytest.mark.parametrize("cols", COLS)
def test_noise_alone_against_the_statement(cols, rows):
    truth = R.batch(SEED, KEYS[:rows], cols)
    z = LA.noise_on_device(torch.zeros(rows, cols, device="cuda"), 1.0, seed=SEED, row_keys=KEYS[:rows], clip=None).cpu().numpy()
    e, bar = np.abs(z - truth).max(), _bar(truth, cols, rows)
    print("max|dev - f64|", e, "bar", bar, "ratio", e / bar)
    assert e <= bar


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16, torch.bfloat16))
@pytest.mark.parametrize("cols", (9, 259))
def test_full_formula_against_the_statement(cols, dtype):
    rows, sigma = 3, [0.25, -0.5, 0.125]
    x = (torch.rand(rows, cols, generator=torch.Generator().manual_seed(cols)) * 2.4 - 1.2).to(dtype)  # some samples beyond the clip
    truth = R.batch(SEED, KEYS, cols)
    want = np.clip(x.double().numpy() + np.array(sigma)[:, None] * truth, -1, 1)
    z = LA.noise_on_device(x.cuda(), sigma, seed=SEED, row_keys=KEYS)
    assert z.dtype == dtype and np.abs(want).max() == 1.0  # the clip acts in every case
    err = np.abs(z.cpu().double().numpy() - want)
    bar = np.abs(sigma)[:, None] * _bar(truth, cols, rows) + EPS[dtype] * np.abs(want)
    print("max err / bar", (err / bar).max())
    assert (err <= bar).all()


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_the_bits_depend_on_seed_key_and_sample_index_alone(dtype):
    rows, cols = 3, 259
    x = (torch.randn(rows, cols, generator=torch.Generator().manual_seed(1)) * 0.4).to(dtype).cuda()
    kw = dict(seed=SEED, row_keys=KEYS)
    z = LA.noise_on_device(x, 0.3, **kw)
    assert torch.equal(z, LA.noise_on_device(x, 0.3, **kw)) and not torch.equal(z, LA.noise_on_device(x, 0.3, seed=SEED + 1, row_keys=KEYS))
    for b in range(rows):  # a row alone, as (1, T) and as (T,), is the row inside the batch
        assert torch.equal(LA.noise_on_device(x[b:b + 1], 0.3, seed=SEED, row_keys=KEYS[b:b + 1]), z[b:b + 1])
        assert torch.equal(LA.noise_on_device(x[b], 0.3, seed=SEED, row_keys=KEYS[b:b + 1]), z[b])
    wide = torch.zeros(rows * (cols + 1) + 1, dtype=dtype, device="cuda")
    shifted = wide[1:].view(rows, cols + 1)[:, :cols]  # storage offset of one element, row stride cols + 1
    shifted.copy_(x)
    out = torch.full_like(wide, 7.0)
    assert torch.equal(LA.noise_on_device(shifted, 0.3, out=out[1:].view(rows, cols + 1)[:, :cols], **kw), z)
    assert torch.equal(out[1:].view(rows, cols + 1)[:, cols], torch.full((rows,), 7.0, dtype=dtype, device="cuda")) and float(out[0]) == 7.0
    assert LA.noise_on_device(shifted, 0.3, out=shifted, **kw) is shifted and torch.equal(shifted, z)  # in place


@pytest.mark.parametrize("cols", (5, 259))
def test_amplitude_zero_is_the_clip_bit_for_bit_and_nan_stays(cols):
    x = torch.randn(4, cols, generator=torch.Generator().manual_seed(2)).cuda()
    x[1, cols // 2] = float("nan")
    x[3, 0] = float("nan")
    lengths = [0, 1, cols, cols]
    z = LA.noise_on_device(x, [1.0, 1.0, 0.0, 1.0], seed=SEED, lengths=lengths)
    clipped = torch.clip(x + 0.0, -1, 1)
    assert torch.equal(z[2], clipped[2]) and torch.equal(z[0], clipped[0])
    assert torch.equal(z[1, 1:].isnan(), clipped[1, 1:].isnan()) and torch.equal(z[1, 1:].nan_to_num(5.0), clipped[1, 1:].nan_to_num(5.0))
    full = LA.noise_on_device(x, 1.0, seed=SEED, lengths=torch.tensor([cols] * 4, device="cuda"))
    assert torch.equal(z[1, :1], full[1, :1]) and bool(z[3, 0].isnan()) and torch.equal(z[3, 1:], full[3, 1:]) and not torch.equal(full[0], clipped[0])
    assert torch.equal(full.nan_to_num(5.0), LA.noise_on_device(x, 1.0, seed=SEED).nan_to_num(5.0))


def test_the_module_follows_the_reference_and_replays_under_a_seed():
    T = 2**16
    audio = (torch.randn(4, T, generator=torch.Generator().manual_seed(3)) * 0.01).cuda()
    assert torch.equal(LA.HipRandomizedSmoothing(p=0.0)(audio * 200), torch.clip(audio * 200, -1, 1))
    scheduled = LA.HipRandomizedSmoothing(sigma=[(0, 0.01), (2, 0.1)], sample_sigma=False, p=1.0, seed=5)
    stds = [float((scheduled(audio) - audio).std()) for _ in range(3)]
    assert scheduled.step == 3 and stds[0] < 0.02 and stds[1] < 0.02 and stds[2] > 0.05
    a, b = LA.HipRandomizedSmoothing(seed=11, p=1.0), LA.HipRandomizedSmoothing(seed=11, p=1.0)
    torch.manual_seed(0)
    first, second = a(audio), a(audio)
    torch.manual_seed(0)
    assert a.step == 0 and torch.equal(b(audio), first) and torch.equal(b(audio), second) and not torch.equal(first, second)
    sigma = 0.1
    z = LA.HipRandomizedSmoothing(sigma=sigma, sample_sigma=False, p=1.0, seed=1)(audio)  # |audio| < 0.06 and 5.8 sigma < 0.6: no clip
    std = (z - audio).double().std(dim=1).cpu().numpy()
    assert (np.abs(std - sigma) <= 6 * sigma / np.sqrt(2 * T)).all(), std
    with pytest.raises(LA._lib.HipFeatError, match="no CPU fallback"):
        LA.noise_on_device(audio.cpu(), 0.1, seed=1)
