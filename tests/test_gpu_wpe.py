"""GPU: the fused WPE kernel (hipfeat_wpe_run behind wpe_on_device / HipDereverbWPE) against the float64 statement of the algorithm
(tests/_wpe_ref.py).  Bar, per batch row: E(device) <= max(2 * E(ref32), 4 * 2^-24), E = ||z - truth|| / ||truth||, ref32 = the same
operations in torch complex64 on the CPU; the floor is four float32 roundings of the output.

Frame counts (halo = delay + taps - 1; K = taps * D): R is positive definite only where at least K frames of the statistics have a
non-zero first tap, T - delay of them ("full") or T - halo ("valid").  Below that R is rank deficient and rounding alone decides, in
the truth too, whether a pivot comes out positive -- and with exactly K such frames Yt is square, G fits Y exactly and X = 0: from the second
iteration on the weights are rounding noise.  So "one more than the halo" is taken as the shortest count with twice as many equations
as unknowns, 2 K + delay or 2 K + halo.  At T == halo the last tap's rows of Yt are zero, R has a zero row and column exactly, and every bin returns Y bit for bit.
delay == 0 puts Y itself into Yt: the exact answer is G = [I; 0], X = 0, so every bin must come back either as Y bit for bit (no factor)
or below 1e-3 ||Y|| (the truth is at 1e-13; the bar on a relative error against ~0 would say nothing).
Every case runs both routes of the rank-T update (HIPFEAT_WPE_UPDATE = fma | mfma).
"""
import itertools

import numpy as np
import pytest
import torch

import _wpe_ref as W
import lhotse_amd as LA

pytestmark = pytest.mark.gpu
FLOOR = 4 * 2.0**-24
B, F, TILE = 2, 17, LA.signal_transforms.WPE_TILE_FRAMES  # n_fft = 32


def _tvals(D, taps, delay, mode):
    halo = delay + taps - 1
    return {halo, 2 * taps * D + (halo if mode == "valid" else delay), TILE - 1, TILE, TILE + 1, 2 * TILE + halo} - {0}


CASES = [(D, taps, delay, its, mode, T) for D, taps, delay, its, mode in itertools.product((1, 2, 3), (1, 10), (0, 3), (1, 3), ("full", "valid"))
         for T in sorted(_tvals(D, taps, delay, mode))]
# K = 64; and D = 64: the tile halves to 64 frames and pass 2 has more blocks (392; 26 of 16 x 16) than one round takes
CASES += [(4, 16, 3, 3, "full", 300), (64, 1, 3, 2, "full", 300)]


def _device(Y, **kw):
    return LA.wpe_on_device(torch.from_numpy(Y).cuda(), **kw).cpu()


def _check_bar(z, Y, kw, truth=None):
    want, rule = truth or W.truth(Y, **kw)
    r32 = W.ref32(Y, **kw)
    assert np.isfinite(want).all() and np.isfinite(r32).all() and not rule.any()  # a condition on the inputs: no fallback can meet the bar
    e, e32 = W.row_errors(z, want), W.row_errors(r32, want)
    print("E(device)", e, "E(ref32)", e32, "ratio", e / np.maximum(2 * e32, FLOOR))
    assert (e <= np.maximum(2 * e32, FLOOR)).all(), (e, e32)


@pytest.mark.parametrize("D,taps,delay,its,mode,T", CASES)
def test_core_against_the_truth(D, taps, delay, its, mode, T, monkeypatch):
    kw = dict(taps=taps, delay=delay, iterations=its, statistics_mode=mode)
    Y = W.reverberant(B if D < 64 else 1, D, F, T, seed=T + 7 * D)
    truth, Yt = W.truth(Y, **kw), torch.from_numpy(Y)
    for update in ("fma", "mfma"):
        monkeypatch.setenv("HIPFEAT_WPE_UPDATE", update)
        z = _device(Y, **kw)
        assert z.shape == Y.shape and bool(torch.isfinite(torch.view_as_real(z)).all())
        if T == delay + taps - 1:
            assert truth[1].all() and torch.equal(z, Yt)
        elif delay == 0:
            same = (torch.view_as_real(z) == torch.view_as_real(Yt)).all(-1).all(-1).all(1)  # (B, F)
            small = torch.linalg.vector_norm(z, dim=(1, 3)) <= 1e-3 * torch.linalg.vector_norm(Yt, dim=(1, 3))
            assert bool((same | small).all()) and bool(small.any()), (same, small)
        else:
            _check_bar(z.numpy(), Y, kw, truth)


def test_bins_without_a_factor_come_back_unchanged():
    Y = W.reverberant(3, 2, F, 300, seed=1)
    Y[1] = 0  # a silent row
    Y[:, :, 5] = 0  # a silent bin
    for kw in (dict(), dict(statistics_mode="valid")):
        z = _device(Y, **kw)
        assert bool(torch.isfinite(torch.view_as_real(z)).all())
        assert torch.equal(z[1], torch.from_numpy(Y[1])) and torch.equal(z[:, :, 5], torch.from_numpy(Y[:, :, 5]))
        _check_bar(np.delete(z.numpy()[[0, 2]], 5, axis=2), np.delete(Y[[0, 2]], 5, axis=2), kw)  # and the others are dereverberated
    Y = W.reverberant(B, 2, F, 12, seed=2)
    assert torch.equal(_device(Y, statistics_mode="valid"), torch.from_numpy(Y))  # T = delay + taps - 1: no frame in S


def test_strided_views_batch_composition_and_repeats_give_the_same_bits():
    D, T = 2, TILE + 40
    Y = torch.from_numpy(W.reverberant(3, D, F, T, seed=3)).cuda().reshape(3 * D, F, T)
    z = LA.wpe_on_device(Y, channels=D)
    big = torch.zeros(3 * D, F + 3, 2 * T + 5, dtype=torch.complex64, device="cuda")
    view = big[:, 2 : 2 + F, 1 : 1 + 2 * T : 2]
    view.copy_(Y)
    out = torch.full((T + 1, 3 * D, F), float("nan"), dtype=torch.complex64, device="cuda").permute(1, 2, 0)[:, :, 1:]
    assert not view.is_contiguous() and not out.is_contiguous()
    assert LA.wpe_on_device(view, channels=D, out=out) is not None and torch.equal(out, z)
    assert torch.equal(LA.wpe_on_device(Y, channels=D), z)
    assert torch.equal(LA.wpe_on_device(Y[D : 2 * D], channels=D), z[D : 2 * D])  # a cut alone == the cut in its batch
    assert torch.equal(LA.wpe_on_device(Y.reshape(3, D, F, T)), z.reshape(3, D, F, T))
    with pytest.raises(ValueError, match="overlap"):
        LA.wpe_on_device(view, channels=D, out=big[:, 2 : 2 + F, 2 : 2 + 2 * T : 2])


@pytest.mark.parametrize("shape,taps", [((2, 4000), 10), ((2, 3, 4000), 8), ((2, 3, 6000), 10)])
def test_module_against_stft_truth_istft(shape, taps):
    """4000 samples are 32 frames, 29 of them behind the delay: three channels with the default 10 taps (K = 30) would make R rank
    deficient (see the top of the file), so that case runs with 8 taps, and the default 10 taps on three channels at 6000 samples."""
    rng = np.random.default_rng(11)
    src = rng.standard_normal(shape[:1] + (1, shape[-1] + 600))
    h = rng.standard_normal(shape[:1] + (shape[1] if len(shape) == 3 else 1, 600)) * np.exp(-np.arange(600) / 120.0)
    audio = np.stack([[np.convolve(src[b, 0], hc)[600 : 600 + shape[-1]] for hc in h[b]] for b in range(shape[0])])
    audio = (audio + 0.01 * audio.std() * rng.standard_normal(audio.shape)).astype(np.float32).reshape(shape)
    got = LA.HipDereverbWPE(taps=taps)(torch.from_numpy(audio).cuda()).cpu()
    window = torch.blackman_window(512, dtype=torch.float64)
    a64 = torch.from_numpy(audio).double()
    Y = torch.stft(a64.reshape(-1, shape[-1]), n_fft=512, hop_length=128, return_complex=True, window=window)
    Y4 = Y.reshape(shape[0], -1, *Y.shape[1:]).numpy()
    want, rule = W.truth(Y4, taps=taps)
    r32 = W.ref32(Y4, taps=taps)
    back = lambda Z: torch.istft(torch.from_numpy(np.ascontiguousarray(Z)).reshape(Y.shape), n_fft=512, hop_length=128, window=window)  # noqa: E731
    zw, z32 = back(want).reshape(*shape[:-1], -1), back(r32.astype(np.complex128)).reshape(*shape[:-1], -1)
    assert got.shape == zw.shape and got.dtype == torch.float32 and not rule.any()
    e, e32 = W.row_errors(got.numpy(), zw.numpy()), W.row_errors(z32.numpy(), zw.numpy())
    print("module E(device)", e, "E(ref32)", e32)
    assert (e <= np.maximum(2 * e32, FLOOR)).all(), (e, e32)
    if len(shape) == 2:  # (B, T) rows are (B, 1, T) examples
        assert torch.equal(LA.HipDereverbWPE()(torch.from_numpy(audio).cuda()[:, None]).cpu()[:, 0], got)


def test_limits_raise_the_documented_errors():
    Y = torch.zeros(1, 5, F, 40, dtype=torch.complex64)
    with pytest.raises(NotImplementedError, match="taps \\* channels = 65"):
        LA.wpe_on_device(Y.cuda(), taps=13)
    with pytest.raises(LA._lib.HipFeatError, match="no CPU fallback"):
        LA.wpe_on_device(Y)
    with pytest.raises(LA._lib.HipFeatError, match="no CPU fallback"):
        LA.HipDereverbWPE()(torch.zeros(2, 4000))
