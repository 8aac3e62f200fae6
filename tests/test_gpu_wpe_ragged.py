"""GPU: ragged WPE -- the centred STFT, the WPE kernel with a frame count per example and the inverse STFT with overlap-add
(csrc/kernel_wpe_stft.hpp, kernel_wpe.hpp) behind wpe_stft_on_device / wpe_on_device(frames=) / wpe_istft_on_device / HipDereverbWPE(lengths=).
Bar, per row, as in test_gpu_wpe.py: E(device) <= max(2 * E(ref32), 4 * 2^-24), E = ||x - truth|| / ||truth||; truth = float64 torch on
the CPU on the row ALONE, ref32 = the same operations in float32 / complex64.  Every case prints E(device) / E(ref32).  A row must also
come out bit for bit as it does alone, with exact zeros behind its end, and nothing behind a length is read (NaN lies there)."""
import numpy as np
import pytest
import torch

import _wpe_ref as W
import lhotse_amd as LA

pytestmark = pytest.mark.gpu
FLOOR = 4 * 2.0**-24
TILE, R = LA.signal_transforms.WPE_TILE_FRAMES, LA.signal_transforms.WPE_ISTFT_TILE_HOPS
GRID = [(512, 128), (256, 64), (512, 256), (2048, 512)]
NAN = float("nan")


def _bar(what, got, want, r32):
    want = np.asarray(want)[None]
    e, e32 = W.row_errors(np.asarray(got)[None], want)[0], W.row_errors(np.asarray(r32)[None], want)[0]
    print(what, "E(device)", e, "E(ref32)", e32, "ratio", e / e32)
    assert e <= max(2 * e32, FLOOR), (what, e, e32)


def _zero_bits(t):
    return not bool(t.contiguous().view(torch.int32).any())  # +0.0 alone


@pytest.mark.parametrize("n_fft,hop", GRID)
def test_stft_reflects_at_each_rows_own_ends(n_fft, hop):
    lens = [n_fft // 2 + 1, 7 * hop - 1, 7 * hop, 7 * hop + 1]  # the shortest legal row: every frame reflects at both ends
    T = lens[-1]
    rows = [torch.randn(n, generator=torch.Generator().manual_seed(n)) for n in lens]
    big = torch.full((4, T + 4), NAN)  # odd row stride behind a 4-byte offset: rows alternate between the 8-byte and the 4-byte loads
    audio = big[:, 1 : 1 + T]
    for b, x in enumerate(rows):
        audio[b, : lens[b]] = x
    audio = big.cuda()[:, 1 : 1 + T]
    Y, fr = LA.wpe_stft_on_device(audio, torch.tensor(lens), n_fft, hop)
    assert fr.tolist() == [1 + n // hop for n in lens] and Y.shape == (4, n_fft // 2 + 1, max(fr.tolist())) and Y.dtype == torch.complex64
    for b, (n, x) in enumerate(zip(lens, rows)):
        want, r32 = (torch.stft(x.to(dt), n_fft, hop, window=torch.blackman_window(n_fft, dtype=dt), return_complex=True) for dt in (torch.float64, torch.float32))
        _bar(f"stft {n_fft}/{hop} row {b}", Y[b, :, : fr[b]].cpu(), want, r32)
        assert _zero_bits(torch.view_as_real(Y[b, :, fr[b] :]))
        alone = LA.wpe_stft_on_device(x.cuda()[None], torch.tensor([n]), n_fft, hop)[0]
        assert torch.equal(alone[0], Y[b, :, : fr[b]])


@pytest.mark.parametrize("n_fft,hop,D", [(n, h, 1) for n, h in GRID] + [(512, 128, 2)])
def test_istft_overlap_add_at_the_tile_edges(n_fft, hop, D):
    ov = n_fft // hop
    counts = [ov, ov + 1, R - 1, R, R + 1, 2 * R + 1]
    g = torch.Generator().manual_seed(n_fft + hop + D)
    Z = torch.complex(torch.randn(6, D, n_fft // 2 + 1, 2 * R + 1, generator=g), torch.randn(6, D, n_fft // 2 + 1, 2 * R + 1, generator=g))  # bins 0 and N / 2 too
    dev = Z.cuda()
    for b, c in enumerate(counts):
        dev[b, ..., c:] = NAN
    out = torch.full((6, D, hop * 2 * R), NAN, device="cuda")
    z, zl = LA.wpe_istft_on_device(dev, torch.tensor(counts), n_fft, hop, out=out)
    assert z is out and zl.tolist() == [hop * (c - 1) for c in counts]
    for b, c in enumerate(counts):
        want, r32 = (torch.istft(Z[b, ..., :c].to(cdt), n_fft, hop, window=torch.blackman_window(n_fft, dtype=dt))
                     for cdt, dt in ((torch.complex128, torch.float64), (torch.complex64, torch.float32)))
        _bar(f"istft {n_fft}/{hop} D={D} frames={c}", z[b, :, : zl[b]].cpu(), want, r32)
        assert _zero_bits(z[b, :, zl[b] :])
        alone = LA.wpe_istft_on_device(Z[b : b + 1, ..., :c].cuda(), torch.tensor([c]), n_fft, hop)[0]
        assert torch.equal(alone[0], z[b, :, : zl[b]])


@pytest.mark.parametrize("D,taps", [(1, 10), (3, 8)])
def test_ragged_core_gives_each_row_the_bits_it_has_alone(D, taps, monkeypatch):
    fr = [TILE - 1, TILE, TILE + 1, 2 * taps * D + 3]
    Y = torch.from_numpy(W.reverberant(4, D, 17, TILE + 1, seed=5 + D)).cuda()
    for b, n in enumerate(fr):
        Y[b, ..., n:] = NAN
    for update in ("fma", "mfma"):
        monkeypatch.setenv("HIPFEAT_WPE_UPDATE", update)
        z = LA.wpe_on_device(Y, taps=taps, frames=torch.tensor(fr))
        for b, n in enumerate(fr):
            alone = LA.wpe_on_device(Y[b : b + 1, ..., :n], taps=taps)
            assert bool(torch.isfinite(torch.view_as_real(alone)).all()) and not torch.equal(alone[0], Y[b, ..., :n])
            assert torch.equal(z[b, ..., :n], alone[0]) and _zero_bits(torch.view_as_real(z[b, ..., n:]))


def _module_truth(a, taps):
    """stft -> W.truth / W.ref32 -> istft in float64 for one cut alone, a: (D, n) float32."""
    w = torch.blackman_window(512, dtype=torch.float64)
    Y = torch.stft(torch.from_numpy(a).double(), n_fft=512, hop_length=128, return_complex=True, window=w).numpy()[None]
    (want, rule), r32 = W.truth(Y, taps=taps), W.ref32(Y, taps=taps)
    assert not rule.any() and np.isfinite(r32).all()  # conditions on the inputs
    return [torch.istft(torch.from_numpy(np.ascontiguousarray(Z[0], dtype=np.complex128)), n_fft=512, hop_length=128, window=w).numpy() for Z in (want, r32)]


@pytest.mark.parametrize("shape,taps,lens", [((3, 4000), 10, [4000, 3500, 3001]), ((2, 3, 7000), 8, [7000, 6500])])
def test_module_with_lengths_against_stft_truth_istft_per_row(shape, taps, lens):
    """The shortest rows have 24 frames (K = 10) and 51 frames (K = 24): at least 2 K + delay, so every system is well posed."""
    rng = np.random.default_rng(11)  # the audio of test_module_against_stft_truth_istft
    B, T, D = shape[0], shape[-1], shape[1] if len(shape) == 3 else 1
    src = rng.standard_normal((B, 1, T + 600))
    h = rng.standard_normal((B, D, 600)) * np.exp(-np.arange(600) / 120.0)
    audio = np.stack([[np.convolve(src[b, 0], hc)[600 : 600 + T] for hc in h[b]] for b in range(B)])
    audio = (audio + 0.01 * audio.std() * rng.standard_normal(audio.shape)).astype(np.float32)
    clean, mod = torch.from_numpy(audio.reshape(shape)).cuda(), LA.HipDereverbWPE(taps=taps)
    dev = clean.clone()
    for b, n in enumerate(lens):
        dev[b, ..., n:] = NAN
    z, zl = mod(dev, lengths=torch.tensor(lens))
    assert zl.tolist() == [128 * (n // 128) for n in lens] and z.shape == shape[:-1] + (max(zl.tolist()),) and z.dtype == torch.float32
    full, fl = mod(clean, lengths=torch.tensor([T] * B))
    dense = mod(clean)
    assert isinstance(dense, torch.Tensor) and full.shape == dense.shape and fl.tolist() == [dense.shape[-1]] * B
    for b, n in enumerate(lens):
        want, r32 = _module_truth(audio[b, :, :n], taps)
        _bar(f"module {shape} row {b}", z[b, ..., : zl[b]].reshape(D, -1).cpu(), want, r32)
        assert _zero_bits(z[b, ..., zl[b] :])
        alone = mod(dev[b : b + 1, ..., :n].contiguous(), lengths=torch.tensor([n]))[0]
        assert torch.equal(alone[0], z[b, ..., : zl[b]])
        if n < T:
            want, r32 = _module_truth(audio[b], taps)
        _bar(f"module {shape} row {b}, all lengths = T", full[b].reshape(D, -1).cpu(), want, r32)


def test_refusals_come_before_any_launch():
    a, mod = torch.randn(2, 4000).cuda(), LA.HipDereverbWPE()
    for lengths, match in (([4000, 256], r"lengths\[1\] = 256"), ([4001, 4000], r"lengths\[0\] = 4001"), ([4000], "shape"), ([[4000, 4000]], "shape")):
        with pytest.raises(ValueError, match=match):
            mod(a, lengths=torch.tensor(lengths))
    with pytest.raises(NotImplementedError, match="n_fft"):
        LA.HipDereverbWPE(n_fft=384, hop_length=96)(a, lengths=torch.tensor([4000, 4000]))
    with pytest.raises(NotImplementedError, match="hop_length"):
        LA.wpe_stft_on_device(a, torch.tensor([4000, 4000]), 512, 100)
    with pytest.raises(ValueError, match=r"frames\[0\] = 41"):
        LA.wpe_on_device(torch.zeros(1, 1, 17, 40, dtype=torch.complex64).cuda(), frames=torch.tensor([41]))
    assert isinstance(mod(a), torch.Tensor)  # without lengths: today's path and its single tensor
