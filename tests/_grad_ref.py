"""Test infrastructure of the waveform-gradient tests: a differentiable restatement of the six layers, the golden cases and the bars.

``forward(cls, kw, x)``  the six forwards of lhotse/features/kaldi/layers.py as torch ops in the dtype of ``x`` (float32 or float64), written
    from the statement in include/hipfeat.h (the gradient block): the frames of the index map as a strided view, d = s - mean(s), the raw
    log-energy, p_i = d_i - c d_{max(i-1,0)}, w = p win, zero padding, the windowed log-energy, X = rfft(w), then power / magnitude, log,
    mel, DCT and lifter.  The tables are those of lhotse_amd.constants, which tests/test_constants.py holds to the reference's bit for
    bit.  Autograd through it is the gradient the device is held to where no golden exists (edge lengths, overlap, FFT sizes).
``CASES``   the golden cases: tests/golden/grad.npz holds per case the input ``x``, the cotangent(s) and what the LIVE reference layer's
    autograd returned in float32 (``g32``) and, after ``.to(torch.float64)``, in float64 (``g64``); for the linear kinds also the
    relative adjoint gap of the reference's float32 forward / autograd (``gap32``).  tests/_grad_golden.py writes the file.

Bars.  Per row, with E(g) = ||g - g64||_2 / ||g64||_2:  E(device) <= max(2 E(g32), 1e-6).  The factor 2 is the bar the STFT and stream tests
use against ref32 (a different FFT order, the same precision); 1e-6 (about 16 float32 ulp) keeps the bar from being zero where the
reference happens to be exact.  A row with g64 == 0 must be exactly zero and finite.
"""
from __future__ import annotations

import math
import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from lhotse_amd import constants

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "grad.npz")
FLOOR_BAR = 1e-6
EPSILON = 1.1920928955078125e-07  # lhotse.utils.EPSILON = torch.finfo(torch.float32).eps: the default energy_floor

CLASSES = ("Wav2Win", "Wav2FFT", "Wav2Spec", "Wav2LogSpec", "Wav2LogFilterBank", "Wav2MFCC")


def sizes(kw: dict, cls: str) -> Tuple[int, int, int]:
    """(frame length, shift, fft or pad length) in samples."""
    rate = kw.get("sampling_rate", 16000)
    n, shift, fft = constants.frame_sizes(rate, kw.get("frame_length", 0.025), kw.get("frame_shift", 0.01), kw.get("round_to_power_of_two", True))
    if cls == "Wav2Win":
        fft = n if kw.get("pad_length") is None else kw["pad_length"]
    return n, shift, fft


def num_frames(S: int, n: int, shift: int, snip_edges: bool) -> int:
    if snip_edges:
        return 0 if S < n else 1 + (S - n) // shift
    return (S + shift // 2) // shift


def frame_index(S: int, n: int, shift: int, snip_edges: bool) -> np.ndarray:
    """(T, n) int64: the sample every tap of every frame reads (layers.py:747-772 as an index map)."""
    T = num_frames(S, n, shift, snip_edges)
    left = 0 if snip_edges else (n - shift) // 2
    j = np.arange(T, dtype=np.int64)[:, None] * shift - left + np.arange(n, dtype=np.int64)[None, :]
    j = np.where(j < 0, -j - 1, j)
    j = np.where(j >= S, 2 * S - 1 - j, j)
    assert T == 0 or (j.min() >= 0 and j.max() < S), "the row is shorter than its reflection"
    return j


def frames(x: torch.Tensor, n: int, shift: int, snip_edges: bool) -> torch.Tensor:
    """(B, S) -> (B, T, n): frame t is the row extended by its mirror images at both ends, from t shift on -- ``frame_index`` as a
    strided view, so that autograd sums the overlapping taps in the order it does for the reference."""
    B, S = x.shape
    T = num_frames(S, n, shift, snip_edges)
    if not snip_edges:
        left = (n - shift) // 2
        right = (T - 1) * shift + n - S - left
        assert T > 0 and left <= S and right <= S, "the row is shorter than its reflection"
        parts = [x[:, :left].flip(1), x] + ([x[:, S - right:].flip(1)] if right > 0 else [])
        x = torch.cat(parts, dim=1)
    return x.as_strided((B, T, n), (x.stride(0), shift * x.stride(1), x.stride(1)))


def _log_energy(v: torch.Tensor, floor: float) -> torch.Tensor:
    e = (v.pow(2).sum(-1) + 1e-15).log()
    if floor > 0.0:
        e = torch.max(e, torch.tensor(math.log(floor), dtype=e.dtype, device=e.device))
    return e


def mel_filters(cls: str, kw: dict) -> np.ndarray:
    """(fft / 2 + 1, num_filters) float32: the Kaldi filters, or with ``torchaudio_compatible_mel_scale=False`` the HTK ones (with or
    without ``norm_filters``); tests/test_constants.py holds both matrices to the reference's."""
    rate, fft = kw.get("sampling_rate", 16000), sizes(kw, cls)[2]
    M = kw.get("num_filters", 80 if cls == "Wav2LogFilterBank" else 23)
    low, high = kw.get("low_freq", 20.0), kw.get("high_freq", -400.0)
    if kw.get("torchaudio_compatible_mel_scale", True):
        return constants.make_kaldi_mel(M, fft, rate, low, high)
    return constants.make_htk_mel(M, fft, rate, low, high, kw.get("norm_filters", False))


def forward(cls: str, kw: dict, x: torch.Tensor):
    """``x``: (B, S) float32 or float64 (it may require a gradient) -> what the layer returns, in that dtype (Wav2FFT: its complex type;
    Wav2Win: the tuple (frames, log-energies or None))."""
    dt = x.dtype
    n, shift, fft = sizes(kw, cls)
    snip = kw.get("snip_edges", False)
    energy = kw.get("return_log_energy", False) if cls == "Wav2Win" else kw.get("use_energy", cls in ("Wav2FFT", "Wav2Spec", "Wav2LogSpec"))
    raw = kw.get("raw_energy", True)
    floor = kw.get("energy_floor", EPSILON)
    c = kw.get("preemph_coeff", 0.97)
    window = torch.from_numpy(constants.make_window(n, kw.get("window_type", "povey"))).to(device=x.device, dtype=dt)
    s = frames(x, n, shift, snip)  # (B, T, n)
    d = s - s.mean(dim=2, keepdim=True) if kw.get("remove_dc_offset", True) else s
    log_e: Optional[torch.Tensor] = _log_energy(d, floor) if energy and raw else None
    p = d - c * torch.nn.functional.pad(d, (1, 0), mode="replicate")[:, :, :-1] if c != 0.0 else d
    w = p * window
    if fft != n:
        w = torch.nn.functional.pad(w, (0, fft - n))
    if energy and not raw:
        log_e = _log_energy(w, floor)
    if cls == "Wav2Win":
        return w, log_e
    X = torch.fft.rfft(w, dim=-1)
    if cls == "Wav2FFT":
        if energy:
            X = torch.cat([log_e.unsqueeze(-1).to(X.dtype), X[:, :, 1:]], dim=-1)
        return X
    P = X.abs() if kw.get("use_fft_mag", False) else X.abs() ** 2
    if cls in ("Wav2Spec", "Wav2LogSpec"):
        if cls == "Wav2LogSpec":
            P = (P + 1e-15).log()
        if energy:
            P = torch.cat([log_e.unsqueeze(-1), P[:, :, 1:]], dim=-1)
        return P
    M = kw.get("num_filters", 80 if cls == "Wav2LogFilterBank" else 23)
    fb = mel_filters(cls, kw)
    # (K, M) as the transposed view of an (M, K) matrix, which is how the reference holds it (layers.py:553): the matrix product then
    # sums in the reference's order
    fb = torch.from_numpy(np.ascontiguousarray(fb.T)).to(device=x.device, dtype=dt).T
    mel = torch.max(torch.matmul(P, fb), torch.tensor(constants.MEL_FLOOR, dtype=dt, device=x.device)).log()
    if cls == "Wav2LogFilterBank":
        return torch.cat([log_e.unsqueeze(-1), mel], dim=-1) if energy else mel
    C, q = kw.get("num_ceps", 13), kw.get("cepstral_lifter", 22)
    out = torch.matmul(mel, torch.from_numpy(constants.make_dct(C, M)).to(device=x.device, dtype=dt))
    if q > 0:
        out = out * torch.from_numpy(constants.make_lifter(C, q)).to(device=x.device, dtype=dt)
    if energy:  # C0 is replaced (the documented forward of HipWav2MFCC; the reference raises a shape error there)
        out = torch.cat([log_e.unsqueeze(-1), out[:, :, 1:]], dim=-1)
    return out


def outputs(res) -> Tuple[torch.Tensor, ...]:
    """The differentiable outputs of a layer's result as a tuple of tensors (Wav2Win without log-energies: the frames alone)."""
    if isinstance(res, tuple):
        return tuple(r for r in res if r is not None)
    return (res,)


def gradient(cls: str, kw: dict, x: np.ndarray, cots, dtype=torch.float64) -> np.ndarray:
    """The gradient of sum_i <out_i, cot_i> (real inner product: re * re + im * im) with respect to ``x`` through ``forward``."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_(True)
    outs = outputs(forward(cls, kw, xt))
    loss = pairing(outs, cots, dtype)
    if not loss.requires_grad:
        return np.zeros(x.shape, dtype=np.float64 if dtype == torch.float64 else np.float32)
    loss.backward()
    return xt.grad.numpy()


def pairing(outs, cots, dtype) -> torch.Tensor:
    """sum_i <out_i, cot_i> as a scalar of ``dtype``: for a complex output Re(out) Re(cot) + Im(out) Im(cot), torch's convention for the
    cotangent a + ib of a real loss dL = a dRe + b dIm."""
    total = torch.zeros((), dtype=dtype)
    for o, c in zip(outs, cots):
        if c is None:
            continue
        c = torch.as_tensor(c)
        if o.is_complex():
            o, c = torch.view_as_real(o), torch.view_as_real(c.to(torch.complex128 if dtype == torch.float64 else torch.complex64))
        total = total + (o.to(dtype) * c.to(dtype)).sum()
    return total


def row_error(g: np.ndarray, g64: np.ndarray) -> np.ndarray:
    """E(g) per row; rows with g64 == 0 give 0.0 when g is zero as well and inf otherwise."""
    g, g64 = np.asarray(g, dtype=np.float64), np.asarray(g64, dtype=np.float64)
    norm = np.linalg.norm(g64, axis=1)
    err = np.linalg.norm(g - g64, axis=1)
    return np.where(norm > 0, err / np.where(norm > 0, norm, 1.0), np.where(err > 0, np.inf, 0.0))


def hold(label: str, g: np.ndarray, g32: np.ndarray, g64: np.ndarray) -> float:
    """The golden bar for one case; prints every figure before it asserts and returns the worst E(device) / E(g32) of the rows whose
    bar is the reference's own error."""
    assert g.shape == g64.shape and g.dtype == np.float32, (label, g.shape, g.dtype)
    assert np.isfinite(g).all(), label
    ed, er = row_error(g, g64), row_error(g32, g64)
    worst = 0.0
    for b in range(g.shape[0]):
        if not np.any(g64[b]):
            print(f"[grad] {label} row {b}: g64 == 0, device max |g| {np.abs(g[b]).max():.3g}")
            assert not np.any(g[b]), (label, b, "a row with a zero gradient must be exactly zero")
            continue
        bar = max(2.0 * er[b], FLOOR_BAR)
        ratio = ed[b] / er[b] if er[b] > 0 else float("nan")
        print(f"[grad] {label} row {b}: E(device) {ed[b]:.3g}  E(g32) {er[b]:.3g}  ratio {ratio:.3g}  bar {bar:.3g}")
        if 2.0 * er[b] >= FLOOR_BAR:
            worst = max(worst, ratio)
    for b in range(g.shape[0]):
        if np.any(g64[b]):
            assert ed[b] <= max(2.0 * er[b], FLOOR_BAR), (label, b, ed[b], er[b])
    return worst


# ---- the golden cases ------------------------------------------------------------------------------------------------------------------------
# name -> (reference class, constructor arguments).  Every class; use_energy / return_log_energy, raw and windowed energy, use_fft_mag,
# energy_floor = 0, snip_edges, no DC removal, no pre-emphasis, hamming, and 8 / 16 / 22.05 / 44.1 kHz.
CASES: Dict[str, Tuple[str, dict]] = {
    "win-default": ("Wav2Win", dict()),
    "win-energy-raw": ("Wav2Win", dict(return_log_energy=True)),
    "win-energy-windowed-pad512": ("Wav2Win", dict(return_log_energy=True, raw_energy=False, pad_length=512)),
    "win-snip-hamming-plain": ("Wav2Win", dict(snip_edges=True, window_type="hamming", remove_dc_offset=False, preemph_coeff=0.0)),
    "fft-default": ("Wav2FFT", dict()),
    "fft-no-energy": ("Wav2FFT", dict(use_energy=False)),
    "fft-8k-no-energy-snip": ("Wav2FFT", dict(sampling_rate=8000, use_energy=False, snip_edges=True)),
    "fft-44k-windowed-energy": ("Wav2FFT", dict(sampling_rate=44100, raw_energy=False)),
    "spec-default": ("Wav2Spec", dict()),
    "spec-mag-no-energy": ("Wav2Spec", dict(use_fft_mag=True, use_energy=False)),
    "spec-22k-floor0": ("Wav2Spec", dict(sampling_rate=22050, energy_floor=0.0)),
    "spec-snip-no-dc": ("Wav2Spec", dict(snip_edges=True, remove_dc_offset=False)),
    "logspec-default": ("Wav2LogSpec", dict()),
    "logspec-mag-windowed": ("Wav2LogSpec", dict(use_fft_mag=True, raw_energy=False)),
    "logspec-8k-plain-hamming": ("Wav2LogSpec", dict(sampling_rate=8000, preemph_coeff=0.0, window_type="hamming", use_energy=False)),
    "fbank-default": ("Wav2LogFilterBank", dict()),
    "fbank-energy-raw": ("Wav2LogFilterBank", dict(use_energy=True)),
    "fbank-energy-windowed-floor0": ("Wav2LogFilterBank", dict(use_energy=True, raw_energy=False, energy_floor=0.0)),
    "fbank-mag-snip": ("Wav2LogFilterBank", dict(use_fft_mag=True, snip_edges=True)),
    "fbank-44k-128": ("Wav2LogFilterBank", dict(sampling_rate=44100, num_filters=128)),
    "fbank-22k-40-no-dc": ("Wav2LogFilterBank", dict(sampling_rate=22050, num_filters=40, remove_dc_offset=False)),
    "mfcc-default": ("Wav2MFCC", dict()),
    "mfcc-8k-lifter10": ("Wav2MFCC", dict(sampling_rate=8000, cepstral_lifter=10)),  # (the reference cannot be built without a lifter)
    "mfcc-mag-40x40-snip": ("Wav2MFCC", dict(use_fft_mag=True, num_filters=40, num_ceps=40, snip_edges=True)),
}
LINEAR = ("win-default", "win-snip-hamming-plain", "fft-no-energy", "fft-8k-no-energy-snip")


def case_input(name: str) -> np.ndarray:
    """(3, S) float32, S = 900 samples at 16 kHz and the same duration elsewhere: uniform noise of +-0.5 plus a tone (no bin sits at the
    float32 floor), on a grid of 2^-12 so that the file compresses; row 1 is all zeros, row 2 holds a stretch of two whole silent
    frames (frames 2 and 3)."""
    cls, kw = CASES[name]
    n, shift, _ = sizes(kw, cls)
    rate = kw.get("sampling_rate", 16000)
    S = 900 * rate // 16000
    rng = np.random.RandomState(1000 + sorted(CASES).index(name))
    t = np.arange(S)
    x = rng.uniform(-0.5, 0.5, size=(3, S)) + 0.25 * np.sin(2 * np.pi * 440.0 * t / rate + rng.rand(3, 1))
    x = np.round(x * 4096.0) / 4096.0
    x[1] = 0.0
    start = 2 * shift - (0 if kw.get("snip_edges", False) else (n - shift) // 2)
    x[2, start: start + n + shift] = 0.0
    assert start + n + shift < S
    return x.astype(np.float32)


def case_cotangents(name: str, shapes) -> list:
    """One cotangent per differentiable output, on a grid of 1 / 8 in [-1, 1] (complex for Wav2FFT)."""
    cls, _ = CASES[name]
    rng = np.random.RandomState(5000 + sorted(CASES).index(name))
    out = []
    for shape in shapes:
        c = rng.randint(-8, 9, size=shape).astype(np.float32) / 8.0
        if cls == "Wav2FFT":
            c = (c + 1j * (rng.randint(-8, 9, size=shape).astype(np.float32) / 8.0)).astype(np.complex64)
        out.append(c)
    return out


def load_golden() -> dict:
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_cotangents(gold: dict, name: str) -> list:
    return [gold[f"{name}/cot{i}"] for i in range(2) if f"{name}/cot{i}" in gold]


def hip_layer(cls: str, kw: dict):
    """The Hip* layer of a reference class and its arguments, in differentiable mode."""
    import warnings

    import lhotse_amd

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return getattr(lhotse_amd, "Hip" + cls)(**kw).differentiable_()


def device_gradient(layer, x: np.ndarray, cots, device="cuda") -> np.ndarray:
    """x.grad of sum_i <out_i, cot_i> through ``layer`` on the device, as float32 numpy."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(device).requires_grad_(True)
    outs = outputs(layer(xt))
    cots = [None if c is None else torch.as_tensor(c).to(device) for c in cots]
    keep = [(o, c) for o, c in zip(outs, cots) if c is not None]
    torch.autograd.backward([o for o, _ in keep], [c for _, c in keep])
    return xt.grad.cpu().numpy()
