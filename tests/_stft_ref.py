"""Test infrastructure of the Wav2Win / Wav2FFT tests: the two statements the device output is held to, and the bars.

``ref32``   the reference's own float32 torch call sequence (Wav2Win._forward_strided layers.py:151-187, Wav2FFT._forward_strided
            layers.py:309-320) on ``oracle.kaldi_torch.TorchKaldi``'s ``_strided``, ``_log_energy`` and window -- the pieces that
            tests/test_oracle.py holds to the live layers bit for bit; tests/test_stft_reference.py holds THIS composition to the live
            ``Wav2Win`` / ``Wav2FFT`` with torch.equal.
``truth``   the same arithmetic in float64 on the same float32 samples: ``kaldi_ref.frames_from_wave`` + ``preprocess_frames`` and
            ``np.fft.rfft`` of those.

Bars (``hold``): with y the device output, r = ref32, t = truth,
  1. per frame |y - t| <= 1e-4 max|t_frame| + 1e-7 elementwise (frames; re and im), every log-energy within 1e-4 -- the standing bound of
     tests/test_gpu_layers.py;
  2. E(y) <= 2 E(r), E(.) = max over non-zero frames of ||._f - t_f||_2 / ||t_f||_2; where E(r) == 0 the output equals r bit for bit.
"""
from __future__ import annotations

import itertools
from typing import Optional, Tuple

import numpy as np
import torch

from oracle import kaldi_ref as K
from oracle.kaldi_torch import TorchKaldi

# sampling_rate, N, fft_length (25 ms frames, 10 ms shift)
RATES = [(16000, 400, 512), (8000, 200, 256), (22050, 551, 1024), (48000, 1200, 2048)]
WINDOWS = ["povey", "hanning", "hamming", "rectangular", "blackman"]


def config(sampling_rate: int, want_energy: bool = True, **opts) -> K.RefConfig:
    return K.RefConfig(kind="spectrogram", sampling_rate=sampling_rate, use_energy=want_energy, **opts)


def option_grid(sampling_rate: int):
    """snip_edges x remove_dc_offset x preemph_coeff x window x raw_energy x energy on / off: 160 configurations."""
    for snip, dc, pre, win, raw, en in itertools.product((False, True), (True, False), (0.97, 0.0), WINDOWS, (True, False), (True, False)):
        yield config(sampling_rate, en, snip_edges=snip, remove_dc_offset=dc, preemph_coeff=pre, window_type=win, raw_energy=raw)


def layer_kwargs(cfg: K.RefConfig) -> dict:
    """The constructor arguments Wav2Win and Wav2FFT share (without pad_length / round_to_power_of_two / the energy switch)."""
    return dict(sampling_rate=cfg.sampling_rate, frame_length=cfg.frame_length, frame_shift=cfg.frame_shift, remove_dc_offset=cfg.remove_dc_offset,
                preemph_coeff=cfg.preemph_coeff, window_type=cfg.window_type, dither=0.0, snip_edges=cfg.snip_edges, energy_floor=cfg.energy_floor,
                raw_energy=cfg.raw_energy)


@torch.no_grad()
def ref32_tensors(x: torch.Tensor, cfg: K.RefConfig, pad: Optional[int] = None, spectrum: bool = True):
    """The call sequence itself on a (B, S) float32 tensor with at least one frame, on the tensor's device -> (frames, log-energies or
    None, spectrum or None)."""
    tk = TorchKaldi(cfg)
    pad = tk.fft if pad is None else pad
    window = tk.window.to(x.device)
    xs = tk._strided(x)
    if cfg.remove_dc_offset:
        mu = torch.mean(xs, dim=2, keepdim=True)
        xs = xs - mu
    log_e = None
    if cfg.use_energy and cfg.raw_energy:
        log_e = tk._log_energy(xs)
    if cfg.preemph_coeff != 0.0:
        off = torch.nn.functional.pad(xs, (1, 0), mode="replicate")
        xs = xs - cfg.preemph_coeff * off[:, :, :-1]
    xs = xs * window
    if pad != tk.n:
        xs = torch.nn.functional.pad(xs.unsqueeze(1), [0, pad - tk.n], mode="constant", value=0.0).squeeze(1)
    if cfg.use_energy and not cfg.raw_energy:
        log_e = tk._log_energy(xs)
    if not spectrum:
        return xs, log_e, None
    X = torch.fft.rfft(xs, dim=-1)
    if cfg.use_energy and log_e is not None:
        X[:, :, 0] = log_e
    return xs, log_e, X


def ref32(x: np.ndarray, cfg: K.RefConfig, pad: Optional[int] = None) -> Tuple[np.ndarray, Optional[np.ndarray], np.ndarray]:
    """(B, S) float32 -> (frames (B, T, pad) float32, log-energies (B, T) float32 or None, spectrum (B, T, pad / 2 + 1) complex64 with the
    log-energy in bin 0 when cfg.use_energy).  pad defaults to the fft length."""
    n, shift, fft = K.window_sizes(cfg)
    pad = fft if pad is None else pad
    B, S = x.shape
    T = K.num_frames(S, n, shift, cfg.snip_edges)
    if B == 0 or T == 0:
        return (np.zeros((B, T, pad), np.float32), np.zeros((B, T), np.float32) if cfg.use_energy else None, np.zeros((B, T, pad // 2 + 1), np.complex64))
    xs, log_e, X = ref32_tensors(torch.from_numpy(np.ascontiguousarray(x)), cfg, pad)
    return xs.numpy(), (None if log_e is None else log_e.numpy()), X.numpy()


def truth(x: np.ndarray, cfg: K.RefConfig, pad: Optional[int] = None) -> Tuple[np.ndarray, Optional[np.ndarray], np.ndarray]:
    """The same three arrays in float64 / complex128 (raises ValueError where the reflection needs more samples than the row has)."""
    n, shift, fft = K.window_sizes(cfg)
    pad = fft if pad is None else pad
    window = K.frame_window(n, cfg.window_type, np.float64)
    frames, energies, spectra = [], [], []
    for row in np.asarray(x, dtype=np.float64):
        f, e = K.preprocess_frames(K.frames_from_wave(row, n, shift, cfg.snip_edges), cfg, window, pad, cfg.use_energy)
        X = np.fft.rfft(f, axis=-1)
        if e is not None:
            X[:, 0] = e
        frames.append(f), energies.append(e), spectra.append(X)
    T = K.num_frames(x.shape[1], n, shift, cfg.snip_edges)
    if not frames:
        return np.zeros((0, T, pad)), (np.zeros((0, T)) if cfg.use_energy else None), np.zeros((0, T, pad // 2 + 1), np.complex128)
    return np.stack(frames), (np.stack(energies) if cfg.use_energy else None), np.stack(spectra)


def _flat(a: np.ndarray) -> np.ndarray:
    """(B, T, W) real or complex -> (B * T, W') float64 rows (re and im side by side)."""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        a = np.stack([a.real, a.imag], axis=-1)
    return a.astype(np.float64).reshape(a.shape[0] * a.shape[1], -1)


def frame_error(a: np.ndarray, t: np.ndarray) -> float:
    """E(a): max over the non-zero frames of t of ||a_f - t_f||_2 / ||t_f||_2 (0.0 when every frame of t is zero)."""
    a, t = _flat(a), _flat(t)
    norm = np.linalg.norm(t, axis=1)
    live = norm > 0
    return float((np.linalg.norm(a - t, axis=1)[live] / norm[live]).max()) if live.any() else 0.0


def hold(label: str, y: np.ndarray, r: np.ndarray, t: np.ndarray, energy_bin: bool = False) -> Tuple[float, float]:
    """Both bars for one output (frames or spectrum); returns (E(y), E(r)).  `energy_bin`: column 0 of the spectrum holds the log-energy,
    whose bar is 1e-4 absolute."""
    assert y.shape == r.shape == t.shape, (label, y.shape, r.shape, t.shape)
    yf, tf = _flat(y), _flat(t)
    tol = np.broadcast_to(1e-4 * np.abs(tf).max(axis=1, keepdims=True) + 1e-7, tf.shape).copy() if tf.size else np.zeros(tf.shape)
    if energy_bin and tf.size:
        tol[:, 0] = 1e-4
    worst = float((np.abs(yf - tf) - tol).max()) if tf.size else -1.0
    ey, er = frame_error(y, t), frame_error(r, t)
    print(f"[stft] {label}: E(device) {ey:.3g}  E(ref32) {er:.3g}  ratio {ey / er if er > 0 else float('nan'):.3g}  bar-1 slack {-worst:.3g}")
    assert worst <= 0.0, (label, worst)
    if er == 0.0:
        assert np.array_equal(np.asarray(y), np.asarray(r)), (label, "E(ref32) == 0: the output must equal the reference bit for bit")
    else:
        assert ey <= 2.0 * er, (label, ey, er)
    return ey, er


def hold_energy(label: str, e: np.ndarray, t: np.ndarray) -> None:
    assert e.shape == t.shape, (label, e.shape, t.shape)
    if t.size:
        worst = float(np.abs(e.astype(np.float64) - t).max())
        assert worst <= 1e-4, (label, worst)


def shortest_reflectable(n: int, shift: int) -> int:
    """The fewest samples frame_indices accepts without snip_edges: a frame exists and both reflections fit into the row."""
    for s in range(1, 4 * n):
        if K.num_frames(s, n, shift, False) == 0:
            continue
        try:
            K.frame_indices(s, n, shift, False)
            return s
        except ValueError:
            continue
    raise AssertionError("no length below 4 N is accepted")


def lengths(n: int, shift: int, snip_edges: bool):
    """Row lengths giving 1, 2, 3 and 5 frames (and their neighbours): S = k shift + r with r in {0, shift/2 - 1, shift/2, shift - 1}, which
    flips the rounding of the frame count and the sign of the right reflection; with snip_edges the same remainders behind N + (k - 1) shift."""
    out = []
    for k in (1, 2, 3, 5):
        for r in (0, shift // 2 - 1, shift // 2, shift - 1):
            out.append((n + (k - 1) * shift if snip_edges else k * shift) + r)
    return out


def signal(seed: int, batch: int, num_samples: int) -> np.ndarray:
    """Noise with a DC offset and a slow sine, float32."""
    rng = np.random.RandomState(seed)
    t = np.arange(num_samples)
    x = 0.1 * rng.standard_normal((batch, num_samples)) + 0.05 + 0.2 * np.sin(2 * np.pi * t / 97.0 + rng.rand(batch, 1))
    return x.astype(np.float32)


# name -> (sampling_rate, options of `config`, pad_length of the Wav2Win case (None: N), (batch, frames)): tests/golden/stft.npz holds, per
# case, the input `x` and what the LIVE Wav2Win(pad_length, return_log_energy=want_energy) and Wav2FFT(use_energy=want_energy) returned
GOLDEN_CASES = {
    "16k-default": (16000, dict(), None, (2, 5)),
    "16k-rectangular-plain": (16000, dict(window_type="rectangular", remove_dc_offset=False, preemph_coeff=0.0, raw_energy=False), 401, (1, 3)),
    "8k-snip-hamming": (8000, dict(snip_edges=True, window_type="hamming", raw_energy=False), 256, (2, 3)),
    "22k-odd-blackman": (22050, dict(window_type="blackman", remove_dc_offset=False), 552, (1, 4)),
    "48k-hanning-no-energy": (48000, dict(want_energy=False, window_type="hanning", preemph_coeff=0.0), 1201, (1, 3)),
}


def golden_case(name: str):
    """(cfg, pad_length of the frames case, input (B, S) float32)."""
    rate, opts, pad, (batch, frames) = GOLDEN_CASES[name]
    cfg = config(rate, **opts)
    n, shift, _ = K.window_sizes(cfg)
    S = (n + (frames - 1) * shift if cfg.snip_edges else frames * shift) + 17
    assert K.num_frames(S, n, shift, cfg.snip_edges) == frames
    return cfg, (n if pad is None else pad), signal(sorted(GOLDEN_CASES).index(name) + 11, batch, S)
