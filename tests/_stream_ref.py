"""Test infrastructure of the ``online_inference`` tests: the framing of a stream restated in numpy, and the statements the device is held to.

``online_inference(x, context)`` of the reference (layers.py:199-224, 326-333, 775-856) frames a VIRTUAL waveform ``V = [A | x]``: ``A`` is
the context, or at the start of a stream nothing (``snip_edges``) / the flipped first ``min(P, S)`` samples of the chunk, ``P = (N - s) // 2``.
Frame f is ``V[f s : f s + N]`` for ``f < T = 1 + (L - N) // s`` -- which is exactly ``snip_edges=True`` framing of ``V`` -- and the remainder is
``V[:, T s:]``.  So every statement about a call is a statement of the existing oracles about ``V`` with ``snip_edges=True``:

  ``ref32`` / ``truth``   ``_stft_ref.ref32`` / ``_stft_ref.truth`` on ``V`` (frames, log-energies, spectrum), with the bars ``_stft_ref.hold``;
  ``features_truth``      ``oracle.kaldi_ref.RefExtractor`` in float64 on the frames of ``V``, with the bars of tests/test_gpu_layers.py
                          (``hold_features``: copied from there unchanged).

tests/test_stream_reference.py holds ``virtual`` / ``split`` / ``ref32`` to the live layers with torch.equal.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Sequence, Tuple

import numpy as np

import _stft_ref as R
from oracle import kaldi_ref as K

LAYERS = ["Wav2Win", "Wav2FFT", "Wav2Spec", "Wav2LogSpec", "Wav2LogFilterBank", "Wav2MFCC"]
KINDS = {"Wav2Spec": "spectrogram", "Wav2LogSpec": "log-spectrogram", "Wav2LogFilterBank": "fbank", "Wav2MFCC": "mfcc"}


def virtual(x: np.ndarray, context: Optional[np.ndarray], n: int, shift: int, snip_edges: bool) -> np.ndarray:
    """V = [A | x] for a (B, S) chunk and a (B, R) context (None: the start of a stream)."""
    if context is not None:
        assert context.ndim == 2 and context.shape[0] == x.shape[0]
        return np.concatenate([context, x], axis=1)
    if snip_edges:
        return x.copy()
    head = min((n - shift) // 2, x.shape[1])  # a first chunk shorter than P reflects only what it has
    return np.concatenate([x[:, :head][:, ::-1], x], axis=1)


def counts(length: int, n: int, shift: int) -> Tuple[int, int]:
    """(T, remainder length) of a virtual waveform of `length` samples; no frame when it is shorter than one."""
    T = 1 + (length - n) // shift if length >= n else 0
    return T, length - T * shift


def split(V: np.ndarray, n: int, shift: int) -> Tuple[int, np.ndarray]:
    T, _ = counts(V.shape[1], n, shift)
    return T, np.ascontiguousarray(V[:, T * shift:])


def snipped(cfg: K.RefConfig) -> K.RefConfig:
    return dataclasses.replace(cfg, snip_edges=True)


def ref32(V: np.ndarray, cfg: K.RefConfig, pad: Optional[int] = None):
    return R.ref32(V, snipped(cfg), pad)


def truth(V: np.ndarray, cfg: K.RefConfig, pad: Optional[int] = None):
    return R.truth(V, snipped(cfg), pad)


def feature_config(layer) -> Tuple[K.RefConfig, str]:
    """RefConfig of a feature layer (ours or the reference's: same attributes) and its kind."""
    kind = KINDS[type(layer).__name__.replace("Hip", "")]
    opts = {k: getattr(layer, k) for k in K.RefConfig.__dataclass_fields__ if hasattr(layer, k)}
    return K.RefConfig(**{**opts, "kind": kind}), kind


def features_truth(V: np.ndarray, cfg: K.RefConfig) -> np.ndarray:
    """(B, L) -> (B, T, F) float64: RefExtractor on the frames of V."""
    ref = K.RefExtractor(cfg, np.float64)
    T, _ = counts(V.shape[1], ref.n, ref.shift)
    if T == 0 or V.shape[0] == 0:
        return np.zeros((V.shape[0], T, ref.feature_dim))
    return np.stack([ref.from_frames(K.frames_from_wave(row.astype(np.float64), ref.n, ref.shift, True)) for row in V])


def hold_features(kind: str, use_energy: bool, got: np.ndarray, want: np.ndarray) -> None:
    """The bounds of tests/test_gpu_layers.py::test_layer_forward_matches_the_oracle for one (T, F) row block, unchanged."""
    assert got.shape == want.shape, (got.shape, want.shape)
    if kind == "spectrogram":
        tol = np.broadcast_to(1e-4 * np.abs(want[:, 1:]).max(axis=1, keepdims=True) + 1e-7, want.shape).copy()
        if use_energy:
            tol[:, 0] = 1e-4  # column 0 holds the log-energy
        assert np.all(np.abs(got - want) <= tol)
    elif kind == "mfcc":
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-4
    else:
        err = np.abs(got - want)
        # log domain: 1e-4 relative = 1e-4 absolute; bins at the float32 noise floor of their frame are bounded in the linear domain
        loud = want >= want.max(axis=1, keepdims=True) - 14.0
        assert err[loud].max() <= 2e-4, err[loud].max()
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-4


def chunked(x: np.ndarray, sizes: Sequence[int]) -> List[np.ndarray]:
    assert sum(sizes) == x.shape[1], (sum(sizes), x.shape)
    edges = np.cumsum([0] + list(sizes))
    return [np.ascontiguousarray(x[:, a:b]) for a, b in zip(edges[:-1], edges[1:])]


def walk(x: np.ndarray, sizes: Sequence[int], n: int, shift: int, snip_edges: bool, context: Optional[np.ndarray] = None):
    """The restated stream: per call (chunk, context it gets, V, T, remainder it returns)."""
    calls = []
    for chunk in chunked(x, sizes):
        V = virtual(chunk, context, n, shift, snip_edges)
        T, remainder = split(V, n, shift)
        calls.append((chunk, context, V, T, remainder))
        context = remainder
    return calls


# ---- goldens: tests/golden/stream.npz, written by tests/_stream_golden.py from the LIVE layers -------------------------------------
# name -> (reference class, constructor arguments, batch, chunk sizes): every call has at least one frame (the reference raises otherwise)
GOLDEN_CASES = {
    "win-16k": ("Wav2Win", dict(pad_length=401, return_log_energy=True), 2, (560, 333, 487)),
    "win-8k-snip": ("Wav2Win", dict(sampling_rate=8000, snip_edges=True, window_type="hamming", raw_energy=False, return_log_energy=True), 1, (280, 170, 250)),
    "fft-16k": ("Wav2FFT", dict(), 2, (560, 333, 487)),
    "fft-8k-plain": ("Wav2FFT", dict(sampling_rate=8000, use_energy=False, remove_dc_offset=False, preemph_coeff=0.0, window_type="hanning"), 1, (280, 170, 250)),
    "spec-16k": ("Wav2Spec", dict(), 1, (560, 333, 487)),
    "logspec-8k": ("Wav2LogSpec", dict(sampling_rate=8000, use_energy=False), 1, (280, 170, 250)),
    "fbank-16k": ("Wav2LogFilterBank", dict(), 2, (560, 333, 487)),
    "fbank-8k-energy": ("Wav2LogFilterBank", dict(sampling_rate=8000, num_filters=23, use_energy=True, snip_edges=True), 2, (280, 170, 250)),
    "mfcc-16k": ("Wav2MFCC", dict(), 2, (560, 333, 487)),
}


def golden_input(name: str) -> np.ndarray:
    _, _, batch, sizes = GOLDEN_CASES[name]
    return R.signal(sorted(GOLDEN_CASES).index(name) + 41, batch, sum(sizes))


def golden_feature_config(name: str) -> K.RefConfig:
    """RefConfig of a feature case: the constructor arguments over the layers' own defaults (where they differ from RefConfig's)."""
    cls, kw, _, _ = GOLDEN_CASES[name]
    defaults = dict(Wav2Spec=dict(use_energy=True), Wav2LogSpec=dict(use_energy=True), Wav2LogFilterBank=dict(num_filters=80), Wav2MFCC=dict(num_filters=23))[cls]
    return K.RefConfig(**{"kind": KINDS[cls], **defaults, **kw})


def stft_config(kw: dict, energy_key: str) -> K.RefConfig:
    """RefConfig of a Wav2Win / Wav2FFT constructor call (energy_key: return_log_energy / use_energy)."""
    opts = {k: v for k, v in kw.items() if k not in ("pad_length", "return_log_energy", "use_energy")}
    default = energy_key == "use_energy"  # Wav2FFT asks for the energy by default, Wav2Win does not
    return R.config(opts.pop("sampling_rate", 16000), kw.get(energy_key, default), **opts)
