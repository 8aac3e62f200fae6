"""The seeded sweep of the waveform gradient over the option surface, shared by tests/test_grad_sweep_reference.py (CPU: the restatement's
own error, the margins from the discontinuities and the coverage of the kept list) and tests/test_gpu_grad_sweep.py (the device under
``_grad_ref.hold``).  The pattern is that of tests/_random_cases.py: everything about case ``i`` derives from ``i``.

``sweep_case(i)``        (class, constructor arguments): uniform over the six classes and over the options of the table below.
``sweep_input(i)``       (3, S) float32, S = N + 5 shift + r, r in [0, shift): 6 to 9 frames, the smallest row with interior, left-reflected
                         and right-reflected frames.  ``_grad_ref.case_input``'s noise plus tone; row 1 is scaled by 0.02 and row 2 by
                         3e-4, so that under the energy floors 1e-3 and 1.0 the rows sit on different sides of the floor and row 2 is partly
                         mel-floored.
``sweep_cotangents``     standard normal float32, complex for Wav2FFT.
``reference(i)``         the restatement's float32 and float64 gradients and, in float64, what decides whether the case can hold a device
                         to them: the mel energies against MEL_FLOOR and the frame log-energies against log(energy_floor).
``EXCLUDED``             the cases whose float32 reference is itself off by more than CAP on some row, or which sit within MARGIN of a
                         discontinuity; tests/test_grad_sweep_reference.py asserts that each of them really does, and that they are few.

8 kHz at 16 ms is a frame of 128 samples, whose FFT size the gradient kernels do not have (that refusal is tested in
tests/test_gpu_grad.py): such a draw of a spectral class takes 32 ms, which is N == fft == 256.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import _grad_ref as GR
from lhotse_amd import constants

NUM_CASES = 160
SEED_BASE = 3000  # case i: RandomState(SEED_BASE + i); its input: SEED_BASE + 4000 + i; its cotangents: SEED_BASE + 6000 + i
CAP = 1e-3        # E(g32) of every row of a kept case: max(2 E(g32), 1e-6) is a bar only where g32 is itself accurate
MARGIN = 1e-4     # |mel / MEL_FLOOR - 1| and |log-energy - log(energy_floor)| of a kept case, in float64
FFT_SIZES = (256, 512, 1024, 2048)
SPECTRAL = GR.CLASSES[1:]
WINDOWS = ("povey", "hanning", "hamming", "rectangular", "blackman")

# index -> why the case cannot hold a device to its float32 reference (asserted in tests/test_grad_sweep_reference.py)
EXCLUDED = {
    # rectangular window, DC removal and no pre-emphasis: bin 0 is the sum of a mean-free frame, zero up to rounding, and the gradient
    # through 1 / (P_0 + 1e-15) is ill-conditioned in any float32
    77: "Wav2LogSpec, N == fft == 1024: E(g32) = 1.0e-2",
    92: "Wav2LogSpec at 48 kHz / 32 ms: E(g32) = 5.1e-3",
    85: "Wav2MFCC, 65 filters: a mel energy of the quiet row within 2.2e-5 of MEL_FLOOR",
}


def sweep_case(i: int):
    rng = np.random.RandomState(SEED_BASE + i)
    cls = str(rng.choice(GR.CLASSES))
    kw = dict(sampling_rate=int(rng.choice([8000, 16000, 16000, 22050, 24000, 32000, 44100, 48000])))
    kw["frame_length"] = float(rng.choice([0.025, 0.025, 0.02, 0.032, 0.016]))
    kw["frame_shift"] = min(float(rng.choice([0.01, 0.01, 0.0125, 0.008, 0.016])), kw["frame_length"])  # (so that shift == N occurs)
    kw["window_type"] = str(rng.choice(WINDOWS))
    kw["remove_dc_offset"] = bool(rng.rand() < 0.5)
    kw["preemph_coeff"] = float(rng.choice([0.97, 0.0, 0.9]))
    kw["snip_edges"] = bool(rng.rand() < 0.5)
    kw["return_log_energy" if cls == "Wav2Win" else "use_energy"] = bool(rng.rand() < 0.5)
    kw["raw_energy"] = bool(rng.rand() < 0.5)
    kw["energy_floor"] = float(rng.choice([GR.EPSILON, 0.0, 1e-3, 1.0]))
    if cls in ("Wav2Spec", "Wav2LogSpec", "Wav2LogFilterBank", "Wav2MFCC"):
        kw["use_fft_mag"] = bool(rng.rand() < 0.5)
    if cls in ("Wav2LogFilterBank", "Wav2MFCC"):
        kw["num_filters"] = int(rng.choice([23, 40, 64, 65, 80, 128]))
        kw["low_freq"] = float(rng.choice([20.0, 0.0, 60.0]))
        kw["high_freq"] = float(rng.choice([-400.0, 0.0, -100.0]))
        if rng.rand() < 0.15:
            kw["torchaudio_compatible_mel_scale"] = False
            kw["norm_filters"] = bool(rng.rand() < 0.5)
    if cls == "Wav2MFCC":
        kw["num_ceps"] = int(min(kw["num_filters"], rng.choice([13, 20, 23])))
        kw["cepstral_lifter"] = int(rng.choice([22, 10, 0]))
    if cls != "Wav2Win" and GR.sizes(kw, cls)[2] not in FFT_SIZES:
        kw["frame_length"] = 0.032  # 8 kHz at 16 ms (see the module's docstring)
    if cls == "Wav2Win" and rng.rand() < 0.5:
        kw["pad_length"] = int(GR.sizes(kw, cls)[0] + rng.choice([1, 3, 112]))
    return cls, kw


def sweep_input(i: int) -> np.ndarray:
    cls, kw = sweep_case(i)
    n, shift, _ = GR.sizes(kw, cls)
    rng = np.random.RandomState(SEED_BASE + 4000 + i)
    S = n + 5 * shift + int(rng.randint(0, shift))
    t = np.arange(S)
    x = rng.uniform(-0.5, 0.5, size=(3, S)) + 0.25 * np.sin(2 * np.pi * 440.0 * t / kw["sampling_rate"] + rng.rand(3, 1))
    x[1] *= 0.02
    x[2] *= 3e-4
    return x.astype(np.float32)


def sweep_cotangents(i: int, shapes) -> list:
    cls, _ = sweep_case(i)
    rng = np.random.RandomState(SEED_BASE + 6000 + i)
    out = []
    for shape in shapes:
        c = rng.standard_normal(shape).astype(np.float32)
        if cls == "Wav2FFT":
            c = (c + 1j * rng.standard_normal(shape).astype(np.float32)).astype(np.complex64)
        out.append(c)
    return out


def energy_flag(cls: str, kw: dict) -> bool:
    return bool(kw["return_log_energy" if cls == "Wav2Win" else "use_energy"])


_FRONT = ("sampling_rate", "frame_length", "frame_shift", "window_type", "remove_dc_offset", "preemph_coeff", "snip_edges", "raw_energy")


def unfloored_log_energy(cls: str, kw: dict, x: np.ndarray) -> np.ndarray:
    """(3, T) float64: the frame log-energies the case's output carries, before the energy floor."""
    front = {k: kw[k] for k in _FRONT}
    _, log_e = GR.forward("Wav2Win", dict(front, return_log_energy=True, energy_floor=0.0), torch.from_numpy(x).double())
    return log_e.numpy()


def unfloored_mel(cls: str, kw: dict, x: np.ndarray) -> np.ndarray:
    """(3, T, num_filters) float64: the mel energies of a filterbank or MFCC case, before MEL_FLOOR."""
    front = {k: kw[k] for k in _FRONT}
    P = GR.forward("Wav2Spec", dict(front, use_fft_mag=kw["use_fft_mag"], use_energy=False), torch.from_numpy(x).double())
    return P.numpy() @ GR.mel_filters(cls, kw).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(i: int) -> dict:
    """Case ``i`` through the restatement: ``x``, ``cots``, ``g32``, ``g64``, ``e32`` (E(g32) per row), and in float64 ``mel_margin`` (the
    smallest |mel / MEL_FLOOR - 1|, inf without a filterbank), ``mel_floored`` (the share of a row's mel energies at or under the floor,
    None without a filterbank), ``energy_margin`` (the smallest |log-energy - log(energy_floor)|, inf where no energy is asked for or the
    floor is 0) and ``energy_floored`` (per row the share of frames whose log-energy the floor replaced, None likewise)."""
    cls, kw = sweep_case(i)
    x = sweep_input(i)
    shapes = [tuple(o.shape) for o in GR.outputs(GR.forward(cls, kw, torch.from_numpy(x)))]
    cots = sweep_cotangents(i, shapes)
    g64, g32 = GR.gradient(cls, kw, x, cots, torch.float64), GR.gradient(cls, kw, x, cots, torch.float32)
    ref = dict(cls=cls, kw=kw, x=x, cots=cots, g32=g32, g64=g64, e32=GR.row_error(g32, g64), mel_margin=math.inf, mel_floored=None,
               energy_margin=math.inf, energy_floored=None, empty_filters=0)
    if "num_filters" in kw:
        mel = unfloored_mel(cls, kw, x)
        ref["mel_margin"] = float(np.abs(mel / constants.MEL_FLOOR - 1.0).min())
        ref["mel_floored"] = (mel <= constants.MEL_FLOOR).reshape(3, -1).mean(axis=1)
        ref["empty_filters"] = int(((GR.mel_filters(cls, kw) != 0).sum(axis=0) == 0).sum())
    if energy_flag(cls, kw) and kw["energy_floor"] > 0.0:
        log_e, log_floor = unfloored_log_energy(cls, kw, x), math.log(kw["energy_floor"])
        ref["energy_margin"] = float(np.abs(log_e - log_floor).min())
        ref["energy_floored"] = (log_e < log_floor).mean(axis=1)
    return ref


def why_excluded(ref: dict):
    """None, or what keeps the case from holding a device to its float32 reference."""
    if not np.all(ref["e32"] <= CAP):
        return f"E(g32) {ref['e32'].max():.2g} > {CAP:g}"
    if ref["mel_margin"] < MARGIN:
        return f"a mel energy within {ref['mel_margin']:.2g} of MEL_FLOOR"
    if ref["energy_margin"] < MARGIN:
        return f"a frame log-energy within {ref['energy_margin']:.2g} of log(energy_floor)"
    return None


KEPT = [i for i in range(NUM_CASES) if i not in EXCLUDED]
