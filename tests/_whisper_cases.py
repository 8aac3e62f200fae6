"""Inputs for the tests of the Whisper per-cut normalisation (tests/test_gpu_whisper_clamp.py), each built for ONE purpose that
tests/test_whisper_cases.py proves on the CPU from the float64 oracle (oracle/whisper_ref.py) -- a case that does not do what it
says would let the code path it is meant for go unvisited without anybody noticing.

All cases are seeded uniform noise of amplitude `amp` with sections scaled down and, for the dropped column, a burst behind the last
kept frame.  White noise spans about 4.5 decades between its loudest and its quietest mel bin, so a section scaled by 5e-5 (8.6
decades of power) lies WHOLLY under the clamp at max - 8; at amplitude 1000 (maximum near 10^6.5) it still stays more than a decade
above the 1e-10 mel floor, which would otherwise hide what the clamp does (the narrow low filters of a 128-filter bank weigh single
bins by very little: their quietest values lie 7 decades under the maximum).

Frames-per-workgroup (`fpw`) classifications name, per row block of whisper3_kernel, whether the block holds nothing under the
clamp ("none": not listed by section 6 of the kernel), something ("part") or only such values ("all")."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

from oracle import whisper_ref as W

HOP = W.HOP
QUIET = 5e-5    # 8.6 decades of power
MARGIN = 0.05   # decades (of log10 power) a value keeps from the clamp level before it counts as under / over it


@dataclass(frozen=True)
class Case:
    name: str
    purpose: str
    frames: int            # valid frames = S // 160
    extra: int             # S % 160 (>= 80: the matrix ends with the zero padding row)
    amp: float
    seed: int
    quiet: Tuple[Tuple[int, int, float], ...] = ()   # (first sample, end sample, factor); end < 0: to the end of the cut
    burst: float = 0.0     # amplitude of a burst over the samples >= frames * 160 + 40 (seen by the dropped STFT column only)
    acts: bool = True      # the clamp changes values
    blocks: Tuple[Tuple[int, str], ...] = ()  # (fpw, classes of the row blocks as a string of n / p / a)

    @property
    def num_samples(self) -> int:
        return self.frames * HOP + self.extra

    @property
    def rows(self) -> int:
        return W.num_rows(self.num_samples)


def _sec(f0: int, f1: int, factor: float = QUIET):
    """the prototype's section: samples f0 * 160 + 37 .. f1 * 160 + 91 (no frame boundary)"""
    return (f0 * HOP + 37, f1 * HOP + 91, factor)


CASES: Dict[str, Case] = {c.name: c for c in [
    # ---- clamp cases: 1100 frames = 5 row blocks of 256, 3 of 384, 18 of 64 (the last one 12 frames) ----
    Case("mid", "quiet middle: whole row blocks under the clamp between two partial ones, untouched blocks on both sides",
         1100, 100, 1000.0, 101, (_sec(300, 800),), blocks=((256, "npapn"), (384, "pap"), (64, "nnnnpaaaaaaapnnnnn"))),
    Case("tail", "quiet to the end: the LAST (partial) row block is listed, the maximum sits in the first",
         1100, 100, 1000.0, 102, ((700 * HOP + 37, -1, QUIET),), blocks=((256, "nnpaa"), (384, "npa"), (64, "nnnnnnnnnnpaaaaaaa"))),
    Case("head", "quiet start: the FIRST row block is listed, the maximum sits in a later workgroup",
         1100, 100, 1000.0, 103, ((0, 420 * HOP + 91, QUIET),), blocks=((256, "apnnn"), (384, "apn"), (64, "aaaaaapnnnnnnnnnnn"))),
    Case("spots", "two short quiet sections inside row blocks: every listed block is a partial one",
         1100, 100, 1000.0, 104, (_sec(100, 140), _sec(900, 1000)), blocks=((256, "pnnpn"), (384, "pnp"), (64, "nppnnnnnnnnnnnppnn"))),
    # ---- odd frame counts for the scalar tails (frames % 4 != 0; 1101 x 23, 1101 x 81 and 1101 x 127 are no multiples of 4) ----
    Case("tail_odd", "as `tail` with 1101 frames: with an odd filter count the last row block ends in a scalar tail",
         1101, 100, 1000.0, 105, ((700 * HOP + 37, -1, QUIET),), blocks=((64, "nnnnnnnnnnpaaaaaaa"),)),
    Case("long_odd", "4301 frames: with 23 filters more than 24576 float4 (the two-read route of whisper_norm_kernel) and a scalar tail",
         4301, 90, 1000.0, 106, (_sec(1000, 3000),)),
    # ---- semantics ----
    Case("dropped", "a burst that only the dropped last STFT column sees, over a section 3 decades down: counting the dropped frame "
         "for the maximum would clamp that section; the correct maximum clamps nothing",
         300, 150, 300.0, 107, ((100 * HOP, 260 * HOP, 10 ** -1.5),), burst=1e6, acts=False),
    Case("loud", "PCM-scale amplitude: the clamp level c = (max - 4) / 4 is positive, so a sweep over the zero padding row or over "
         "collated fill rows would show", 200, 120, 3e4, 108, (_sec(60, 130),), blocks=((64, "papn"),)),
    Case("pad_only", "128 frames + padding row: at 64 frames per workgroup the third workgroup holds only the padding row",
         128, 130, 1000.0, 109, (_sec(20, 50),), blocks=((64, "pn"),)),
]}


def boundary_lengths(k: int):
    """Cut lengths around S = 160 * 4k + 680, the first at which the span of the wave that starts at frame 4k (samples
    640 k - 200 .. 640 k + 679) lies inside the cut and is staged by LDS-DMA instead of the reflecting loads."""
    s = HOP * 4 * k + 680
    return (s - 1, s, s + 1)


@functools.lru_cache(maxsize=None)
def signal(name: str) -> np.ndarray:
    c = CASES[name]
    rs = np.random.RandomState(c.seed)
    x = (rs.rand(c.num_samples) - 0.5) * c.amp
    for a, b, factor in c.quiet:
        x[a:(c.num_samples if b < 0 else b)] *= factor
    if c.burst:
        x[c.frames * HOP + 40:] = (rs.rand(c.num_samples - c.frames * HOP - 40) - 0.5) * c.burst
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def noise(num_samples: int, amp: float, seed: int) -> np.ndarray:
    x = ((np.random.RandomState(seed).rand(num_samples) - 0.5) * amp).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def filters(n_mels: int) -> np.ndarray:
    """The oracle's filterbank; tests/test_whisper_cases.py: bit for bit constants.make_slaney_mel(n_mels, 400, 16000).T"""
    f = W.slaney_mel_filters(W.SAMPLING_RATE, W.N_FFT, n_mels)
    f.setflags(write=False)
    return f


def raw_log_mel(x: np.ndarray, n_mels: int, keep_dropped: bool = False) -> np.ndarray:
    """float64 log10(max(mel, 1e-10)) of the S // 160 kept frames BEFORE the clamp (whisper_ref.log_mel_spectrogram up to its line
    `log_spec = np.log10(...)`); keep_dropped: with the last STFT column the reference drops, as row S // 160."""
    x = np.asarray(x, dtype=np.float64)
    xp = np.pad(x, (W.N_FFT // 2, W.N_FFT // 2), mode="reflect")
    nfr = 1 + (len(xp) - W.N_FFT) // HOP
    idx = (np.arange(nfr) * HOP)[:, None] + np.arange(W.N_FFT)[None, :]
    spec = np.fft.rfft(xp[idx] * W.hann_periodic(W.N_FFT, np.float64)[None, :], axis=1)
    mag = np.abs(spec if keep_dropped else spec[:-1]) ** 2
    return np.log10(np.maximum(mag @ filters(n_mels).astype(np.float64).T, 1e-10))


def finish(raw: np.ndarray, rows: int, cut_max: float = None) -> np.ndarray:
    """clamp at cut_max - 8 (default: the maximum of `raw`), (x + 4) / 4, zero rows up to `rows`"""
    top = raw.max() if cut_max is None else cut_max
    y = (np.maximum(raw, top - 8.0) + 4.0) / 4.0
    return np.concatenate([y, np.zeros((rows - len(y), y.shape[1]))]) if rows > len(y) else y


def classify(raw: np.ndarray, fpw: int) -> str:
    """per row block of fpw frames: n(one) / p(art) / a(ll) of its values under max - 8; values within MARGIN of the level are an error"""
    level = raw.max() - 8.0
    assert not np.any(np.abs(raw - level) < MARGIN), "a value sits on the clamp level: the case does not classify"
    out = ""
    for f0 in range(0, len(raw), fpw):
        under = raw[f0:f0 + fpw] < level
        out += "a" if under.all() else ("p" if under.any() else "n")
    return out


@functools.lru_cache(maxsize=None)
def _reference(key, n_mels: int):
    x = signal(key) if isinstance(key, str) else noise(*key)
    truth = W.log_mel_spectrogram(x, filters(n_mels), dtype=np.float64)
    ref32 = W.log_mel_spectrogram(x, filters(n_mels), dtype=np.float32)
    truth.setflags(write=False)
    ref32.setflags(write=False)
    return truth, ref32


def reference(key, n_mels: int):
    """(float64 oracle, float32 oracle) of a case (by name) or of noise(num_samples, amp, seed) (by that tuple); computed once"""
    return _reference(key, n_mels)
