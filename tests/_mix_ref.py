"""Test infrastructure: the mixing rule of ``MixedCut.load_audio`` / ``AudioMixer`` (lhotse/cut/mixed.py:1312-1409,
lhotse/audio/mixer.py:10-176) restated in numpy over plain track tables -- the contract of ``hipfeat_mix_*`` (include/hipfeat.h):

    E_t = mean(x_t^2);  g_t = 1 without an SNR, without a reference, when E_ref <= 0 or E_t <= 0, or for a first track that is the
    reference itself; else g_t = float32(sqrt(E_ref * 10^(-snr_t / 10) / E_t));
    out[i] = ((0 + g_0 x_0[i - o_0]) + g_1 x_1[i - o_1]) + ...  in track order over the tracks that cover i, float32, product rounded
    before the add; uncovered samples 0; max_t(o_t + n_t) samples, truncated to `max_samples`.

``energy="float32"`` takes the energies the way the reference does (``float(np.average(x ** 2))`` on the float32 samples): with it the
rule is bit-equal to ``load_audio()``; ``"float64"`` is what the device computes.  ``accumulate=np.float64`` gives the float64 mix of
the same float32 tracks (the yardstick of the GPU audio tests).  The product never imports this."""
from math import sqrt

import numpy as np


def track_energy(x: np.ndarray, energy: str = "float64") -> float:
    if energy == "float32":
        return float(np.average(x ** 2))  # audio_energy, mixer.py:175-176
    return float(np.mean(np.asarray(x, dtype=np.float64) ** 2))


def track_gains(tracks, ref: int, energy: str = "float64", rounded: bool = True):
    """tracks: [(samples (1-D float32) or the sample count of a padding track, offset_samples, snr or None)]; ref: index or -1.
    ``rounded=False`` keeps the gains in float64 (the exact mix)."""
    e_ref = None
    gains = []
    for t, (x, _, snr) in enumerate(tracks):
        g = 1.0
        scaled = snr is not None and not (isinstance(snr, float) and np.isnan(snr))
        if scaled and ref >= 0 and not np.isscalar(x) and not (t == 0 and ref == 0):
            if e_ref is None:
                e_ref = track_energy(tracks[ref][0], energy)
            if e_ref > 0:
                e_t = track_energy(x, energy)
                if e_t > 0:
                    g = sqrt(e_ref * (10.0 ** (-snr / 10)) / e_t)
        gains.append(np.float32(g) if rounded else np.float64(g))
    return gains


def mix_tracks(tracks, ref: int = -1, max_samples: int = -1, energy: str = "float64", accumulate=np.float32) -> np.ndarray:
    """``accumulate=np.float64``: float64 energies, gains, products and sums over the same float32 tracks -- no rounding anywhere."""
    exact = accumulate == np.float64
    gains = track_gains(tracks, ref, "float64" if exact else energy, rounded=not exact)
    total = max(int(o) + (int(x) if np.isscalar(x) else len(x)) for x, o, _ in tracks)
    out = np.zeros(total, dtype=accumulate)
    for (x, o, _), g in zip(tracks, gains):
        if np.isscalar(x):
            continue
        scaled = g * np.asarray(x, dtype=np.float32)  # float32 product, rounded (gain * audio, mixer.py:166); float64 when exact
        out[int(o) : int(o) + len(x)] += scaled.astype(accumulate)
    if max_samples is not None and 0 <= max_samples < total:
        out = out[:max_samples]
    return out


def mix_in_arena_cpu(arena, track_first, src_offsets, src_lens, dst_offsets, snrs, ref_tracks, max_samples, tail_start, energy="float64"):
    """CPU stand-in with the interface and the layout of ``lhotse_amd.augmentation.mix_in_arena`` (``arena``: a CPU torch tensor)."""
    assert len(track_first) > 1, "hipfeat_mix_plan refuses an empty batch (HIPFEAT_ERR_INVALID)"
    a = arena.numpy()
    tail = (int(tail_start) + 3) & ~3
    offs, lens = [], []
    for c in range(len(track_first) - 1):
        tracks = []
        for t in range(int(track_first[c]), int(track_first[c + 1])):
            so, n = int(src_offsets[t]), int(src_lens[t])
            assert so < 0 or so + n <= tail_start
            tracks.append((n if so < 0 else a[so : so + n].copy(), int(dst_offsets[t]), None if snrs is None else snrs[t]))
        y = mix_tracks(tracks, -1 if ref_tracks is None else int(ref_tracks[c]), -1 if max_samples is None else int(max_samples[c]), energy)
        assert tail + len(y) <= len(a), "arena too small"
        a[tail : tail + len(y)] = y
        offs.append(tail), lens.append(len(y))
        tail = (tail + len(y) + 3) & ~3
    return np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)
