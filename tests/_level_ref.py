"""The level rule (Volume, Clipping) in numpy, written from the rule of include/hipfeat.h -- test infrastructure, the product never imports
this.

A program is a list of ``("volume", factor)`` / ``("clip", hard, gain_db, normalize)``; an item is ONE array (its peak is taken over all of
it).  ``exact`` is the rule in float64 throughout (the truth the soft clip is measured against); ``model32`` is the device's arithmetic:
float32, one rounding per step, the steps in the device's order, IEEE divisions, the soft clip as the float64 tanh rounded once, and the
CLIP's peak pushed through the SCALEs in front of it instead of being taken again."""
import numpy as np

SILENCE_PEAK = np.float32(float.fromhex("0x1.09e69ep-16"))  # restated, not imported: tests compare it with lhotse_amd.constants
EPS24 = 2.0 ** -24


def gain_of(gain_db):
    """(g, use_gain) as the host computes them (clipping.py:44-45)."""
    return np.float32(10 ** (gain_db / 20.0)), abs(gain_db) >= 0.1


def propagated_peak(x, factors):
    """max |x| pushed through the SCALEs with the samples' own float32 products: p = fl(fl(peak * |f1|) * |f2|)."""
    p = np.float32(np.max(np.abs(np.asarray(x, np.float32))))
    for f in factors:
        p = np.float32(p * np.abs(np.float32(f)))
    return p


def model32(x, program):
    x = np.asarray(x, np.float32)
    v = x.copy()
    factors = []
    for op in program:
        if op[0] == "volume":
            v = v * np.float32(op[1])
            factors.append(op[1])
            continue
        _, hard, gain_db, normalize = op
        p = propagated_peak(x, factors)
        if p == 0 or p < SILENCE_PEAK:
            continue
        g, use_gain = gain_of(gain_db)
        if normalize:
            v = v / p
        if use_gain:
            v = v * g
        v = np.minimum(np.maximum(v, np.float32(-1)), np.float32(1)) if hard else np.tanh(v.astype(np.float64)).astype(np.float32)
        if use_gain:
            v = v / g
        if normalize:
            v = v * p
        assert v.dtype == np.float32
    return v


def exact(x, program):
    """float64 throughout; the float32 parameters (factor, g) and the silence decision are the rule's, so that only rounding differs."""
    x32 = np.asarray(x, np.float32)
    v = x32.astype(np.float64)
    factors = []
    for op in program:
        if op[0] == "volume":
            v = v * np.float64(np.float32(op[1]))
            factors.append(op[1])
            continue
        _, hard, gain_db, normalize = op
        if propagated_peak(x32, factors) == 0 or propagated_peak(x32, factors) < SILENCE_PEAK:
            continue
        p = float(np.max(np.abs(v)))
        g, use_gain = gain_of(gain_db)
        g = float(g)
        if normalize:
            v = v / p
        if use_gain:
            v = v * g
        v = np.clip(v, -1.0, 1.0) if hard else np.tanh(v)
        if use_gain:
            v = v / g
        if normalize:
            v = v * p
    return v


def exact64(v, program):
    """``exact`` for samples that are float64 already (behind a float64 resampler or convolution): the peak is the float64 one."""
    v = np.asarray(v, np.float64)
    for op in program:
        if op[0] == "volume":
            v = v * np.float64(np.float32(op[1]))
            continue
        _, hard, gain_db, normalize = op
        p = float(np.max(np.abs(v)))
        if p == 0 or np.float32(p) < SILENCE_PEAK:
            continue
        g, use_gain = gain_of(gain_db)
        g = float(g)
        if normalize:
            v = v / p
        if use_gain:
            v = v * g
        v = np.clip(v, -1.0, 1.0) if hard else np.tanh(v)
        if use_gain:
            v = v / g
        if normalize:
            v = v * p
    return v


def distances(y, truth):
    """(max abs error, rel-L2) of y from the float64 truth."""
    d = np.asarray(y, np.float64) - truth
    den = float(np.sqrt(np.sum(truth ** 2)))
    return float(np.max(np.abs(d), initial=0.0)), (float(np.sqrt(np.sum(d ** 2))) / den if den > 0 else float(np.sqrt(np.sum(d ** 2))))


def soft_bars(ref_max, ref_rel, truth):
    """The soft-clip bars: max abs <= 2 x the reference's own + 2^-24 x peak, rel-L2 <= 2 x the reference's own."""
    return 2.0 * ref_max + EPS24 * float(np.max(np.abs(truth), initial=0.0)), 2.0 * ref_rel


def signal(seed, n, amplitude=0.5):
    """A deterministic test signal: uniform noise in (-amplitude, amplitude), float32.  The golden generator and the GPU tests draw the same."""
    return ((np.random.RandomState(seed).rand(n) * 2.0 - 1.0) * amplitude).astype(np.float32)


# the soft-clip cases whose reference figures tools/make_golden_level.py records in tests/golden/level.json ("soft_cases"):
# (name, seed, samples, amplitude, program).  Lengths on both sides of the 4-sample groups and the 4096-sample tiles.
SOFT_CASES = [(f"soft_n{n}_g{gi}_{'n' if norm else 'r'}", 1000 + 7 * k + gi, n, amp, [("clip", False, gain_db, norm)])
              for k, n in enumerate((1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4099, 70001))
              for gi, (gain_db, norm, amp) in enumerate(((0.0, True, 0.5), (0.05, False, 1.5), (-6.0, True, 0.25), (20.0, False, 0.9)))]
SOFT_CASES += [("soft_scale_clip", 2001, 4099, 0.5, [("volume", 1.7), ("clip", False, 20.0, True)]),
               ("soft_clip_scale", 2002, 4099, 0.5, [("clip", False, -6.0, True), ("volume", 0.6)]),
               ("soft_four_ops", 2003, 4099, 0.5, [("volume", -1.3), ("volume", 0.9), ("clip", False, 20.0, True), ("volume", 1.1)])]
