"""Test infrastructure: loader of tests/golden/reverb.npz + reverb.json (written by tools/make_golden_reverb.py under the real lhotse) and
the track tables of its cuts over the regenerated corpus of oracle/driver_corpus.py -- all a machine without lhotse needs."""
import json
import os

import numpy as np

from _mix_golden import corpus_files, track_samples  # noqa: F401  (the same corpus, the same rows)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUPS = ("reverb", "speed_reverb", "reverb_cutmix", "options", "k2")


def load_reverb_goldens():
    with open(os.path.join(GOLDEN_DIR, "reverb.json")) as f:
        meta = json.load(f)
    return dict(np.load(os.path.join(GOLDEN_DIR, "reverb.npz"))), meta


def rir_samples(arrays, reverb):
    """The float32 RIR as the reference loads it: int16 / 32768, the first 50 ms (800 taps at 16 kHz) with early_only."""
    pcm = arrays[f"rir/{reverb['rir']}"]
    return np.ascontiguousarray((pcm[:800] if reverb["early_only"] else pcm).astype(np.float32) / np.float32(32768.0))


def tracks_of(entry, paths, arrays):
    """One golden cut as ``FusedMiniBatch.features_of_tracks`` takes it (a reverberated track has 7 elements)."""
    out = []
    for r in entry["tracks"]:
        t = (track_samples(r, paths), r["factor"], r["offset"], r["snr"], r["ref"], r["num_samples"])
        if "reverb" in r:
            t += ((rir_samples(arrays, r["reverb"]), r["reverb"]["normalize"]),)
        out.append(t)
    return out


def exact_audio(arrays, group, i):
    """The float64 truth of the cut (stored as its float32 difference from the reference's load_audio())."""
    return arrays[f"{group}/{i}/audio"].astype(np.float64) + arrays[f"{group}/{i}/exact_minus_audio"].astype(np.float64)
