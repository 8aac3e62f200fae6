"""Test infrastructure: loader of tests/golden/level.npz + level.json (written by tools/make_golden_level.py under the real lhotse) and
the track tables of its cuts over the regenerated corpus of oracle/driver_corpus.py -- all a machine without lhotse needs."""
import json
import os

import numpy as np

from _mix_golden import corpus_files, track_samples  # noqa: F401  (the same corpus, the same rows)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUPS = ("volume", "clip_hard", "clip_soft", "clip_oversampled", "speed_volume_clip_reverb", "volume_cutmix", "k2")
EXACT_GROUPS = ("volume", "clip_hard")  # chains of nothing but Volume or a hard Clipping: the audio is the reference's, bit for bit


def load_level_goldens():
    with open(os.path.join(GOLDEN_DIR, "level.json")) as f:
        meta = json.load(f)
    return dict(np.load(os.path.join(GOLDEN_DIR, "level.npz"))), meta


def steps_of(block):
    """A block as JSON keeps it -> the steps ``FusedMiniBatch.features_of_tracks`` takes (tuples)."""
    if block is None:
        return None
    return [("level", [tuple(op) for op in st[1]]) if st[0] == "level" else (st[0], int(st[1])) for st in block]


def rir_samples(arrays, reverb):
    return np.ascontiguousarray(arrays[f"rir/{reverb['rir']}"].astype(np.float32) / np.float32(32768.0))


def tracks_of(entry, paths, arrays, rirs=None):
    """One golden cut as ``FusedMiniBatch.features_of_tracks`` takes it: 9-element tracks where a row has level blocks, the 6- or
    7-element tracks of before where it has none.  ``rirs``: a dict shared over the mini-batch so that a RIR is one array object."""
    rirs = {} if rirs is None else rirs
    out = []
    for r in entry["tracks"]:
        t = (track_samples(r, paths), r["factor"], r["offset"], r["snr"], r["ref"], r["num_samples"])
        rv = None
        if r.get("reverb"):
            rv = (rirs.setdefault(r["reverb"]["rir"], rir_samples(arrays, r["reverb"])), r["reverb"]["normalize"])
        if r.get("level"):
            t += (rv, None, (steps_of(r["level"][0]), steps_of(r["level"][1])))
        elif rv is not None:
            t += (rv,)
        out.append(t)
    return out


def exact_audio(arrays, group, i):
    """The float64 truth of the cut (stored as its float32 difference from the reference's load_audio())."""
    return arrays[f"{group}/{i}/audio"].astype(np.float64) + arrays[f"{group}/{i}/exact_minus_audio"].astype(np.float64)
