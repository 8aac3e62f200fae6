"""Test infrastructure: loader of tests/golden/lowpass.npz + lowpass.json (written by tools/make_golden_lowpass.py under the real lhotse)
and the track tables of its cuts over the regenerated corpus of oracle/driver_corpus.py -- all a machine without lhotse needs."""
import json
import os

import numpy as np

from _level_golden import rir_samples
from _mix_golden import corpus_files  # noqa: F401  (the same corpus, the same rows)
from _mix_golden import track_samples as _corpus_samples

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GROUPS = ("band", "speed_band", "band_volume_clip", "band_reverb", "lead", "band_cutmix", "k2")
AUDIO_GROUPS = ("band", "speed_band", "band_volume_clip", "band_reverb", "lead")  # single-track cuts: the reference's load_audio() is stored


def load_lowpass_goldens():
    with open(os.path.join(GOLDEN_DIR, "lowpass.json")) as f:
        meta = json.load(f)
    return dict(np.load(os.path.join(GOLDEN_DIR, "lowpass.npz"))), meta


def steps_of(block):
    """A block as JSON keeps it -> the steps ``FusedMiniBatch.features_of_tracks`` takes (tuples): ``("level", [ops])``, ``("up", k)``,
    ``("down", k)``, ``("rate", src, dst)``."""
    if block is None:
        return None
    return [("level", [tuple(op) for op in st[1]]) if st[0] == "level" else (st[0],) + tuple(int(v) for v in st[1:]) for st in block]


def track_samples(row, paths, arrays=None):
    """The samples a track read in front of its pending transforms; a file outside the corpus (the group ``lead``: a recording at
    11130 Hz) is stored in the archive as ``src/<file>`` (PCM16)."""
    if row["file"] is None or row["file"] in paths or row["file"] == "zero":
        return _corpus_samples(row, paths)
    pcm = arrays[f"src/{row['file']}"][row["first"] : row["first"] + row["count"]]
    return np.ascontiguousarray(pcm.astype(np.float32) / np.float32(32768.0))


def tracks_of(entry, paths, arrays, rirs=None):
    """One golden cut as ``FusedMiniBatch.features_of_tracks`` takes it: 9-element tracks where a row has level blocks, 8-element tracks
    where it has a source rate of its own (a leading ``Resample``), the 6- or 7-element tracks of before where it has neither.
    ``rirs``: a dict shared over the mini-batch so that a RIR is one array object."""
    rirs = {} if rirs is None else rirs
    out = []
    for r in entry["tracks"]:
        t = (track_samples(r, paths, arrays), r["factor"], r["offset"], r["snr"], r["ref"], r["num_samples"])
        rv = None
        if r.get("reverb"):
            rv = (rirs.setdefault(r["reverb"]["rir"], rir_samples(arrays, r["reverb"])), r["reverb"]["normalize"])
        if r.get("level"):
            t += (rv, r.get("source_rate"), (steps_of(r["level"][0]), steps_of(r["level"][1])))
        elif r.get("source_rate"):
            t += (rv, r["source_rate"])
        elif rv is not None:
            t += (rv,)
        out.append(t)
    return out


def exact_audio(arrays, group, i):
    """The float64 truth of the cut (stored as its float32 difference from the reference's load_audio())."""
    return arrays[f"{group}/{i}/audio"].astype(np.float64) + arrays[f"{group}/{i}/exact_minus_audio"].astype(np.float64)
