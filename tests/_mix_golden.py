"""Test infrastructure: loader of tests/golden/mix.npz + mix.json (written by tools/make_golden_mix.py under the real lhotse) and the
track tables of its cuts over the regenerated corpus of oracle/driver_corpus.py -- all a machine without lhotse needs."""
import json
import os

import numpy as np

from oracle.driver_corpus import read_wav, write_corpus

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_mix_goldens():
    with open(os.path.join(GOLDEN_DIR, "mix.json")) as f:
        meta = json.load(f)
    return dict(np.load(os.path.join(GOLDEN_DIR, "mix.npz"))), meta


def corpus_files(directory, meta):
    """Regenerate the WAV corpus and check it against what the reference saw (CRC) -> {file id: path}."""
    files = write_corpus(directory)
    for f, g in zip(files, meta["files"]):
        assert (f["id"], f["num_samples"], f["crc"]) == (g["id"], g["num_samples"], g["crc"]), "the regenerated corpus drifted from the one the reference saw"
    return {f["id"]: f["path"] for f in files}


def track_samples(row, paths):
    """The samples a track read in front of its pending Speed (1-D float32), or its sample count for a padding track."""
    if row["file"] is None:
        return int(row["count"])
    if row["file"] == "zero":
        return np.zeros(row["count"], dtype=np.float32)
    return np.ascontiguousarray(read_wav(paths[row["file"]], row["first"], row["count"])[0])


def tracks_of(entry, paths):
    """One golden cut as ``FusedMiniBatch.features_of_tracks`` takes it."""
    return [(track_samples(r, paths), r["factor"], r["offset"], r["snr"], r["ref"], r["num_samples"]) for r in entry["tracks"]]


def ref_tracks_of(entry, paths):
    """One golden cut (unperturbed tracks only) as tests/_mix_ref.mix_tracks takes it -> (tracks, reference index)."""
    assert all(r["factor"] == 1.0 for r in entry["tracks"])
    tracks = [(track_samples(r, paths), r["offset"], r["snr"]) for r in entry["tracks"]]
    return tracks, next((k for k, r in enumerate(entry["tracks"]) if r["ref"]), -1)


def exact_mix(arrays, group, i):
    """The float64 mix of the cut's float32 tracks (stored as its float32 difference from the reference's load_audio())."""
    return arrays[f"{group}/{i}/audio"].astype(np.float64) + arrays[f"{group}/{i}/exact_minus_audio"].astype(np.float64)
