"""Test infrastructure: loader of tests/golden/resample_chain.npz + .json (written by tools/make_golden_resample_chain.py under the real
lhotse), the regenerated source files at their own sampling rates, the track tables as ``FusedMiniBatch.features_of_tracks`` takes them
(8-element tracks with a ``source_rate``), and the two numpy statements of the chain ``[Resample]? [Speed]?`` over such a table:

  * ``model_track``: float32, the device's summation order per stage -- accumulator from 0, taps ascending, one fma per tap (product
    exact in float64, one rounding to float32 per tap), the second stage over the first stage's float32 output;
  * ``exact_track``: ``oracle.resample_ref.resample(..., dtype=np.float64)`` per stage, nothing rounded in between.

The product never imports this."""
import json
import os
import zlib

import numpy as np

from oracle import resample_ref as R
from oracle.driver_corpus import pcm16, read_wav, write_wav

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SR = 16000
# (id, signal family, samples, seed, sampling rate): <= 0.5 s cuts come out of these
SOURCES = [
    ("s44a", "speechlike", 22050, 11, 44100),
    ("s44b", "voiced", 17640, 12, 44100),
    ("s22a", "speechlike", 9922, 13, 22050),
    ("s22b", "voiced", 11025, 14, 22050),
    ("n8a", "uniform", 6000, 15, 8000),
    ("n8b", "uniform", 4400, 16, 8000),
    ("s16a", "speechlike", 7000, 17, 16000),
]


def write_sources(directory, sources=SOURCES):
    """Write the files; -> [{"id", "kind", "n", "seed", "rate", "crc", "path"}] in order."""
    os.makedirs(directory, exist_ok=True)
    out = []
    for fid, kind, n, seed, rate in sources:
        pcm = pcm16(kind, n, seed, rate)
        path = os.path.join(str(directory), f"{fid}.wav")
        write_wav(path, pcm, rate)
        out.append({"id": fid, "kind": kind, "n": int(n), "seed": int(seed), "rate": int(rate), "crc": zlib.crc32(pcm.tobytes()) & 0xFFFFFFFF, "path": path})
    return out


def load_goldens():
    with open(os.path.join(GOLDEN_DIR, "resample_chain.json")) as f:
        meta = json.load(f)
    return dict(np.load(os.path.join(GOLDEN_DIR, "resample_chain.npz"))), meta


def source_files(directory, meta):
    """Regenerate the source files from the json's (kind, n, seed, rate) and check them against what the reference saw (CRC)."""
    files = write_sources(directory, [(g["id"], g["kind"], g["n"], g["seed"], g["rate"]) for g in meta["files"]])
    for f, g in zip(files, meta["files"]):
        assert f["crc"] == g["crc"], "the regenerated sources drifted from the ones the reference saw"
    return {f["id"]: f["path"] for f in files}


def rir_of(arrays, row):
    """The float32 RIR of a reverberated row as the reference loads it (int16 / 32768)."""
    return np.ascontiguousarray(arrays[f"rir/{row['reverb']['rir']}"].astype(np.float32) / np.float32(32768.0))


def track_samples(row, paths):
    if row["file"] is None:
        return int(row["count"])
    return np.ascontiguousarray(read_wav(paths[row["file"]], row["first"], row["count"])[0])


def tracks_of(entry, paths, arrays=None, rirs=None):
    """One golden cut as ``FusedMiniBatch.features_of_tracks`` takes it: (samples, factor, offset, snr, is_reference, num_samples,
    reverb or None, source_rate).  ``rirs``: a dict shared over the mini-batch so that a RIR is one array object."""
    out = []
    for r in entry["tracks"]:
        rv = None
        if r.get("reverb"):
            rirs = {} if rirs is None else rirs
            h = rirs.setdefault(r["reverb"]["rir"], rir_of(arrays, r))
            rv = (h, r["reverb"]["normalize"])
        out.append((track_samples(r, paths), r["factor"], r["offset"], r["snr"], r["ref"], r["num_samples"], rv, r["source_rate"]))
    return out


def fma_resample(x, src, dst):
    """float32 sinc resampling in the device's order: per output the ascending-tap chain acc = fma(x, k, acc) from 0."""
    from lhotse_amd import constants

    if int(src) == int(dst):
        return np.asarray(x, dtype=np.float32)
    k, width, orig, new = constants.sinc_resample_kernel(src, dst)
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    xp = np.concatenate([np.zeros(width, np.float32), x, np.zeros(width + orig, np.float32)]).astype(np.float64)
    kw = 2 * width + orig
    nj = (len(xp) - kw) // orig + 1
    base = np.arange(nj) * orig
    k64 = k.astype(np.float64)
    acc = np.zeros((nj, new), dtype=np.float32)
    for i in range(kw):
        acc = (acc.astype(np.float64) + xp[base + i][:, None] * k64[:, i][None, :]).astype(np.float32)
    return acc.reshape(-1)[: R.resampled_length(len(x), orig, new)]


def stages(source_rate, factor, sr=SR):
    """The (source, target) rates of the chain's resampling stages."""
    out = []
    if source_rate is not None and int(source_rate) != int(sr):
        out.append((int(source_rate), int(sr)))
    if factor != 1.0:
        out.append((round(sr * factor), int(sr)))
    return out


def model_track(x, source_rate, factor, sr=SR):
    y = np.asarray(x, dtype=np.float32)
    for a, b in stages(source_rate, factor, sr):
        y = fma_resample(y, a, b)
    return y


def exact_track(x, source_rate, factor, sr=SR):
    y = np.asarray(x, dtype=np.float64)
    for a, b in stages(source_rate, factor, sr):
        y = R.resample(y, a, b, dtype=np.float64)
    return y


def exact_mix(tracks, ref, want):
    """float64 mix of float64 tracks [(samples or count, offset, snr)] by the rule of tests/_mix_ref.py, nothing rounded."""
    from _mix_ref import track_gains

    gains = track_gains(tracks, ref, "float64", rounded=False)
    total = max(int(o) + (int(x) if np.isscalar(x) else len(x)) for x, o, _ in tracks)
    out = np.zeros(total, dtype=np.float64)
    for (x, o, _), g in zip(tracks, gains):
        if not np.isscalar(x):
            out[int(o) : int(o) + len(x)] += g * np.asarray(x, dtype=np.float64)
    return out[:want]


def chain_tracks(entry, paths, fn):
    """The tracks of a golden cut behind their chains (``fn`` = model_track or exact_track), truncated to their sample counts, as
    tests/_mix_ref.mix_tracks takes them -> (tracks, reference index)."""
    tracks = []
    for r in entry["tracks"]:
        x = track_samples(r, paths)
        if not np.isscalar(x):
            x = fn(x, r["source_rate"], r["factor"])[: r["num_samples"]]
        tracks.append((x, r["offset"], r["snr"]))
    return tracks, next((k for k, r in enumerate(entry["tracks"]) if r["ref"]), -1)


def exact_audio(arrays, group, i):
    """The float64 chain of the cut (stored as its float32 difference from the reference's load_audio())."""
    return arrays[f"{group}/{i}/audio"].astype(np.float64) + arrays[f"{group}/{i}/exact_minus_audio"].astype(np.float64)
