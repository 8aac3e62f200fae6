#!/usr/bin/env python3
"""The feature-mix launches (lhotse_amd.augmentation.featmix_in_arena behind lhotse_amd.FusedFeatureBatch: the stored tracks of a
mini-batch -> the padded (B, Tmax, F) float32 batch) against the per-cut host path they replace, in one process.

Workload: a ragged 600 s mini-batch of 80-dim log-mel features (cuts of about 12.7 s, 100 frames per second) in which every second cut
carries one ``CutMix`` noise track (SNR 10 ... 20 dB, a random offset, padded to the cut), the others are right-padded copies.

Legs, the median of --steps timed runs after --warmup untimed ones:

  * float32 / binary16 "launches": the two launches over a device-resident arena, by HIP events around the call (the staged tables
    included);
  * float32 / binary16 "end_to_end": FusedFeatureBatch.features_of from host matrices (fill of the pinned staging buffer, ONE upload, the
    launches), by the host clock around a device synchronise, since part of it is host time;
  * "host_per_cut": what the parent class does for the same cuts, restated in numpy because the reference is Python and is not on the GPU
    machine: per cut the ``FeatureMixer`` steps of lhotse/features/mixer.py (np.vstack padding of every track, ``Fbank.mix`` = log(maximum(
    1e-10, exp(a) + gain * exp(b))) in float32, ``compute_energy`` = sum(exp(x))), the fill of a (B, Tmax, F) tensor and its upload.

Every leg's result is compared with the float64 truth (tests/_featmix_ref.py) before anything is timed.  Prints one JSON line and writes
it to --out (default profiles/featmix_bench.json).

    python tools/bench_featmix.py [--steps 30] [--warmup 5] [--out profiles/featmix_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = 80
LOG_EPSILON = float(np.log(1e-10))


def workload(rng, seconds=600.0):
    """-> [(speech (n, F) float32, noise (m, F) float32 or None, offset, snr)], binary16-representable values."""
    cuts, total = [], 0.0
    while True:
        dur = float(np.clip(rng.normal(12.7, 3.6), 1.4, 24.5))
        if total + dur > seconds:
            break
        total += dur
        n = int(dur * 100)
        speech = rng.uniform(-15.0, 5.0, (n, F)).astype(np.float16).astype(np.float32)
        if len(cuts) % 2:
            off = int(rng.randint(0, n // 2))
            noise = rng.uniform(-15.0, 0.0, (n - off, F)).astype(np.float16).astype(np.float32)
            cuts.append((speech, noise, off, float(rng.uniform(10, 20))))
        else:
            cuts.append((speech, None, 0, None))
    return cuts


def tables(cuts, f16, tmax):
    from lhotse_amd.augmentation import FEATMIX_COPY, FEATMIX_FOLD

    dt = np.float16 if f16 else np.float32
    out = []
    for speech, noise, off, snr in cuts:
        n = len(speech)
        if noise is None:
            out.append(dict(form=FEATMIX_COPY, num_frames=tmax, pad_value=LOG_EPSILON, tracks=[dict(frames=n, array=speech.astype(dt))]))
        else:  # cuts.pad appends a PaddingCut behind the mix
            tracks = [dict(frames=n, array=speech.astype(dt)), dict(frames=len(noise), first=off, snr=snr, array=noise.astype(dt))]
            if tmax > n:
                tracks.append(dict(frames=tmax - n, first=n, value=LOG_EPSILON))
            out.append(dict(form=FEATMIX_FOLD, num_frames=tmax, ref_track=0, tracks=tracks))
    return out


def host_per_cut(cuts, tmax, dev):
    """The parent's path, restated: FeatureMixer per mixed cut, float64 ones * pad + copy per padded cut, fill, upload."""
    batch = torch.empty(len(cuts), tmax, F, dtype=torch.float32)
    for b, (speech, noise, off, snr) in enumerate(cuts):
        n = len(speech)
        if noise is None:
            feats = np.ones((tmax, F)) * LOG_EPSILON  # (mixed.py:1233)
            feats[:n] = speech
        else:
            tracks, gains = [speech], []
            ref_energy = float(np.sum(np.exp(speech)))
            for x, o, s in ((noise, off, snr), (np.ones((tmax - n, F), dtype=np.float32) * np.float32(LOG_EPSILON), n, None)):
                if not len(x):
                    continue
                cur, inc = tracks[0].shape[0], len(x) + o
                mix_n = max(cur, inc)
                if cur < mix_n:
                    tracks = [np.vstack([t, np.full((mix_n - cur, F), -1000.0, dtype=np.float32)]) for t in tracks]
                add = np.vstack([np.full((o, F), -1000.0, dtype=np.float32), x]) if o > 0 else x
                if inc < mix_n:
                    add = np.vstack([add, np.full((mix_n - inc, F), -1000.0, dtype=np.float32)])
                gain = 1.0
                if s is not None and ref_energy > 0.0:
                    e = float(np.sum(np.exp(x)))
                    if e > 0.0:
                        gain = ref_energy * (10.0 ** (-s / 10)) / e
                tracks.append(add), gains.append(gain)
            feats = tracks[0]
            for t, g in zip(tracks[1:], gains):
                feats = np.log(np.maximum(1e-10, np.exp(feats) + g * np.exp(t)))
        batch[b] = torch.from_numpy(feats)
    return batch.to(dev)


def timed(fn, steps, warmup, events):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(steps + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]) if events else (time.perf_counter() - t0) * 1e3)
    return {"ms": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="timed runs per leg (at least 20; the host leg runs 5)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "featmix_bench.json"))
    args = ap.parse_args()
    steps = max(args.steps, 20)
    if not torch.cuda.is_available():
        raise SystemExit("bench_featmix.py measures on the GPU: no HIP device is visible")

    import _featmix_ref as R

    import lhotse_amd.input_strategies as IS
    from lhotse_amd import FusedFeatureBatch
    from lhotse_amd import augmentation as A

    dev = torch.device("cuda", 0)
    cuts = workload(np.random.RandomState(0))
    tmax = max(len(c[0]) for c in cuts)
    res = {"tool": "tools/bench_featmix.py", "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": args.warmup, "timing": "median (min, max) in ms",
           "cuts": len(cuts), "mixed_cuts": sum(c[1] is not None for c in cuts), "Tmax": tmax, "F": F, "out_MB": round(len(cuts) * tmax * F * 4 / 1e6, 2), "legs": {}}
    batch = FusedFeatureBatch(dev)
    seen = {}
    real = IS._featmix_in_arena

    def spy(arena, table, nf, rows, layout=None):
        seen["arena"], seen["table"] = arena, table
        return real(arena, table, nf, rows, layout)

    IS._featmix_in_arena = spy
    outs = {}
    for key, f16 in (("float32", False), ("binary16", True)):
        tab = tables(cuts, f16, tmax)
        feats, lens = batch.features_of(tab, F, tmax)
        torch.cuda.synchronize()
        arena, table = seen["arena"], seen["table"]
        outs[key] = feats
        truth = R.batch(arena.cpu().numpy(), table, F, tmax)
        err = float(np.abs(feats.cpu().numpy().astype(np.float64) - truth).max())
        assert err < 1e-5, (key, err)  # faster and different is not faster
        out = torch.empty_like(feats)
        legs = res["legs"][key] = {"arena_MB": round(arena.numel() / 1e6, 2), "max_abs_from_float64": err}
        legs["launches"] = timed(lambda: A.featmix_in_arena(arena, table, F, tmax, out=out), steps, args.warmup, True)
        legs["end_to_end"] = timed(lambda: batch.features_of(tab, F, tmax), steps, args.warmup, False)
    assert torch.equal(outs["float32"], outs["binary16"])
    host = host_per_cut(cuts, tmax, dev)
    assert float((host - outs["float32"]).abs().max()) < 1e-4
    res["legs"]["host_per_cut"] = timed(lambda: host_per_cut(cuts, tmax, dev), 5, 1, False)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
