#!/usr/bin/env python3
"""Device level changes (Volume, Clipping) in front of the feature launch, device resident, on the BASELINE configs[4] shape: 600 s
mini-batches of LibriSpeech-like cut lengths -> 80-dim fbank; every cut scaled, half of them clipped.  THE MEASUREMENT STILL TO BE TAKEN on
an MI355X: no throughput figure of the level route exists yet, and nothing in the documents quotes one.  Prints one JSON line, per form
("plain": Volume + Clipping in place; "oversampled": the Clipping between Resample(sr -> k sr) and Resample(k sr -> sr), k = 2 and 4):

  * cuts/s of the mini-batch WITH the level ops (pack -> [up-resample ->] peak -> apply [-> down-resample] -> feature launch,
    FusedMiniBatch.features_of_tracks with 9-element tracks) next to the same cuts WITHOUT them (the route of the commit before this tool);
  * the level launches alone (HIP events around level_in_arena, after warm-up) for a hard and for a soft clip -- the soft one evaluates a
    float64 tanh per sample, and whether that shows in a memory-bound kernel is the open question this settles -- with their algorithmic
    bytes (peak: every sample read once; apply: read once, written once) and the GB/s they amount to;
  * with --cpu P: the CPU path's arithmetic (numpy, as lhotse's Volume / Clipping run it) over P processes on the same box.

    python tools/bench_level.py [--batches 4] [--steps 10] [--cpu 16] [--once]

--once runs ONE oversampled (k = 4) mini-batch after the warm-up and exits (rocprofv3 --kernel-trace --stats -- python tools/bench_level.py --once):
the split between the two extra resample passes and the level launches is what decides whether fusing the oversampling into the clipping
kernel is worth building."""
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
SR = 16000
FORMS = (("plain", None), ("oversampled_2", 2), ("oversampled_4", 4))


def make_batch(rng, seconds=600.0):
    """-> per cut (samples, clipped?)"""
    cuts, total = [], 0.0
    while True:
        dur = float(np.clip(rng.normal(12.7, 3.6), 1.4, 24.5))
        if total + dur > seconds:
            break
        total += dur
        cuts.append((int(dur * SR), len(cuts) % 2 == 0))
    return cuts


def blocks_of(clipped, k, hard):
    clip = ("clip", hard, 12.0, True)
    if not clipped:
        return ([("level", [("volume", 0.7)])], None)
    if k is None:
        return ([("level", [("volume", 0.7), clip])], None)
    return ([("level", [("volume", 0.7)]), ("up", k), ("level", [clip]), ("down", k)], None)


def cpu_level(args):
    import _level_ref as L

    n, clipped, seed = args
    x = L.signal(seed, n, 0.5) * np.float32(0.7)
    if clipped:  # clipping.py:28-61 on float32 arrays
        p = np.max(np.abs(x))
        x = np.tanh(x / p * np.float32(3.98)) / np.float32(3.98) * p
    return len(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4, help="distinct mini-batches cycled through")
    ap.add_argument("--steps", type=int, default=10, help="timed passes over the mini-batches")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu", type=int, default=0, help="processes of the host leg (0 = skip)")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    shapes = [make_batch(rng) for _ in range(args.batches)]
    res = {"workload": f"{args.batches} mini-batches of 600 s, {sum(len(b) for b in shapes)} cuts, every cut scaled, half clipped (soft, 12 dB), fbank80, "
                       "device resident", "forms": {}}

    if args.cpu and not args.once:  # before the device is touched (worker processes are spawned, they never see a HIP context)
        import multiprocessing as mp

        with mp.get_context("spawn").Pool(args.cpu) as pool:
            work = [(n, c, k) for k, (n, c) in enumerate(shapes[0])]
            pool.map(cpu_level, work[: args.cpu])
            t0 = time.perf_counter()
            for _ in range(3):
                pool.map(cpu_level, work, chunksize=1)
            res["cpu_numpy"] = {"processes": args.cpu, "cuts": len(work), "ms_per_minibatch": round((time.perf_counter() - t0) / 3 * 1e3, 2),
                                "note": "float32 numpy over in-memory samples (no decoding, no oversampling)"}

    import lhotse_amd as LA
    from lhotse_amd import augmentation as A
    from lhotse_amd.input_strategies import FusedMiniBatch

    dev = torch.device("cuda", 0)
    fm = FusedMiniBatch(LA.HipFbank(LA.HipFbankConfig(device="cuda:0")))
    waves = [[torch.empty(n, device=dev).uniform_(-0.5, 0.5) for n, _ in b] for b in shapes]

    def batches_of(k, level=True):
        return [([[(x, 1.0, 0, None, True, n, None, None, blocks_of(c, k, False) if level else None)] for (n, c), x in zip(b, ws)], [n for n, _ in b])
                for b, ws in zip(shapes, waves)]

    def run(batches):
        for tr, wants in batches:
            fm.features_of_tracks(tr, wants, SR)

    plain = batches_of(None, level=False)
    ncuts = sum(len(b) for b in shapes)
    for name, k in reversed(FORMS) if args.once else FORMS:
        r = res["forms"].setdefault(name, {})
        lvl = batches_of(k)
        for _ in range(max(args.warmup, 2)):
            run(lvl), run(plain)
        torch.cuda.synchronize()
        if args.once:
            run(lvl[:1])
            torch.cuda.synchronize()
            return
        for leg, batches in (("with_level", lvl), ("without_level", plain), ("with_level_again", lvl), ("without_level_again", plain)):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run(batches)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / args.steps
            r[leg] = {"ms_per_minibatch": round(wall / len(batches) * 1e3, 3), "cuts_per_s": round(ncuts / wall, 1)}

    # the level launches alone, on one arena: mini-batch 0, every cut clipped in place
    lens = np.array([n for n, _ in shapes[0]], dtype=np.int64)
    src = np.zeros(len(lens), dtype=np.int64)
    np.cumsum(((lens + 3) & ~3)[:-1], out=src[1:])
    arena = torch.empty(int(src[-1] + lens[-1]), device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for name, prog in (("scale", [("volume", 0.7)]), ("hard_clip", [("volume", 0.7), ("clip", True, 12.0, True)]), ("soft_clip", [("volume", 0.7), ("clip", False, 12.0, True)])):
        ms = []
        for i in range(args.steps + 3):
            arena.uniform_(-0.5, 0.5)
            ev[0].record()
            A.level_in_arena(arena, src, lens, [prog] * len(lens))
            ev[1].record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(ev[0].elapsed_time(ev[1]))
        t = float(np.median(ms))
        nbytes = 4 * int(lens.sum()) * (2 if name == "scale" else 3)
        res.setdefault("launches_of_one_minibatch", {})[name] = {
            "items": len(lens), "samples": int(lens.sum()), "ms": round(t, 4), "algorithmic_MB": round(nbytes / 1e6, 2), "GBps": round(nbytes / t / 1e6, 1), "note": "HIP events around the call (launch gaps included)"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
