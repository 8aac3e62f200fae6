#!/usr/bin/env python3
"""The collate launch (lhotse_amd.augmentation.collate_in_arena: ragged cuts of one device arena -> the dense zero-padded (B, Tmax) tensor)
against the two ways of getting that tensor without it, in one process, on two shapes:

  * "config5": the BASELINE configs[4] shape, a ragged 600 s mini-batch of LibriSpeech-like cuts (about 10 s each) at 16 kHz;
  * "one_30s": one 30 s cut (the Whisper window): what a launch costs when there is next to nothing to move.

Per shape and output type, by HIP events around the call (launch gaps and the staged row table included), the median of --steps timed runs
after --warmup untimed ones:

  * collate            the new launch; sources packed on 16-byte boundaries (as pack_to_device packs host items);
  * collate_misaligned the same with the sources back to back at every residue modulo 4 (as device-resident items are packed): the
                       16-byte loads of the kernel then straddle 16-byte boundaries;
  * baseline_host      what return_audio=True did before there was a launch: one blocking arena[o : o + n].cpu() per cut, zero padding on the
                       host (collate_vectors: a filled tensor + one slice copy per cut), one .to(device) back -- by the host clock around a
                       device synchronise, since most of it is host time;
  * baseline_torch     torch on the device: torch.zeros(B, Tmax) + one slice copy per cut (B + 1 launches).

Bytes: 4 * sum(len) read + sizeof(out type) * B * Tmax written; GB/s = bytes / time, next to the 6.29 TB/s the micro-architecture guide
measured for a float4 copy.  Every variant's result is compared with the first one's before anything is timed.  Prints one JSON line and
writes it to --out (default profiles/collate_bench.json).

    python tools/bench_collate.py [--steps 30] [--warmup 5] [--out profiles/collate_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 16000
COPY_ROOF_TBPS = 6.29  # MI355X, float4 copy


def config5_lengths(rng, seconds=600.0):
    lens, total = [], 0.0
    while True:
        dur = float(np.clip(rng.normal(12.7, 3.6), 1.4, 24.5))
        if total + dur > seconds:
            break
        total += dur
        lens.append(int(dur * SR))
    return np.asarray(lens, dtype=np.int64)


def layout(lens, aligned):
    offs = np.zeros(len(lens), dtype=np.int64)
    if aligned:
        np.cumsum(((lens + 3) & ~3)[:-1], out=offs[1:])
    else:  # back to back behind one float: with odd lengths every residue modulo 4 occurs
        np.cumsum(lens[:-1], out=offs[1:])
        offs += 1
    return offs


def median_ms_events(fn, steps, warmup):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(steps + warmup):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def median_ms_host(fn, steps, warmup):
    ms = []
    for i in range(steps + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="timed runs per variant (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collate_bench.json"))
    args = ap.parse_args()
    steps = max(args.steps, 20)
    if not torch.cuda.is_available():
        raise SystemExit("bench_collate.py measures on the GPU: no HIP device is visible")

    from lhotse_amd import augmentation as A

    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    shapes = {"config5": config5_lengths(rng) | 1, "one_30s": np.asarray([30 * SR], dtype=np.int64)}
    res = {"tool": "tools/bench_collate.py", "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": args.warmup, "timing": "median (min, max) in ms",
           "copy_roof_TBps": COPY_ROOF_TBPS, "shapes": {}}
    for name, lens in shapes.items():
        B, tmax = len(lens), int(lens.max())
        r = res["shapes"][name] = {"cuts": B, "Tmax": tmax, "samples": int(lens.sum()), "padding_share": round(1 - float(lens.sum()) / (B * tmax), 4)}
        offs = {True: layout(lens, True), False: layout(lens, False)}
        if B > 4:
            assert sorted({int(o) % 4 for o in offs[False]}) == [0, 1, 2, 3]
        arena = torch.empty(int(max(offs[True][-1], offs[False][-1]) + lens[-1]) + 8, device=dev).uniform_(-0.5, 0.5)
        for dtype, key in ((torch.float32, "float32"), (torch.float16, "float16"), (torch.bfloat16, "bfloat16")):
            nbytes = 4 * int(lens.sum()) + torch.empty((), dtype=dtype).element_size() * B * tmax
            out = torch.empty((B, tmax), dtype=dtype, device=dev)
            legs = r.setdefault(key, {"algorithmic_MB": round(nbytes / 1e6, 3)})

            def collate(aligned):
                return A.collate_in_arena(arena, offs[aligned], lens, row_len=tmax, dtype=dtype, out=out)[0]

            def baseline_torch(aligned=True):
                o = torch.zeros((B, tmax), dtype=dtype, device=dev)
                for i, (s, n) in enumerate(zip(offs[aligned].tolist(), lens.tolist())):
                    o[i, :n] = arena[s : s + n]
                return o

            def baseline_host(aligned=True):
                cuts = [arena[s : s + n].cpu() for s, n in zip(offs[aligned].tolist(), lens.tolist())]
                padded = torch.zeros((B, tmax), dtype=torch.float32)  # collate_vectors(..., padding_value=0)
                for i, c in enumerate(cuts):
                    padded[i, : len(c)] = c
                return padded.to(dev).to(dtype)

            want = baseline_torch(True)
            torch.cuda.synchronize()
            for aligned in (True, False):  # faster and different is not faster
                assert torch.equal(collate(aligned).view(torch.int16 if dtype != torch.float32 else torch.int32),
                                   baseline_torch(aligned).view(torch.int16 if dtype != torch.float32 else torch.int32)), (name, key, aligned)
            assert torch.equal(baseline_host(True), want)
            variants = [("collate", lambda: collate(True), median_ms_events), ("collate_misaligned", lambda: collate(False), median_ms_events),
                        ("baseline_torch", baseline_torch, median_ms_events)]
            if dtype == torch.float32:
                variants.append(("baseline_host", baseline_host, median_ms_host))
            for _ in range(2):  # alternate the variants: two passes, the second one is reported next to the first
                for leg, fn, timer in variants:
                    med, lo, hi = timer(fn, steps if leg != "baseline_host" else 20, args.warmup)
                    legs.setdefault(leg, []).append({"ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4), "GBps": round(nbytes / med / 1e6, 1),
                                                     "of_copy_roof": round(nbytes / med / 1e6 / (COPY_ROOF_TBPS * 1e3), 4)})
            legs["collate_over_baseline_torch"] = round(legs["collate"][-1]["ms"] / legs["baseline_torch"][-1]["ms"], 3)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
