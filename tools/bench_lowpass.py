#!/usr/bin/env python3
"""The band bracket of LowpassUsingResampling on the device, on the BASELINE configs[4] shape: one 600 s mini-batch of LibriSpeech-like cut
lengths at 16 kHz, every second cut lowpassed (p = 0.5) with its own integer cutoff c, log-uniform in [3500, 8000): Resample(16000 -> 2c),
then Resample(2c -> 16000).  Prints one JSON line:

  * ``routed``: HIP events around the two ``resample_in_arena`` calls the chain makes (per direction: ONE ``hipfeat_sinc_run`` for the rate
    pairs without a dense bank + one ``hipfeat_resample`` launch per distinct pair that has one), median over --steps after a warm-up;
  * ``sinc_launches``: the same with every pair on the bankless kernel (``sinc_in_arena``): HIP events around the two ``hipfeat_sinc_run`` launches (``sinc_in_arena``: all lowpassed cuts of the mini-batch, each
    with its own ratio, per direction), median over --steps after a warm-up, with the plan + table copy inside the timed region;
  * ``dense_per_cut`` (--dense N cuts, 0 = skip): for the first N lowpassed cuts, what the route had to do before -- build the dense bank
    of the cut's two ratios on the host (``constants.sinc_resample_kernel``: float64, new x (2 width + orig) weights), upload it
    (``hipfeat_resampler_create``) and run ONE ``hipfeat_resample`` launch per direction: host seconds for the banks, HIP-event milliseconds for
    the launches alone, and the bank sizes -- or the library's refusal: the dense kernels stage ``orig`` input samples per hop in LDS, which
    ratios such as 8000:5969 exceed.  Only ratios whose two banks fit ``--dense-max-floats`` are taken.

    python tools/bench_lowpass.py [--steps 10] [--dense 2]

Nothing here compares against the parent commit: there such cuts went through cut.load_audio() on the CPU."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 16000


def make_batch(rng, seconds=600.0):
    """-> per cut (samples, cutoff or None)"""
    cuts, total = [], 0.0
    while True:
        dur = float(np.clip(rng.normal(12.7, 3.6), 1.4, 24.5))
        if total + dur > seconds:
            break
        total += dur
        cutoff = int(math.exp(rng.uniform(math.log(3500), math.log(8000)))) if len(cuts) % 2 == 0 else None  # lowpass.py:41-45
        cuts.append((int(dur * SR), cutoff))
    return cuts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dense", type=int, default=2, help="lowpassed cuts that also go through freshly built dense banks (0 = skip)")
    ap.add_argument("--dense-max-floats", type=int, default=1 << 27, help="largest dense bank that is built (floats)")
    args = ap.parse_args()

    from lhotse_amd import augmentation as A
    from lhotse_amd import constants as C

    cuts = make_batch(np.random.RandomState(0))
    dev = torch.device("cuda", 0)
    lens = np.array([n for n, _ in cuts], dtype=np.int64)
    offs = np.zeros(len(cuts), dtype=np.int64)
    np.cumsum(((lens + 3) & ~3)[:-1], out=offs[1:])
    front = int(offs[-1] + lens[-1])
    down = [None if c is None else (SR, 2 * c) for _, c in cuts]
    up = [None if c is None else (2 * c, SR) for _, c in cuts]
    o1, l1, end1 = A.resample_layout(offs, lens, down, front)
    o2, l2, end2 = A.resample_layout(o1, l1, up, end1)
    arena = torch.empty(end2 + 4, device=dev).uniform_(-0.5, 0.5)
    routes = [A.resample_route(*r) for r in down + up if r is not None]
    res = {"workload": f"one 600 s mini-batch at 16 kHz, {len(cuts)} cuts, {sum(c is not None for _, c in cuts)} lowpassed with their own cutoff",
           "samples_lowpassed": int(sum(n for n, c in cuts if c is not None)),
           "routes_of_the_rate_pairs": {"bank": routes.count("bank"), "sinc": routes.count("sinc"), "unserved": routes.count(None)}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ms = {"down": [], "up": [], "both": []}
    for i in range(args.steps + args.warmup):
        ev[0].record()
        A.sinc_in_arena(arena, offs, lens, down, front)
        ev[1].record()
        A.sinc_in_arena(arena, o1, l1, up, end1)
        ev[2].record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            ms["down"].append(ev[0].elapsed_time(ev[1])), ms["up"].append(ev[1].elapsed_time(ev[2])), ms["both"].append(ev[0].elapsed_time(ev[2]))
    res["sinc_launches"] = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
    res["sinc_launches"]["note"] = "ms, HIP events around sinc_in_arena (plan, table copy and launch gaps included); every rate pair on the bankless kernel"
    # the product's route: resample_in_arena sends the pairs with a dense bank to one hipfeat_resample launch each, the rest into one sinc launch
    ms = {"down": [], "up": [], "both": []}
    for i in range(args.steps + args.warmup):
        ev[0].record()
        A.resample_in_arena(arena, offs, lens, down, front)
        ev[1].record()
        A.resample_in_arena(arena, o1, l1, up, end1)
        ev[2].record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            ms["down"].append(ev[0].elapsed_time(ev[1])), ms["up"].append(ev[1].elapsed_time(ev[2])), ms["both"].append(ev[0].elapsed_time(ev[2]))
    res["routed"] = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
    res["routed"]["dense_launches"] = {"down": len({r for r in down if r is not None and A.resample_route(*r) == "bank"}),
                                       "up": len({r for r in up if r is not None and A.resample_route(*r) == "bank"})}
    res["routed"]["note"] = "ms, HIP events around resample_in_arena: what the chain runs -- one sinc launch + one dense launch per distinct banked ratio, per direction"

    dense = []
    for k, (n, c) in enumerate(cuts):
        if c is None or len(dense) >= args.dense:
            continue
        if max(A._sinc_bank_floats(SR, 2 * c), A._sinc_bank_floats(2 * c, SR)) > args.dense_max_floats:
            continue
        t0 = time.perf_counter()
        banks = [C.sinc_resample_kernel(SR, 2 * c), C.sinc_resample_kernel(2 * c, SR)]
        host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        rs, refused = [], None
        for (kernel, width, orig, new), (a, b) in zip(banks, ((SR, 2 * c), (2 * c, SR))):
            r = A.HipResampleTensor.__new__(A.HipResampleTensor)  # the dense route for a ratio the router no longer sends there
            r.orig_freq, r.new_freq, r.kernel, r.width, r.orig, r.new, r.bankless = a, b, kernel, width, orig, new, False
            from lhotse_amd import _lib

            r.lib, r.device, out = _lib.load(), dev, np.zeros(1, dtype=np.uint64)
            r.handle = 0
            try:
                r.lib.check("hipfeat_resampler_create", orig, new, width, _lib.addr(kernel), 0, _lib.addr(out))
            except _lib.HipFeatError as e:  # (the dense kernels stage `orig` input samples per hop in LDS: ratios such as 8000:5969 do not fit)
                refused = str(e)
                break
            r.handle = int(out[0])
            r.kernel_name = r.lib.string("hipfeat_resampler_kernel_name", r.handle)
            rs.append(r)
        if refused is not None:
            dense.append({"cutoff": c, "samples": n, "bank_floats": [int(b[0].size) for b in banks], "host_s_building_the_banks": round(host_s, 3),
                          "refused_by_hipfeat_resampler_create": refused})
            for r in rs:
                r.close()
            continue
        torch.cuda.synchronize()
        upload_s = time.perf_counter() - t0
        x = arena[int(offs[k]) : int(offs[k]) + n]
        t = []
        for i in range(args.steps + args.warmup):
            ev[0].record()
            y, yo, yl = rs[0].run(x, np.zeros(1, dtype=np.int64), np.array([n], dtype=np.int64))
            rs[1].run(y, yo, yl)
            ev[1].record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                t.append(ev[0].elapsed_time(ev[1]))
        dense.append({"cutoff": c, "samples": n, "bank_floats": [int(b[0].size) for b in banks], "kernel": [r.kernel_name for r in rs],
                      "host_s_building_the_banks": round(host_s, 3), "s_uploading": round(upload_s, 3), "ms_two_launches": round(float(np.median(t)), 4)})
        for r in rs:
            r.close()
    if dense:
        res["dense_per_cut"] = dense
    print(json.dumps(res))


if __name__ == "__main__":
    main()
