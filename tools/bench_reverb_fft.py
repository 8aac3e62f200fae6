#!/usr/bin/env python3
"""The two routes of the device reverb against each other: direct form (kernel_reverb.hpp) and partitioned FFT convolution
(kernel_reverb_fft.hpp), HIP events around hipfeat_reverb_run alone (the plan is host work and is made outside the events).

Workload: 24 items x 200 000 samples (the reverberated half of a 600 s mini-batch), 4 distinct impulse responses, all normalised, at
L = 256 ... 32768 taps; and ONE item of 30 s (480 000 samples), where the fixed costs of four launches show.  Per L the legs alternate
(direct, fft, torch) inside every repetition, after a warm-up of all of them; the figure is the median of --reps (30) repetitions, in one
process.  The torch leg is the reference's call sequence (rfft, rfft, product, irfft at next_fast_len(N + L - 1), slice, power gain) as
torch.fft ops on the same device, item by item, as a second baseline.

    python tools/bench_reverb_fft.py [--reps 30] [--out profiles/reverb_fft_bench.json]
    rocprofv3 --kernel-trace --stats -- python tools/bench_reverb_fft.py --once 16384     (the split of launches A and B, a run of its own)

Prints one JSON line (and writes it to --out): per L the three medians in ms, fft / direct, and `auto_min_taps`: the smallest L of the
grid from which the FFT route is faster than the direct form at every larger L (null if it is not at the largest)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
TAPS = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768)
EARLY_ONLY_TAPS = 800  # ReverbWithImpulseResponse(early_only=True) at 16 kHz: reported, not part of the crossover grid


def make_rir(rng, taps):
    h = rng.randn(taps) * np.exp(-6.0 * np.arange(taps) / taps) * 0.1
    h[min(40, taps - 1)] = 1.0
    return (np.round(h * 20000.0) / 32768.0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--items", type=int, default=24)
    ap.add_argument("--samples", type=int, default=200000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", type=int, default=0, metavar="L", help="one FFT-route run at L taps after a warm-up, then exit (for a kernel trace)")
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()

    import _reverb_ref as R
    from lhotse_amd import augmentation as A

    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    rv = A.get_or_create_reverb(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def case(items, samples, taps):
        """-> {leg: callable that returns the milliseconds of one run}"""
        lens = np.full(items, samples, dtype=np.int64)
        n4, l4 = (samples + 3) & ~3, (taps + 3) & ~3
        nr = min(4, items)
        hs = [A.scaled_rir(make_rir(rng, taps)) for _ in range(nr)]
        rir0 = items * n4
        front = rir0 + nr * l4
        ro = [rir0 + (k % nr) * l4 for k in range(items)]
        shifts = [hs[k % nr][1] for k in range(items)]
        arena = torch.empty(front + A.reverb_fft_tail_floats(lens, [taps] * items, shifts, ro), device=dev)
        arena[:front].uniform_(-0.5, 0.5)
        for k, (h, _) in enumerate(hs):
            arena[rir0 + k * l4 : rir0 + k * l4 + taps] = torch.from_numpy(h).to(dev)
        tabs = (np.arange(items, dtype=np.int64) * n4, lens, ro, [taps] * items, shifts, [1] * items, front)

        def device_leg(method):
            def run():
                ticket, _, _ = rv.plan(*tabs, method)
                ev[0].record()
                rv.run(ticket, arena)
                ev[1].record()
                torch.cuda.synchronize()
                return ev[0].elapsed_time(ev[1])
            return run

        xs = [arena[k * n4 : k * n4 + samples] for k in range(items)]
        hd = [arena[rir0 + k * l4 : rir0 + k * l4 + taps] for k in range(nr)]
        size = R._next_fast_len(samples + taps - 1)

        def torch_leg():
            ev[0].record()
            for k, x in enumerate(xs):
                y = torch.fft.irfft(torch.fft.rfft(x, n=size) * torch.fft.rfft(hd[k % nr], n=size), n=size)[shifts[k] : shifts[k] + samples]
                y = y * torch.sqrt(x.square().sum() / y.square().sum())
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1])

        legs = {"direct": device_leg("direct"), "fft": device_leg("fft")}
        if not args.no_torch:
            legs["torch_fft"] = torch_leg
        return legs

    def measure(items, samples, taps):
        legs = case(items, samples, taps)
        for _ in range(args.warmup):
            for run in legs.values():
                run()
        ms = {name: [] for name in legs}
        for _ in range(args.reps):
            for name, run in legs.items():  # the legs alternate inside a repetition
                ms[name].append(run())
        out = {name + "_ms": round(float(np.median(v)), 4) for name, v in ms.items()}
        out["fft_over_direct"] = round(out["fft_ms"] / out["direct_ms"], 3)
        out["spread"] = {name: [round(float(np.percentile(v, 10)), 4), round(float(np.percentile(v, 90)), 4)] for name, v in ms.items()}
        return out

    if args.once:
        legs = case(args.items, args.samples, args.once)
        for _ in range(2):
            legs["fft"]()
        legs["fft"]()
        return

    res = {"workload": f"{args.items} items x {args.samples} samples, 4 distinct impulse responses, normalised; HIP events around hipfeat_reverb_run; "
                       f"medians of {args.reps}, legs alternating, warm-up {args.warmup}, one process",
           "device": torch.cuda.get_device_name(0), "minibatch": {}, "one_item_30s": {}}
    for taps in TAPS + (EARLY_ONLY_TAPS,):
        res["minibatch"][str(taps)] = measure(args.items, args.samples, taps)
        res["one_item_30s"][str(taps)] = measure(1, 480000, taps)

    def crossover(table):
        best = None
        for taps in reversed(TAPS):
            if table[str(taps)]["fft_ms"] < table[str(taps)]["direct_ms"]:
                best = taps
            else:
                break
        return best

    res["auto_min_taps"] = crossover(res["minibatch"])
    res["auto_min_taps_one_item_30s"] = crossover(res["one_item_30s"])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
