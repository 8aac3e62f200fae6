#!/usr/bin/env python3
"""Device reverberation (recorded RIR) in front of the feature launch, device resident, on the BASELINE configs[4] shape: 600 s mini-batches
of LibriSpeech-like cut lengths, half the cuts reverberated, a third of the cuts speed-perturbed (0.9 / 1.1) -> 80-dim fbank; at RIR lengths
L = 800 (early_only) and L = 8000.  Prints one JSON line, per L:

  * cuts/s of the mini-batch WITH the reverb (pack -> resample -> convolution -> gain -> feature launch, FusedMiniBatch.features_of_tracks)
    next to the same cuts WITHOUT it (the route of the commit before this tool: speed + feature launch pair);
  * the two new launches alone (HIP events around reverb_in_arena, after warm-up): 2 * sum(N) * L / t against the 157 TF vector peak, and
    their algorithmic bytes (sources and RIRs read once, outputs written once and read + written once more by the gain launch);
  * with --cpu P: the CPU path's arithmetic (tests/_reverb_ref.py::fft32, float32 FFTs of next_fast_len(N + L - 1)) over P processes on the
    same box: the route these cuts take without the device reverb;
  * with --torch-gpu: the same items through torch.fft on the device (a second baseline; the library links the HIP runtime only).

    python tools/bench_reverb.py [--batches 4] [--steps 10] [--cpu 16] [--torch-gpu] [--once]

--once runs ONE reverberated mini-batch (L = 8000) after the warm-up and exits (rocprofv3 --kernel-trace --stats -- python tools/bench_reverb.py --once)."""
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
VECTOR_PEAK_TFLOPS = 157.0
TAPS = (800, 8000)


def make_batch(rng, seconds=600.0):
    """-> per cut (samples, factor, reverberated?)"""
    cuts, total = [], 0.0
    while True:
        dur = float(np.clip(rng.normal(12.7, 3.6), 1.4, 24.5))
        if total + dur > seconds:
            break
        total += dur
        cuts.append((int(dur * SR), [1.0, 1.0, 0.9, 1.1, 1.0, 1.0][len(cuts) % 6], len(cuts) % 2 == 0))
    return cuts


def make_rir(rng, taps):
    h = rng.randn(taps) * np.exp(-6.0 * np.arange(taps) / taps) * 0.1
    h[min(40, taps - 1)] = 1.0
    return (np.round(h * 20000.0) / 32768.0).astype(np.float32)


def cpu_reverb(args):
    import _reverb_ref as R

    n, rir, seed = args
    x = np.random.RandomState(seed).rand(n).astype(np.float32) - np.float32(0.5)
    hs, shift = R.scale_and_shift(rir)
    return len(R.fft32(x, hs, shift, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4, help="distinct mini-batches cycled through")
    ap.add_argument("--steps", type=int, default=10, help="timed passes over the mini-batches")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu", type=int, default=0, help="processes of the host leg (0 = skip)")
    ap.add_argument("--torch-gpu", action="store_true")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    shapes = [make_batch(rng) for _ in range(args.batches)]
    rirs = {taps: [make_rir(rng, taps) for _ in range(4)] for taps in TAPS}
    res = {"workload": f"{args.batches} mini-batches of 600 s, {sum(len(b) for b in shapes)} cuts, half reverberated (4 distinct RIRs per mini-batch), "
                       "a third speed-perturbed, fbank80, device resident", "taps": {}}

    def out_len(n, factor):
        return int(round(n / factor)) - 2 if factor != 1.0 else n  # (a sample or two truncated)

    if args.cpu and not args.once:  # before the device is touched (worker processes are spawned, they never see a HIP context)
        import multiprocessing as mp

        with mp.get_context("spawn").Pool(args.cpu) as pool:
            for taps in TAPS:
                work = [(out_len(n, f), rirs[taps][k % 4], k) for k, (n, f, rv) in enumerate(shapes[0]) if rv]
                pool.map(cpu_reverb, work[: args.cpu])
                t0 = time.perf_counter()
                for _ in range(3):
                    pool.map(cpu_reverb, work, chunksize=1)
                res["taps"].setdefault(str(taps), {})["cpu_fft32"] = {
                    "processes": args.cpu, "reverberated_cuts": len(work), "ms_per_minibatch": round((time.perf_counter() - t0) / 3 * 1e3, 2),
                    "note": "float32 rfft / irfft of next_fast_len(N + L - 1) over in-memory samples (no decoding, no Speed)"}

    import lhotse_amd as LA
    from lhotse_amd import augmentation as A
    from lhotse_amd.input_strategies import FusedMiniBatch

    dev = torch.device("cuda", 0)
    fm = FusedMiniBatch(LA.HipFbank(LA.HipFbankConfig(device="cuda:0")))
    waves = [[torch.empty(n, device=dev).uniform_(-0.5, 0.5) for n, _, _ in b] for b in shapes]

    def batches_of(taps):
        out = []
        for b, ws in zip(shapes, waves):
            tr, wants = [], []
            for k, ((n, f, rv), x) in enumerate(zip(b, ws)):
                want = out_len(n, f)
                tr.append([(x, f, 0, None, True, want) + (((rirs[taps][k % 4], True),) if taps and rv else ())])
                wants.append(want)
            out.append((tr, wants))
        return out

    def run(batches):
        for tr, wants in batches:
            fm.features_of_tracks(tr, wants, SR)

    plain = batches_of(0)
    ncuts = sum(len(b) for b in shapes)
    for taps in reversed(TAPS) if args.once else TAPS:
        r = res["taps"].setdefault(str(taps), {})
        rvb = batches_of(taps)
        for _ in range(max(args.warmup, 2)):
            run(rvb), run(plain)
        torch.cuda.synchronize()
        if args.once:
            run(rvb[:1])
            torch.cuda.synchronize()
            return
        for name, batches in (("with_reverb", rvb), ("without_reverb", plain), ("with_reverb_again", rvb), ("without_reverb_again", plain)):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run(batches)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / args.steps
            r[name] = {"ms_per_minibatch": round(wall / len(batches) * 1e3, 3), "cuts_per_s": round(ncuts / wall, 1)}

        # the two new launches alone, on one arena: the reverberated cuts of mini-batch 0 at their output lengths
        lens = np.array([out_len(n, f) for n, f, rv in shapes[0] if rv], dtype=np.int64)
        hs = [A.scaled_rir(h) for h in rirs[taps]]
        l4 = (taps + 3) & ~3
        src = np.zeros(len(lens), dtype=np.int64)
        np.cumsum(((lens + 3) & ~3)[:-1], out=src[1:])
        rir0 = int(src[-1] + ((lens[-1] + 3) & ~3))
        front = rir0 + 4 * l4
        arena = torch.empty(front + A.reverb_tail_floats(lens), device=dev).uniform_(-0.5, 0.5)
        for k, (h, _) in enumerate(hs):
            arena[rir0 + k * l4 : rir0 + k * l4 + taps] = torch.from_numpy(h).to(dev)
        tabs = (src, lens, [rir0 + (k % 4) * l4 for k in range(len(lens))], [taps] * len(lens), [hs[k % 4][1] for k in range(len(lens))], [1] * len(lens), front)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = []
        for i in range(args.steps + 3):
            ev[0].record()
            A.reverb_in_arena(arena, *tabs)
            ev[1].record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(ev[0].elapsed_time(ev[1]))
        t = float(np.median(ms))
        flop = 2.0 * float(lens.sum()) * taps
        nbytes = 4 * (4 * int(lens.sum()) + 4 * taps)
        r["launches_of_one_minibatch"] = {
            "items": len(lens), "samples": int(lens.sum()), "conv_plus_gain_ms": round(t, 4), "TFLOPS": round(flop / t / 1e9, 2),
            "fraction_of_vector_peak": round(flop / t / 1e9 / VECTOR_PEAK_TFLOPS, 4), "algorithmic_MB": round(nbytes / 1e6, 2),
            "GBps": round(nbytes / t / 1e6, 1), "note": "HIP events around the call (launch gaps included)"}
        if args.torch_gpu:
            import _reverb_ref as R

            xs = [arena[int(o) : int(o) + int(n)] for o, n in zip(src, lens)]
            hd = [torch.from_numpy(h).to(dev) for h, _ in hs]

            def torch_route():
                outs = []
                for k, x in enumerate(xs):
                    size = R._next_fast_len(len(x) + taps - 1)
                    y = torch.fft.irfft(torch.fft.rfft(x, n=size) * torch.fft.rfft(hd[k % 4], n=size), n=size)[hs[k % 4][1] : hs[k % 4][1] + len(x)]
                    outs.append(y * torch.sqrt(x.square().sum() / y.square().sum()))
                return outs

            for _ in range(3):
                torch_route()
            ms = []
            for _ in range(args.steps):
                ev[0].record()
                torch_route()
                ev[1].record()
                torch.cuda.synchronize()
                ms.append(ev[0].elapsed_time(ev[1]))
            r["torch_fft_gpu_ms"] = round(float(np.median(ms)), 4)
        if "cpu_fft32" in r:
            r["device_route_beats_cpu"] = bool(r["with_reverb"]["ms_per_minibatch"] - r["without_reverb"]["ms_per_minibatch"] < r["cpu_fft32"]["ms_per_minibatch"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
