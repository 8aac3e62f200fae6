#!/usr/bin/env python3
"""Device mixing of MixedCut tracks in front of the feature launch, device resident, on the BASELINE configs[4] shape: 600 s mini-batches
of LibriSpeech-like cut lengths, half the cuts mixed with one to three noise tracks at 10-20 dB, a third of the cuts speed-perturbed
(0.9 / 1.1) -> 80-dim fbank.  Prints one JSON line:

  * cuts/s of the mini-batch WITH mixing (pack on the device -> resample -> energy -> mix -> feature launch, FusedMiniBatch.features_of_tracks)
    next to the same cuts WITHOUT their noise tracks (the route the commit before this tool had: speed + feature launch pair);
  * the two new launches alone (HIP events around mix_in_arena) and their bytes/s against the algorithmic traffic -- every track that
    needs an energy read once more, every track read once by the mix, the mixed cuts written once -- next to what the per-factor
    resample launches reach on the same arena (input read + output written);
  * with --cpu N: the reference arithmetic on the host (tests/_mix_ref.py, the numpy restatement of MixedCut.load_audio) over N processes.

    python tools/bench_mix.py [--batches 8] [--steps 20] [--cpu 16] [--once]

--once runs ONE mixed mini-batch after the warm-up and exits (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/bench_mix.py --once)."""
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


def make_batch(rng, seconds=600.0):
    """-> per cut (speech samples, factor, [(noise samples, offset, snr)])"""
    cuts, total = [], 0.0
    while True:
        dur = float(np.clip(rng.normal(12.7, 3.6), 1.4, 24.5))
        if total + dur > seconds:
            break
        total += dur
        n = int(dur * SR)
        factor = [1.0, 1.0, 0.9, 1.1, 1.0, 1.0][len(cuts) % 6]  # a third of the cuts perturbed
        noises = []
        if len(cuts) % 2 == 0:  # half of the cuts mixed
            want = int(round(n / factor)) if factor != 1.0 else n
            for _ in range(int(rng.randint(1, 4))):
                m = int(rng.randint(SR, max(SR + 1, want)))
                noises.append((m, int(rng.randint(0, want - m + 1)), float(rng.uniform(10, 20))))
        cuts.append((n, factor, noises))
    return cuts


def cpu_mix(args):
    from _mix_ref import mix_tracks

    tracks, ref, want = args
    return len(mix_tracks(tracks, ref, want, energy="float32"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8, help="distinct mini-batches cycled through")
    ap.add_argument("--steps", type=int, default=20, help="timed passes over the mini-batches")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu", type=int, default=0, help="processes of the host leg (0 = skip)")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    shapes = [make_batch(rng) for _ in range(args.batches)]
    res = {"workload": f"{args.batches} mini-batches of 600 s, {sum(len(b) for b in shapes)} cuts, half mixed with 1-3 noise tracks, a third speed-perturbed, fbank80, device resident"}

    if args.cpu and not args.once:  # before the device is touched (worker processes are spawned, they never see a HIP context)
        import multiprocessing as mp

        work = []
        for n, factor, noises in shapes[0]:
            if noises:
                want = int(round(n / factor)) if factor != 1.0 else n
                tr = [((rng.rand(want).astype(np.float32) - 0.5), 0, None)] + [((rng.rand(m).astype(np.float32) - 0.5) * 0.3, o, s) for m, o, s in noises]
                work.append((tr, 0, want))
        with mp.get_context("spawn").Pool(args.cpu) as pool:
            pool.map(cpu_mix, work[:2])
            t0 = time.perf_counter()
            for _ in range(3):
                pool.map(cpu_mix, work, chunksize=1)
            res["cpu_reference_mix"] = {"processes": args.cpu, "mixed_cuts": len(work), "ms_per_minibatch": round((time.perf_counter() - t0) / 3 * 1e3, 2),
                                        "note": "numpy restatement of MixedCut.load_audio over in-memory tracks (no decoding, no Speed)"}

    import lhotse_amd as LA
    from lhotse_amd import augmentation as A
    from lhotse_amd.input_strategies import FusedMiniBatch

    dev = torch.device("cuda", 0)
    fm = FusedMiniBatch(LA.HipFbank(LA.HipFbankConfig(device="cuda:0")))
    mixed, plain = [], []
    for b in shapes:
        mt, pt, wants = [], [], []
        for n, factor, noises in b:
            x = torch.empty(n, device=dev).uniform_(-0.5, 0.5)
            want = int(round(n / factor)) - 2 if factor != 1.0 else n  # (a sample or two truncated)
            speech = (x, factor, 0, None, True, want)
            mt.append([speech] + [(torch.empty(m, device=dev).uniform_(-0.2, 0.2), 1.0, o, s, False, m) for m, o, s in noises if o + m <= want])
            pt.append([speech])
            wants.append(want)
        mixed.append((mt, wants))
        plain.append((pt, wants))

    def run(batches):
        for tr, wants in batches:
            fm.features_of_tracks(tr, wants, SR)

    for _ in range(max(args.warmup, 3)):
        run(mixed), run(plain)
    torch.cuda.synchronize()
    if args.once:
        run(mixed[:1])
        torch.cuda.synchronize()
        return
    ncuts = sum(len(b) for b in shapes)
    for name, batches in (("with_mixing", mixed), ("without_mixed_cuts", plain), ("with_mixing_again", mixed), ("without_mixed_cuts_again", plain)):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            run(batches)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.steps
        res[name] = {"ms_per_minibatch": round(wall / len(batches) * 1e3, 3), "cuts_per_s": round(ncuts / wall, 1)}

    # the two new launches alone, and the resample launches, on one arena
    tr, wants = mixed[0]
    items = [t[0] for c in tr for t in c]
    factors = [t[1] for c in tr for t in c]
    lens = np.array([len(x) for x in items], dtype=np.int64)
    offs = np.zeros(len(lens), dtype=np.int64)
    np.cumsum(lens[:-1], out=offs[1:])
    front = int(lens.sum())
    res_floats = A.perturbed_tail_floats(lens, factors, SR)
    arena = torch.empty(((front + 3) & ~3) + res_floats + front + 4 * len(items) + 64, device=dev)
    arena[:front] = torch.cat(items)
    po, pl = A.perturb_speed_in_arena(arena, offs, lens, factors, SR, front)
    first, so, sl, do, snrs, refs, cap, k = [0], [], [], [], [], [], [], 0
    for c, w in zip(tr, wants):
        for t in c:
            so.append(int(po[k])), sl.append(min(int(pl[k]), t[5])), do.append(t[2]), snrs.append(t[3])
            k += 1
        if len(c) > 1:
            first.append(len(so)), refs.append(0), cap.append(w)
        else:  # (plain cuts are not mixed)
            del so[first[-1]:], sl[first[-1]:], do[first[-1]:], snrs[first[-1]:]
    mix_start = ((front + 3) & ~3) + res_floats
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    rs_ms, mix_ms = [], []
    for i in range(args.steps + 3):
        ev[0].record()
        A.perturb_speed_in_arena(arena, offs, lens, factors, SR, front)
        ev[1].record()
        A.mix_in_arena(arena, first, so, sl, do, snrs, refs, cap, mix_start)
        ev[2].record()
        torch.cuda.synchronize()
        if i >= 3:
            rs_ms.append(ev[0].elapsed_time(ev[1])), mix_ms.append(ev[1].elapsed_time(ev[2]))
    sl_a, first_a = np.array(sl), np.array(first)
    out_n = A.mixed_num_samples(first, sl, do, cap)
    energy_n = sum(int(sl_a[a:b].sum()) for a, b in zip(first_a[:-1], first_a[1:]))  # (every track of a mixed cut has an SNR or is its reference)
    mix_bytes = 4 * (2 * energy_n + int(out_n.sum()))
    fac = np.array(factors)
    rs_bytes = 4 * (int(lens[fac != 1.0].sum()) + int(pl[fac != 1.0].sum()))
    res["launches_of_one_minibatch"] = {
        "mixed_cuts": len(first) - 1, "tracks": len(so), "energy_plus_mix_ms": round(float(np.median(mix_ms)), 4), "energy_plus_mix_algorithmic_MB": round(mix_bytes / 1e6, 2),
        "energy_plus_mix_GBps": round(mix_bytes / np.median(mix_ms) / 1e6, 1), "resample_ms": round(float(np.median(rs_ms)), 4),
        "resample_algorithmic_MB": round(rs_bytes / 1e6, 2), "resample_GBps": round(rs_bytes / np.median(rs_ms) / 1e6, 1),
        "note": "HIP events around the calls (launch gaps included); one 600 s mini-batch is far too small to fill the chip's bandwidth"}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
