#!/usr/bin/env python3
"""The statistics launches (lhotse_amd.HipStatsAccumulator.update: per-bin sum and unnormalised variance of the cuts of a mini-batch
into float64 totals on the device) against the two things they replace, in one process.

Workload: the 600 s mini-batch of 80-dim log-mel features -- 48 cuts of about 12.5 s, about 60 k frames at 100 frames per second -- as
the packed ``(sum T, F)`` device matrix, float32 and binary16.

Legs, the median of --steps timed runs after --warmup untimed ones:

  * float32 / binary16 "launches": one ``update`` with all cuts (table staging, partial launch, fold launch), by HIP events around the
    call; "per_cut_updates": one ``update`` per cut (48 launch pairs);
  * "torch_on_device": the torch restatement on the device, float64 per cut -- ``x.double().sum(0)``, ``((x.double() - mean) ** 2).sum(0)``
    and the reference's update expression on device tensors, in a loop over the cuts; by HIP events;
  * "host_per_cut": what ``CutSet.compute_global_feature_stats`` does with an extractor's output -- per cut one device -> host copy and
    the numpy ``StatsAccumulator`` arithmetic (tests/_stats_ref.py::ReferenceStatement); by the host clock.

Every leg's result is held to the longdouble truth before anything is timed, and the errors are recorded.  Prints one JSON line and
writes it to --out (default profiles/stats_bench.json).

    python tools/bench_stats.py [--steps 30] [--warmup 5] [--out profiles/stats_bench.json]"""
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


def workload(rng, cuts=48, seconds=600.0):
    """-> [(n, F) float32], binary16-representable log-mel-like values; the durations sum to ``seconds``."""
    dur = np.clip(rng.normal(12.5, 3.6, cuts), 1.4, 24.5)
    dur *= seconds / dur.sum()
    return [(rng.standard_normal((int(d * 100), F)) * 2.5 - 8.0).astype(np.float16).astype(np.float32) for d in dur]


def torch_on_device(parts):
    """The reference's arithmetic on device tensors, float64 per cut -> (total_frames, total_sum, total_unnorm_var)."""
    tn, tsum, tvar = 0, None, None
    for x in parts:
        xd = x.double()
        n, s = xd.shape[0], xd.sum(0)
        m2 = ((xd - s / n) ** 2).sum(0)
        if tn > 0:
            ratio = tn / n
            tvar = tvar + m2 + ratio / (tn + n) * (tsum / ratio - s) ** 2
            tsum = tsum + s
        else:
            tsum, tvar = s, m2
        tn += n
    return tn, tsum, tvar


def host_per_cut(parts, ref_cls):
    acc = ref_cls(F)
    for x in parts:
        acc.update(x.cpu().numpy())
    return acc


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_bench.json"))
    args = ap.parse_args()
    steps = max(args.steps, 20)
    if not torch.cuda.is_available():
        raise SystemExit("bench_stats.py measures on the GPU: no HIP device is visible")

    import _stats_ref as S

    from lhotse_amd import HipStatsAccumulator

    mats = workload(np.random.RandomState(0))
    frames = [len(m) for m in mats]
    res = {"tool": "tools/bench_stats.py", "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": args.warmup, "timing": "median (min, max) in ms",
           "cuts": len(mats), "frames": int(sum(frames)), "F": F, "errors": "max over bins of |value - longdouble truth| / scale: [mean, std]", "legs": {}}
    ref = S.ReferenceStatement(F)
    for m in mats:
        ref.update(m)
    ref_err = S.errors(ref.norm_means, ref.norm_stds, mats)
    res["reference_statement_error"] = list(ref_err)

    def held(name, means, stds):
        err = S.errors(means, stds, mats)
        assert all(e <= max(2.0 * r, 1e-13) for e, r in zip(err, ref_err)), (name, err, ref_err)  # faster and different is not faster
        return list(err)

    acc = HipStatsAccumulator(F)
    for key, dt in (("float32", torch.float32), ("binary16", torch.float16)):
        packed = torch.from_numpy(np.concatenate(mats)).cuda().to(dt)
        parts = list(packed.split(frames))
        acc.reset()
        acc.update(packed, frames)
        got = acc.get()
        legs = res["legs"][key] = {"input_MB": round(packed.numel() * packed.element_size() / 1e6, 2), "error": held(key, got["norm_means"], got["norm_stds"])}

        def one_update():
            acc.reset()
            acc.update(packed, frames)

        def per_cut():
            acc.reset()
            for p in parts:
                acc.update(p)

        legs["launches"] = timed(one_update, steps, args.warmup, True)
        legs["per_cut_updates"] = timed(per_cut, steps, args.warmup, True)
        if key == "float32":
            tn, tsum, tvar = torch_on_device(parts)
            res["legs"]["torch_on_device"] = {"error": held("torch", (tsum / tn).cpu().numpy(), torch.sqrt(tvar / tn).cpu().numpy())}
            res["legs"]["torch_on_device"].update(timed(lambda: torch_on_device(parts), steps, args.warmup, True))
            host = host_per_cut(parts, S.ReferenceStatement)
            res["legs"]["host_per_cut"] = {"error": held("host", host.norm_means, host.norm_stds)}
            res["legs"]["host_per_cut"].update(timed(lambda: host_per_cut(parts, S.ReferenceStatement), 5, 1, False))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
