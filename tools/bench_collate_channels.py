#!/usr/bin/env python3
"""The sources form of the collate launch (lhotse_amd.augmentation.collate_sources_in_arena: the channels of multi-channel cuts in one
device arena -> the mono downmix (B, Tmax) or the (B, C, Tmax) tensor, ONE launch each) against the ways of getting those tensors without
it, in one process, on two shapes of 8-channel cuts:

  * "config5_8ch": the BASELINE configs[4] shape, a ragged 600 s mini-batch of cuts of about 10 s at 16 kHz, 8 channels each;
  * "one_30s_8ch": one 30 s cut of 8 channels: what a launch costs when there is next to nothing to move.

Per shape and mode, by HIP events around the call (launch gaps and the staged tables included), the median of --steps timed runs after
--warmup untimed ones, the legs alternating in two passes:

  * downmix / channels   the new launch (float32 output; the channels of a cut lie back to back, with odd lengths at every residue mod 4);
  * baseline_torch       torch on the device: per cut ``x.mean(0)`` of its (C, n) view (downmix) or the view itself (channels) into
                         ``torch.zeros`` by one slice copy per cut;
  * baseline_host        the parent's path from where the samples are on the host: per cut ``audio.mean(dim=0)`` on the CPU (downmix) or
                         the expansion to (C, n), zero padding on the host, one ``.to(device)`` -- by the host clock around a device
                         synchronise, since most of it is host time.  (Without the reading: the samples are in host memory already.)

Bytes: downmix 4 * C * sum(len) read + 4 * B * Tmax written; channels 4 * C * sum(len) read + 4 * B * C * Tmax written; GB/s = bytes / time,
next to the 6.29 TB/s the micro-architecture guide measured for a float4 copy.  Before anything is timed every result is compared with the
torch form: the channels form bit for bit; the downmix against the float64 mean computed on the device, |y - t| <= 0.5 ulp32(t) (1 + 2^-20)
for the launch (correctly rounded) and <= 4 ulp32(t) for torch's float32 mean, which is not one fixed arithmetic.  Prints one JSON line and
writes it to --out (default profiles/collate_channels_bench.json).

    python tools/bench_collate_channels.py [--steps 30] [--warmup 5] [--out profiles/collate_channels_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_collate import COPY_ROOF_TBPS, SR, config5_lengths, median_ms_events, median_ms_host  # noqa: E402

C = 8


def ulp32(t: torch.Tensor) -> torch.Tensor:
    _, e = torch.frexp(t.abs())
    return torch.ldexp(torch.ones_like(t), torch.clamp(e - 24, min=-149))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="timed runs per leg (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collate_channels_bench.json"))
    args = ap.parse_args()
    steps = max(args.steps, 20)
    if not torch.cuda.is_available():
        raise SystemExit("bench_collate_channels.py measures on the GPU: no HIP device is visible")

    from lhotse_amd import augmentation as A

    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    shapes = {"config5_8ch": config5_lengths(rng) | 1, "one_30s_8ch": np.asarray([30 * SR + 1], dtype=np.int64)}
    res = {"tool": "tools/bench_collate_channels.py", "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": args.warmup, "channels": C,
           "timing": "median (min, max) in ms", "copy_roof_TBps": COPY_ROOF_TBPS, "shapes": {}}
    for name, lens in shapes.items():
        B, tmax = len(lens), int(lens.max())
        base = np.zeros(B, dtype=np.int64)
        np.cumsum(((C * lens + 3) & ~3)[:-1], out=base[1:])  # a cut's channels back to back from a 16-byte boundary
        src = (base[:, None] + np.arange(C)[None, :] * lens[:, None]).reshape(-1)
        total = int(base[-1] + C * lens[-1]) + 8
        host = ((torch.randint(-32768, 32768, (total,), dtype=torch.int32).float()) / 32768.0).contiguous()  # PCM-derived, as decoded int16
        arena = host.to(dev)
        r = res["shapes"][name] = {"cuts": B, "Tmax": tmax, "samples_per_channel": int(lens.sum()), "padding_share": round(1 - float(lens.sum()) / (B * tmax), 4)}
        views = [arena[b : b + C * n].view(C, n) for b, n in zip(base.tolist(), lens.tolist())]
        host_views = [host[b : b + C * n].view(C, n) for b, n in zip(base.tolist(), lens.tolist())]
        first_mean = np.arange(B + 1, dtype=np.int64) * C
        first_chan = np.arange(B * C + 1, dtype=np.int64)
        out_mean = torch.empty((B, tmax), dtype=torch.float32, device=dev)
        out_chan = torch.empty((B * C, tmax), dtype=torch.float32, device=dev)

        def downmix():
            return A.collate_sources_in_arena(arena, first_mean, src, lens, row_len=tmax, out=out_mean)[0]

        def channels():
            return A.collate_sources_in_arena(arena, first_chan, src, np.repeat(lens, C), row_len=tmax, out=out_chan)[0].view(B, C, tmax)

        def torch_downmix():
            o = torch.zeros((B, tmax), dtype=torch.float32, device=dev)
            for i, x in enumerate(views):
                o[i, : x.shape[1]] = x.mean(0)
            return o

        def torch_channels():
            o = torch.zeros((B, C, tmax), dtype=torch.float32, device=dev)
            for i, x in enumerate(views):
                o[i, :, : x.shape[1]] = x
            return o

        def host_downmix():
            o = torch.zeros((B, tmax), dtype=torch.float32)
            for i, x in enumerate(host_views):
                o[i, : x.shape[1]] = x.mean(dim=0)
            return o.to(dev)

        def host_channels():
            o = torch.zeros((B, C, tmax), dtype=torch.float32)
            for i, x in enumerate(host_views):
                o[i, :, : x.shape[1]] = x
            return o.to(dev)

        # faster and different is not faster
        assert torch.equal(channels().view(torch.int32), torch_channels().view(torch.int32)) and torch.equal(host_channels(), torch_channels()), name
        truth = torch.zeros((B, tmax), dtype=torch.float64, device=dev)
        for i, x in enumerate(views):
            truth[i, : x.shape[1]] = x.double().mean(0)  # (PCM samples: the float64 sum is exact, the mean rounded once)
        u = ulp32(truth)
        ours, theirs, hosts = ((y.double() - truth).abs() / u for y in (downmix(), torch_downmix(), host_downmix()))
        assert float(ours.max()) <= 0.5 * (1 + 2.0 ** -20) and float(theirs.max()) <= 4.0 and float(hosts.max()) <= 4.0, (name, float(ours.max()), float(theirs.max()))
        r["downmix_error_ulp32"] = {"launch": round(float(ours.max()), 6), "torch_device_mean": round(float(theirs.max()), 6), "torch_host_mean": round(float(hosts.max()), 6)}
        for mode, legs_of, nbytes in (("downmix", (("downmix", downmix, median_ms_events), ("baseline_torch", torch_downmix, median_ms_events),
                                                   ("baseline_host", host_downmix, median_ms_host)), 4 * C * int(lens.sum()) + 4 * B * tmax),
                                      ("channels", (("channels", channels, median_ms_events), ("baseline_torch", torch_channels, median_ms_events),
                                                    ("baseline_host", host_channels, median_ms_host)), 4 * C * int(lens.sum()) + 4 * B * C * tmax)):
            legs = r[mode] = {"algorithmic_MB": round(nbytes / 1e6, 3)}
            for _ in range(2):  # alternate the legs: two passes, the second one is reported next to the first
                for leg, fn, timer in legs_of:
                    med, lo, hi = timer(fn, steps if leg != "baseline_host" else 20, args.warmup)
                    legs.setdefault(leg, []).append({"ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4), "GBps": round(nbytes / med / 1e6, 1),
                                                     "of_copy_roof": round(nbytes / med / 1e6 / (COPY_ROOF_TBPS * 1e3), 4)})
            legs["launch_over_baseline_torch"] = round(legs[mode][-1]["ms"] / legs["baseline_torch"][-1]["ms"], 3)
            legs["launch_over_baseline_host"] = round(legs[mode][-1]["ms"] / legs["baseline_host"][-1]["ms"], 4)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
