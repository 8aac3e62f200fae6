"""narrowband_on_device (one fused launch) against the unfused device chain on the same batch.

    python tools/bench_narrowband.py [--out profiles/narrowband_bench.json] [--repeats 30] [--rows 1000] [--rate 16000]

Case: `rows` cuts of 10 s at `rate`, float32, restore_orig_sr=True.  Legs, one call of each in turn per repeat after 3 warm-up turns,
timed with HIP events around `inner` calls (enough that a timing covers at least ~1 GB of traffic) and reported per call as medians:
  fused      narrowband_on_device into a preallocated output
  unfused    the device chain that existed: get_or_create_resampler(rate, 8000) -- the dense-bank or the bankless kernel, whichever
             resample_route picks for the pair --, MuLawEncoding / MuLawDecoding as torch ops on the 8 kHz rows,
             get_or_create_resampler(8000, rate), cut to T: two launches, about ten elementwise kernels, the 8 kHz signal through
             device memory, fresh tensors as the transform would return them
  copy       out.copy_(x): one read and one write of the same bytes
GB/s counts the 8 bytes per sample the fused kernel must move (one read, one write).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lhotse_amd as LA  # noqa: E402
from bench_noise import timed_alternating  # noqa: E402  (tools/ is the script's own directory)

MU = 255.0


def mulaw(d):
    mu = torch.tensor(MU, dtype=d.dtype, device=d.device)
    c = ((torch.sign(d) * torch.log1p(mu * torch.abs(d)) / torch.log1p(mu) + 1) / 2 * mu + 0.5).to(torch.int64)
    v = c.to(d.dtype) / mu * 2 - 1.0
    return torch.sign(v) * (torch.exp(torch.abs(v) * torch.log1p(mu)) - 1.0) / mu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/narrowband_bench.json")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--rate", type=int, default=16000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_narrowband needs a GPU"
    rows, rate, T = args.rows, args.rate, 10 * args.rate
    x = 0.1 * torch.randn(rows, T, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    out = torch.empty_like(x)
    down, up = LA.get_or_create_resampler(rate, 8000, "cuda"), LA.get_or_create_resampler(8000, rate, "cuda")

    def unfused():
        return up(mulaw(down(x)))[:, :T]

    nbytes = 2 * rows * T * 4
    legs = {"fused": lambda: LA.narrowband_on_device(x, rate, out=out), "unfused": unfused, "copy": lambda: out.copy_(x)}
    r = timed_alternating(legs, args.repeats, max(1, int(1e9 // nbytes)))
    for leg in r.values():
        leg["GB_per_s"] = nbytes / leg["median_ms"] / 1e6
    diff = (LA.narrowband_on_device(x, rate, out=out) - unfused()).abs()  # (a code may flip between the two float32 chains)
    r["max_abs_fused_minus_unfused"] = float(diff.max())
    r["share_of_samples_that_differ_by_more_than_4e-6"] = float((diff > 4e-6).float().mean())
    r["unfused_kernels"] = [down.kernel_name, up.kernel_name]
    r["shape"], r["rate"], r["bytes_read_plus_written"] = [rows, T], rate, nbytes
    r["speedup_fused_vs_unfused"] = r["unfused"]["median_ms"] / r["fused"]["median_ms"]
    r["fused_over_copy"] = r["fused"]["median_ms"] / r["copy"]["median_ms"]
    result = {"device": torch.cuda.get_device_name(0), f"batch_{rows}x10s_{rate}Hz": r}
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
