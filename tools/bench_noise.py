"""noise_on_device / HipRandomizedSmoothing against the reference's op sequence and a plain copy on the same device.

    python tools/bench_noise.py [--out profiles/noise_bench.json] [--repeats 30] [--rows 10000]

Cases: the 600 s mini-batch (48 x 12.5 s at 16 kHz, float32) and a large batch of `rows` x 10 s, float32 and bfloat16.  Legs, one call
of each in turn per repeat after 3 warm-up turns, timed with HIP events around `inner` calls (enough of them that a timing covers at
least ~1 GB of traffic) and reported per call as medians:
  kernel             noise_on_device into a preallocated output, every row noisy, rows on 16-byte boundaries
  kernel_in_place    the same with out=x
  kernel_unaligned   the same batch one element off the 16-byte boundary: every group straddles one Philox counter more
  kernel_p0.3        the sigma table of RandomizedSmoothing's defaults: 70 % of the rows masked (they make no Philox call)
  module             HipRandomizedSmoothing()(x): host draws, the table's copy, the launch, a fresh output
  torch_ops          the reference's sequence as torch ops on the device: randn_like, sigma *, mask *, +, clip
  copy               out.copy_(x): one read and one write of the same bytes
GB/s counts one read and one write of the batch.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lhotse_amd as LA  # noqa: E402


def timed_alternating(legs, repeats, inner):
    times = {name: [] for name in legs}
    for i in range(3 + repeats):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            if i >= 3:
                times[name].append(a.elapsed_time(b) / inner)
    return {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "repeats": repeats, "calls_per_timing": inner} for name, t in times.items()}


def torch_ops(audio, sigma, mask):
    noise = sigma * torch.randn_like(audio)
    noise = noise * mask
    return torch.clip(audio + noise, min=-1.0, max=1.0)


def case(rows, cols, dtype, repeats):
    g = torch.Generator(device="cuda").manual_seed(rows)
    wide = torch.empty(rows * cols + 8, dtype=dtype, device="cuda")
    x = wide[: rows * cols].view(rows, cols)
    x.copy_((torch.rand(rows, cols, device="cuda", generator=g) - 0.5).to(dtype))
    off = wide[1 : rows * cols + 1].view(rows, cols)
    out, out_off = torch.empty_like(x), torch.empty_like(wide)[1 : rows * cols + 1].view(rows, cols)
    sigma = torch.full((rows,), 0.1, device="cuda")
    table = sigma * (2 * torch.rand(rows, device="cuda", generator=g) - 1) * (torch.rand(rows, device="cuda", generator=g) > 0.7)
    col, mask = sigma[:, None].to(dtype), torch.ones(rows, 1, dtype=dtype, device="cuda")
    module = LA.HipRandomizedSmoothing(seed=1)
    nbytes = 2 * rows * cols * x.element_size()
    legs = {
        "kernel": lambda: LA.noise_on_device(x, sigma, seed=1, out=out),
        "kernel_in_place": lambda: LA.noise_on_device(x, sigma, seed=1, out=x),
        "kernel_unaligned": lambda: LA.noise_on_device(off, sigma, seed=1, out=out_off),
        "kernel_p0.3": lambda: LA.noise_on_device(x, table, seed=1, out=out),
        "module": lambda: module(x),
        "torch_ops": lambda: torch_ops(x, col, mask),
        "copy": lambda: out.copy_(x),
    }
    r = timed_alternating(legs, repeats, max(1, int(1e9 // nbytes)))
    for leg in r.values():
        leg["GB_per_s"] = nbytes / leg["median_ms"] / 1e6
    r["shape"], r["dtype"], r["bytes_read_plus_written"] = [rows, cols], str(dtype), nbytes
    r["kernel_over_copy"] = r["kernel"]["median_ms"] / r["copy"]["median_ms"]
    r["unaligned_over_kernel"] = r["kernel_unaligned"]["median_ms"] / r["kernel"]["median_ms"]
    r["speedup_kernel_vs_torch_ops"] = r["torch_ops"]["median_ms"] / r["kernel"]["median_ms"]
    r["speedup_module_vs_torch_ops"] = r["torch_ops"]["median_ms"] / r["module"]["median_ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/noise_bench.json")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--rows", type=int, default=10000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_noise needs a GPU"
    result = {"device": torch.cuda.get_device_name(0)}
    for name, (rows, cols, dtype) in {
        "minibatch_48x12.5s_float32": (48, 200000, torch.float32),
        f"batch_{args.rows}x10s_float32": (args.rows, 160000, torch.float32),
        f"batch_{args.rows}x10s_bfloat16": (args.rows, 160000, torch.bfloat16),
    }.items():
        result[name] = case(rows, cols, dtype, args.repeats)
        torch.cuda.empty_cache()
        print(name, json.dumps(result[name]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
