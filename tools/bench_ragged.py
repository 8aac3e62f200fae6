#!/usr/bin/env python3
"""``layer(x, lengths)`` on a ragged mini-batch against the two routes there were before it, forward and forward + backward, for
``HipWav2LogFilterBank`` and ``HipWav2FFT`` (16 kHz, the layers' defaults).

The mini-batch is one of bench.py's config 5: cuts of uniform(1, 30) s drawn with seed 0 until 600 s are full, zero-padded to one
``(B, Smax)`` float32 tensor.  Legs:

  * "ragged":  one call ``layer(x, lengths)``: every row framed as the cut alone, padding rows written by the same launch(es);
  * "loop":    one uniform call per cut, ``layer(x[b:b+1, :len_b])`` -- the only correct route without ``lengths``: B forward launches and
               2 B backward launches;
  * "padded":  the uniform call on the padded tensor -- wrong at every shorter cut's last frames and over the padding, but the speed floor.

Legs alternate: every round times each leg once, by HIP events around the calls on the current stream, allocations included; the figures
are the medians (min, max) of --steps rounds after --warmup untimed ones.  The backward runs under fixed cotangents (``padded`` gets the
ragged call's, ``loop`` each cut's own rows of them).  Before anything is timed the ragged outputs and gradients are compared with the
loop's bit for bit.  No time is a pass / fail bar.  Prints one JSON line and writes it to --out.

    python tools/bench_ragged.py [--steps 30] [--warmup 5] [--out profiles/ragged_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 16000


def config5_lengths(seed=0):
    rng = np.random.RandomState(seed)
    lens, tot = [], 0.0
    while True:
        d = rng.uniform(1.0, 30.0)
        if tot + d > 600.0:
            return lens
        lens.append(int(d * SR))
        tot += d


def real(t):
    return torch.view_as_real(t) if t.is_complex() else t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="timed rounds (at least 10)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_bench.json"))
    args = ap.parse_args()
    steps = max(args.steps, 10)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged.py measures on the GPU: no HIP device is visible")

    import lhotse_amd as LA

    lens = config5_lengths()
    B, smax = len(lens), max(lens)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((B, smax), device="cuda", generator=gen) - 0.5
    for b, s in enumerate(lens):
        x[b, s:] = 0.0
    res = {"tool": "tools/bench_ragged.py", "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": args.warmup,
           "timing": "median (min, max) in ms, HIP events, legs alternating", "batch": B, "max_samples": smax, "seconds": round(sum(lens) / SR, 2),
           "padded_seconds": round(B * smax / SR, 2), "layers": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def once(fn):
        torch.cuda.synchronize()
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        del out
        return ev[0].elapsed_time(ev[1])

    for name in ("HipWav2LogFilterBank", "HipWav2FFT"):
        layer = getattr(LA, name)().differentiable_()
        with torch.no_grad():
            out, out_lens = layer(x, lens)
        T = out_lens.tolist()
        cot = torch.randn(real(out).shape, device="cuda", generator=gen)
        cot = torch.view_as_complex(cot) if out.is_complex() else cot
        cots = [cot[b: b + 1, :t].contiguous() for b, t in enumerate(T)]
        rows = [x[b: b + 1, :s] for b, s in enumerate(lens)]

        def ragged(backward):
            if not backward:
                with torch.no_grad():
                    return layer(x, lens)[0]
            xg = x.detach().requires_grad_(True)
            torch.autograd.backward(layer(xg, lens)[0], cot)
            return xg.grad

        def loop(backward):
            if not backward:
                with torch.no_grad():
                    return [layer(r) for r in rows]
            grads = []
            for r, c in zip(rows, cots):
                rg = r.detach().requires_grad_(True)
                torch.autograd.backward(layer(rg), c)
                grads.append(rg.grad)
            return grads

        def padded(backward):
            if not backward:
                with torch.no_grad():
                    return layer(x)
            xg = x.detach().requires_grad_(True)
            torch.autograd.backward(layer(xg), cot)
            return xg.grad

        # parity first: the ragged call is the loop, bit for bit
        alone, galone, gragged = loop(False), loop(True), ragged(True)
        same = all(torch.equal(real(out[b, :t]), real(alone[b][0])) and torch.equal(gragged[b, :s], galone[b][0]) for b, (s, t) in enumerate(zip(lens, T)))
        assert same, f"{name}: the ragged call differs from the per-cut calls"
        assert tuple(padded(False).shape) == tuple(out.shape)
        entry = {"frames": int(sum(T)), "padded_frames": B * max(T), "bit_equal_to_loop": bool(same)}
        for what, backward in (("forward", False), ("forward_backward", True)):
            legs = {"ragged": lambda: ragged(backward), "loop": lambda: loop(backward), "padded": lambda: padded(backward)}
            ms = {k: [] for k in legs}
            for i in range(steps + args.warmup):
                for k, fn in legs.items():
                    t = once(fn)
                    if i >= args.warmup:
                        ms[k].append(t)
            part = {k: {"ms": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)} for k, v in ms.items()}
            part["loop_over_ragged"] = round(part["loop"]["ms"] / part["ragged"]["ms"], 3)
            part["ragged_over_padded"] = round(part["ragged"]["ms"] / part["padded"]["ms"], 3)
            entry[what] = part
        res["layers"][name] = entry
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
