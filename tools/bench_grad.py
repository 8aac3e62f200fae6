#!/usr/bin/env python3
"""Forward + backward of ``HipWav2LogFilterBank().differentiable_()`` (the feature launch, then ``hipfeat_grad_run``: two launches per piece
of rows) against the same layer written as torch ops with torch's autograd on the same device (tests/_grad_ref.py::forward, which
tests/test_grad_reference.py holds to the live reference's gradient).

Shapes, 16 kHz, 25 / 10 ms, povey, pre-emphasis 0.97, DC removal, 80 filters (the layer's defaults), loss = mean((y - target)^2):

  * "minibatch": the headline batch's 600 s mini-batch, 48 cuts of 12.5 s, one (48, 200000) float32 tensor;
  * "seconds":   64 x 1 s, (64, 16000).

Legs alternate (ours, torch, ours with a second workspace budget, ...): every round times each leg once, by HIP events around forward +
backward on the current stream, allocations included; the figures are the medians (min, max) of --steps rounds after --warmup untimed
ones.  ``workspace_bytes`` is what the frames launch writes and the gather reads once more: rows x T x Nr x 4; ``pieces`` the launch
pairs.  Before anything is timed the device gradient of two rows under a fixed cotangent is held to the restatement's float64 autograd (the bar
of tests/_grad_ref.py): faster and different is not faster.  No time is a pass / fail bar.  Prints one JSON line and writes it to --out.

    python tools/bench_grad.py [--steps 30] [--warmup 5] [--second-budget-mib 16] [--out profiles/grad_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N, SHIFT, M = 400, 160, 80
SHAPES = {"minibatch": (48, 200000), "seconds": (64, 16000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="timed rounds (at least 10)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--second-budget-mib", type=int, default=16, help="the workspace budget of the third leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_bench.json"))
    args = ap.parse_args()
    steps = max(args.steps, 10)
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad.py measures on the GPU: no HIP device is visible")

    import _grad_ref as GR

    import lhotse_amd as LA
    from lhotse_amd import layers as LY

    layer = LA.HipWav2LogFilterBank().differentiable_()
    default_budget = LY._GRAD_WORKSPACE_BYTES
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {"tool": "tools/bench_grad.py", "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": args.warmup,
           "timing": "median (min, max) in ms of forward + backward, HIP events, legs alternating",
           "config": "16 kHz, N 400, shift 160, fft 512, povey, preemph 0.97, DC removal, 80 filters; loss mean((y - target)^2)", "shapes": {}}

    def ours(x, target, budget):
        LY._GRAD_WORKSPACE_BYTES = budget
        x = x.detach().requires_grad_(True)
        ((layer(x) - target) ** 2).mean().backward()
        return x.grad

    def theirs(x, target):
        x = x.detach().requires_grad_(True)
        ((GR.forward("Wav2LogFilterBank", {}, x) - target) ** 2).mean().backward()
        return x.grad

    # parity first: two rows of the one-second shape under one fixed random cotangent (the residual of the timed loss), against the
    # restatement's autograd in float32 and float64, as the tests do.  (Through the loss itself the cotangent 2 (y - t) / n carries the
    # float32 error of whichever forward computed y, which the conditioning of 1 / mel then multiplies: that compares forwards.)
    x0 = (torch.rand((2, 16000), device="cuda", generator=gen) - 0.5).cpu().numpy()
    with torch.no_grad():
        shape0 = layer(torch.from_numpy(x0).cuda()).shape
    c0 = [(2.0 / int(np.prod(shape0)) * torch.randn(shape0, device="cuda", generator=gen)).cpu().numpy()]
    worst = GR.hold("bench gradient", GR.device_gradient(layer, x0, c0), GR.gradient("Wav2LogFilterBank", {}, x0, c0, torch.float32),
                    GR.gradient("Wav2LogFilterBank", {}, x0, c0, torch.float64))
    res["parity"] = {"worst_ratio_to_torch_float32": worst}

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def once(fn):
        torch.cuda.synchronize()
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        del out
        return ev[0].elapsed_time(ev[1])

    for name, (B, S) in SHAPES.items():
        x = torch.rand((B, S), device="cuda", generator=gen) - 0.5
        with torch.no_grad():
            target = layer(x)
            target += torch.randn(target.shape, device="cuda", generator=gen)
        T = int(target.shape[1])
        row_bytes = T * N * 4
        second = args.second_budget_mib << 20
        legs = {"ours": lambda: ours(x, target, default_budget), "torch": lambda: theirs(x, target), "ours_second_budget": lambda: ours(x, target, second)}
        ms = {k: [] for k in legs}
        for i in range(steps + args.warmup):
            for k, fn in legs.items():
                t = once(fn)
                if i >= args.warmup:
                    ms[k].append(t)
        shape = {"batch": B, "samples": S, "frames": T, "workspace_bytes": B * row_bytes, "output_bytes": B * T * M * 4, "waveform_bytes": B * S * 4}
        for k, v in ms.items():
            shape[k] = {"ms": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}
        for k, budget in (("ours", default_budget), ("ours_second_budget", second)):
            rows = max(1, min(B, budget // row_bytes))
            shape[k].update(budget_bytes=budget, rows_per_piece=rows, pieces=-(-B // rows))
        shape["torch_over_ours"] = round(shape["torch"]["ms"] / shape["ours"]["ms"], 3)
        shape["second_budget_over_default"] = round(shape["ours_second_budget"]["ms"] / shape["ours"]["ms"], 3)
        res["shapes"][name] = shape
    LY._GRAD_WORKSPACE_BYTES = default_budget
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
