#!/usr/bin/env python3
"""``HipWav2Win`` / ``HipWav2FFT`` (one hipfeat_stft_run launch each) against the reference's own call sequence run as torch ops on the
same device (``Wav2Win._forward_strided`` layers.py:151-187 and ``Wav2FFT._forward_strided`` layers.py:309-320, as restated by
tests/_stft_ref.py::ref32_tensors: as_strided view of the reflected row, mean, subtract, pad, multiply, zero pad, ``torch.fft.rfft``).

Shapes, 16 kHz, 25 / 10 ms, povey, pre-emphasis 0.97, DC removal, energy in bin 0 (the layers' defaults):

  * "headline":  the BASELINE headline batch of bench.py, --cuts (default 10000) x 10 s cuts as one (C, 160000) float32 tensor.  The torch
    leg runs it in pieces of 1000 cuts (its intermediates, several times the output, do not fit otherwise); its time is the sum.
  * "minibatch": one 600 s mini-batch, (60, 160000).

Legs: the median (min, max) of --steps timed calls after --warmup untimed ones, by HIP events around the call on the current stream, output
allocation included (the caching allocator serves it from the second call on).  ``bytes`` is what the algorithm has to move: every
sample read once and every output float written once; GB/s = bytes / median time, a whole-call rate, not a kernel's share of peak.
Before anything is timed the device output of the mini-batch's first cut is held to ref32 and the float64 truth (the bars of
tests/_stft_ref.py): faster and different is not faster.  Prints one JSON line and writes it to --out.

    python tools/bench_stft.py [--steps 30] [--warmup 5] [--cuts 10000] [--out profiles/stft_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SAMPLES_PER_CUT, N, FFT, SHIFT = 160000, 400, 512, 160
TORCH_PIECE = 1000


def timed(fn, steps, warmup):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(steps + warmup):
        torch.cuda.synchronize()
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        del out
        if i >= warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    return {"ms": round(float(np.median(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="timed calls per leg (at least 10)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cuts", type=int, default=10000, help="cuts of the headline batch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stft_bench.json"))
    args = ap.parse_args()
    steps = max(args.steps, 10)
    if not torch.cuda.is_available():
        raise SystemExit("bench_stft.py measures on the GPU: no HIP device is visible")

    import _stft_ref as R

    import lhotse_amd as LA

    cfg = R.config(16000)
    win, stft = LA.HipWav2Win(pad_length=FFT, return_log_energy=True), LA.HipWav2FFT()
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {"tool": "tools/bench_stft.py", "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": args.warmup, "timing": "median (min, max) in ms, HIP events",
           "config": "16 kHz, N 400, shift 160, fft 512, povey, preemph 0.97, DC removal, raw log-energy", "torch_piece_cuts": TORCH_PIECE, "shapes": {}}

    # parity first, on the mini-batch's first cut
    x0 = 0.1 * torch.randn((1, SAMPLES_PER_CUT), device="cuda", generator=gen) + 0.02
    x0n = x0.cpu().numpy()
    r_frames, _, r_spec = R.ref32(x0n, cfg)
    t_frames, t_log_e, t_spec = R.truth(x0n, cfg)
    frames, log_e = win(x0)
    ey, er = R.hold("bench frames", frames.cpu().numpy(), r_frames, t_frames)
    R.hold_energy("bench log-energy", log_e.cpu().numpy(), t_log_e)
    sy, sr = R.hold("bench spectrum", stft(x0).cpu().numpy(), r_spec, t_spec, energy_bin=True)
    res["parity"] = {"frames": {"E_device": ey, "E_ref32": er}, "spectrum": {"E_device": sy, "E_ref32": sr}}

    for name, cuts in (("minibatch", 60), ("headline", args.cuts)):
        x = 0.1 * torch.randn((cuts, SAMPLES_PER_CUT), device="cuda", generator=gen) + 0.02
        T = (SAMPLES_PER_CUT + SHIFT // 2) // SHIFT
        pieces = list(x.split(TORCH_PIECE))
        shape = res["shapes"][name] = {"cuts": cuts, "samples_per_cut": SAMPLES_PER_CUT, "frames": cuts * T, "legs": {}}
        for leg, ours, spectrum, out_floats in (("Wav2Win", lambda: win(x), False, FFT + 1), ("Wav2FFT", lambda: stft(x), True, FFT + 2)):
            nbytes = 4 * (cuts * SAMPLES_PER_CUT + cuts * T * out_floats)

            def torch_ops():
                out = None
                for p in pieces:  # (one piece's result is alive at a time)
                    out = R.ref32_tensors(p, cfg, FFT, spectrum=spectrum)
                return out

            mine, ref = timed(ours, steps, args.warmup), timed(torch_ops, steps, args.warmup)
            shape["legs"][leg] = {"bytes": nbytes, "device_layer": {**mine, "GB_per_s": round(nbytes / mine["ms"] / 1e6, 1)}, "torch_ops_on_device": ref,
                                  "speedup": round(ref["ms"] / mine["ms"], 2)}
        del x, pieces
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
