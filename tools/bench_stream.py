#!/usr/bin/env python3
"""``online_inference`` of ``HipWav2LogFilterBank`` / ``HipWav2FFT`` (one hipfeat_stream_run launch per chunk) against the reference's own
streaming call sequence run as torch ops on the same device: ``torch.cat((remainder, chunk))``, ``as_strided`` (layers.py:834-856),
``Wav2Win._forward_strided`` (:151-187: mean, subtract, log-energy, replicate pad, pre-emphasis, window, zero pad), ``torch.fft.rfft`` and the
epilogue (:309-320 bin 0 = log-energy; :565-578 |X|^2, mel matmul, max, log), with the window and the filterbank resident on the device.

Shape: 64 concurrent streams at 16 kHz (25 / 10 ms, povey, pre-emphasis 0.97, DC removal: the layers' defaults), chunks of 160 ms (2560
samples, 16 frames per stream) and of 1 s (16000 samples, 100 frames), each call continuing a stream (its context is the remainder of a
previous call of the same chunk length).  What a streaming front end pays per chunk is the latency of the call, so the figure is the time
of ONE call: the median (min, max) of --steps timed calls after --warmup untimed ones, by HIP events around the call on the current stream,
output allocation included.  A call of this size is dominated by launch and allocator overhead: that is what is being compared (about 14
launches against one), not a kernel's share of peak.  The two legs alternate, call by call, inside one timed loop.  Before anything is
timed the device outputs of the first two streams are held to the float64 oracle on V (the bars of tests/_stream_ref.py) and the torch
leg's remainder to the device's: faster and different is not faster.  Prints one JSON line and writes it to --out.

    python tools/bench_stream.py [--steps 30] [--warmup 5] [--streams 64] [--out profiles/stream_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RATE, N, SHIFT, FFT = 16000, 400, 160, 512


def timed_pair(a, b, steps, warmup):
    """Alternates the two legs call by call; per leg the median (min, max) of the timed calls, in ms."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = ([], [])
    for i in range(steps + warmup):
        for k, fn in enumerate((a, b)):
            torch.cuda.synchronize()
            ev[0].record()
            out = fn()
            ev[1].record()
            torch.cuda.synchronize()
            del out
            if i >= warmup:
                ms[k].append(ev[0].elapsed_time(ev[1]))
    return [{"ms": round(float(np.median(m)), 4), "min": round(float(np.min(m)), 4), "max": round(float(np.max(m)), 4)} for m in ms]


def torch_stream_ops(context, x, window, fb, eps, log_floor, fbank):
    """The reference's online_inference as torch ops -> (output, remainder)."""
    V = torch.cat((context, x), dim=1)
    B, L = V.shape
    T = (L - (N - SHIFT)) // SHIFT
    remainder = V[:, T * SHIFT:]
    xs = V.as_strided([B, T, N], (V.stride(0), SHIFT * V.stride(1), V.stride(1)))
    xs = xs - torch.mean(xs, dim=2, keepdim=True)
    log_e = None
    if not fbank:  # Wav2FFT(use_energy=True): the raw log-energy goes to bin 0
        log_e = torch.max((xs.pow(2).sum(-1) + 1e-15).log(), log_floor)
    off = torch.nn.functional.pad(xs, (1, 0), mode="replicate")
    xs = xs - 0.97 * off[:, :, :-1]
    xs = xs * window
    xs = torch.nn.functional.pad(xs.unsqueeze(1), [0, FFT - N], mode="constant", value=0.0).squeeze(1)
    X = torch.fft.rfft(xs, dim=-1)
    if not fbank:
        X[:, :, 0] = log_e
        return X, remainder
    mel = torch.matmul(X.abs().pow(2), fb)
    return torch.max(mel, eps).log(), remainder


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="timed calls per leg (at least 10)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.json"))
    args = ap.parse_args()
    steps = max(args.steps, 10)
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream.py measures on the GPU: no HIP device is visible")

    import _stft_ref as R
    import _stream_ref as SR
    from oracle.kaldi_torch import TorchKaldi

    import lhotse_amd as LA

    fbank, stft = LA.HipWav2LogFilterBank(), LA.HipWav2FFT()
    fb_cfg, _ = SR.feature_config(fbank)
    fft_cfg = R.config(RATE)
    tk = TorchKaldi(fb_cfg)
    window, fb, eps = tk.window.cuda(), tk.fb.cuda(), tk.eps.cuda()
    log_floor = torch.tensor(float(np.log(fft_cfg.energy_floor)), device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    B = args.streams
    res = {"tool": "tools/bench_stream.py", "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": args.warmup, "streams": B,
           "timing": "median (min, max) in ms of one call, HIP events, the two legs alternating",
           "config": "16 kHz, N 400, shift 160, fft 512, povey, preemph 0.97, DC removal; fbank: 80 filters; FFT: raw log-energy in bin 0", "chunks": {}}

    for label, S in (("160ms", 2560), ("1s", 16000)):
        x = 0.1 * torch.randn((B, S), device="cuda", generator=gen) + 0.02
        prev = 0.1 * torch.randn((B, S), device="cuda", generator=gen) + 0.02
        _, context = stft.online_inference(prev)  # what a stream of this chunk length hands on
        V = np.concatenate([context.cpu().numpy(), x.cpu().numpy()], axis=1)[:2]
        T, remainder = SR.split(V, N, SHIFT)
        entry = res["chunks"][label] = {"chunk_samples": S, "context_samples": int(context.shape[1]), "frames_per_stream": T, "legs": {}}
        # parity first, on the first two streams
        y, rem = stft.online_inference(x, context)
        ey, er = R.hold(f"bench {label} spectrum", y[:2].cpu().numpy(), SR.ref32(V, fft_cfg)[2], SR.truth(V, fft_cfg)[2], energy_bin=True)
        f, rem_f = fbank.online_inference(x, context)
        want = SR.features_truth(V, fb_cfg)
        for b in range(2):
            SR.hold_features("fbank", False, f[b].cpu().numpy().astype(np.float64), want[b])
        t_spec, t_rem = torch_stream_ops(context, x, window, fb, eps, log_floor, False)
        t_mel, _ = torch_stream_ops(context, x, window, fb, eps, log_floor, True)
        assert torch.equal(rem, t_rem) and torch.equal(rem_f, t_rem) and np.array_equal(rem[:2].cpu().numpy(), remainder)
        assert t_spec.shape == y.shape and t_mel.shape == f.shape
        entry["parity"] = {"spectrum": {"E_device": ey, "E_ref32": er}, "fbank_max_abs_vs_torch_ops": float((f - t_mel).abs().max())}
        for leg, layer, is_fbank, width in (("Wav2LogFilterBank", fbank, True, 80), ("Wav2FFT", stft, False, FFT + 2)):
            mine, ref = timed_pair(lambda: layer.online_inference(x, context), lambda: torch_stream_ops(context, x, window, fb, eps, log_floor, is_fbank),
                                   steps, args.warmup)
            nbytes = 4 * (B * (S + int(context.shape[1])) + B * T * width + B * int(rem.shape[1]))
            entry["legs"][leg] = {"bytes": nbytes, "device_layer": mine, "torch_ops_on_device": ref, "speedup": round(ref["ms"] / mine["ms"], 2)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
