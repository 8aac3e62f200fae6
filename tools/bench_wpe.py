"""HipDereverbWPE against the reference's call sequence on the same device.

    python tools/bench_wpe.py [--out profiles/wpe_bench.json] [--repeats 30]

Two mini-batches of 600 s of 16 kHz audio (seeded noise through a decaying tail): 48 mono cuts of 10-15 s, padded to the longest as the
collation does, and 48 six-channel cuts of 12.5 s (600 s of six-channel audio).  Timed with HIP events around the whole call (stft + kernel + istft), the median of
`repeats` calls after 3 warm-up calls, and around the kernel launch alone with pass 2 on float64 FMAs and on the float64 matrix
instruction (HIPFEAT_WPE_UPDATE = fma | mfma; without it the library picks by K).  The baseline is what DereverbWPE runs per example -- the
algorithm of csrc/kernel_wpe.hpp as torch complex64 operations (matmul, linalg.solve), one example after the other -- on the same
device.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lhotse_amd as LA  # noqa: E402


def wpe_torch(Y, taps=10, delay=3, iterations=3):
    """wpe_v6(psd_context=0, statistics_mode='full') for one example, Y: (F, D, T) complex64 on the device."""
    T = Y.shape[-1]
    rows = []
    for tau in range(taps):
        z = torch.zeros_like(Y)
        z[..., delay + tau:] = Y[..., : T - delay - tau]
        rows.append(z)
    Yt = torch.cat(rows, -2)
    X = Y
    for _ in range(iterations):
        p = (X.real**2 + X.imag**2).mean(-2)
        lam = 1.0 / torch.maximum(p, 1e-10 * p.amax(-1, keepdim=True))
        A = Yt * lam[..., None, :]
        G = torch.linalg.solve(A @ Yt.mH, A @ Y.mH)
        X = Y - G.mH @ Yt
    return X


def reference_sequence(audio, n_fft=512, hop=128):
    window = torch.blackman_window(n_fft, device=audio.device)
    outs = []
    for a in (audio[:, None] if audio.ndim == 2 else audio):
        Y = torch.stft(a, n_fft=n_fft, hop_length=hop, return_complex=True, window=window).permute(1, 0, 2)
        outs.append(torch.istft(wpe_torch(Y).permute(1, 0, 2), n_fft=n_fft, hop_length=hop, window=window))
    return torch.cat(outs, 0) if audio.ndim == 2 else torch.stack(outs, 0)


def timed(fn, repeats):
    for _ in range(3):
        fn()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "repeats": repeats}


def batch(shape, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    tail = torch.exp(-torch.arange(4000) / 800.0) * torch.randn(4000, generator=g)
    n = x.shape[-1]
    y = torch.fft.irfft(torch.fft.rfft(x, 2 * n) * torch.fft.rfft(tail, 2 * n), 2 * n)[..., :n]
    for i, length in enumerate(lengths):
        y[i, ..., length:] = 0
    return (y / y.abs().max()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/wpe_bench.json")
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_wpe needs a GPU"
    g = torch.Generator().manual_seed(0)
    mono_len = torch.randint(160000, 240001, (48,), generator=g).tolist()  # 10-15 s, 600 s in expectation
    cases = {"mono_48x10-15s": batch((48, max(mono_len)), mono_len, 1), "six_channel_48x12.5s": batch((48, 6, 200000), [200000] * 48, 2)}
    module, result = LA.HipDereverbWPE(), {"device": torch.cuda.get_device_name(0), "n_fft": 512, "hop_length": 128, "taps": 10, "delay": 3, "iterations": 3}
    for name, audio in cases.items():
        window = torch.blackman_window(512, device="cuda")
        Y = torch.stft(audio.reshape(-1, audio.shape[-1]), n_fft=512, hop_length=128, return_complex=True, window=window)
        D = 1 if audio.ndim == 2 else audio.shape[1]
        got, want = module(audio), reference_sequence(audio)
        result[name] = {
            "audio_shape": list(audio.shape), "audio_seconds": audio.shape[0] * audio.shape[-1] / 16000, "stft_shape": list(Y.shape),
            "module": timed(lambda: module(audio), args.repeats),
            "kernel_launch_only": timed(lambda: LA.wpe_on_device(Y, channels=D), args.repeats),
            "reference_sequence_complex64": timed(lambda: reference_sequence(audio), args.repeats),
            "rel_l2_module_vs_reference_sequence": float((got - want).norm() / want.norm()),
        }
        r = result[name]
        for update in ("fma", "mfma"):
            os.environ["HIPFEAT_WPE_UPDATE"] = update
            r["kernel_launch_only_" + update] = timed(lambda: LA.wpe_on_device(Y, channels=D), args.repeats)
        del os.environ["HIPFEAT_WPE_UPDATE"]
        r["speedup_module_vs_reference_sequence"] = r["reference_sequence_complex64"]["median_ms"] / r["module"]["median_ms"]
        print(name, json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
