"""HipDereverbWPE against the reference's call sequence on the same device.

    python tools/bench_wpe.py [--out profiles/wpe_bench.json] [--repeats 30]

Two mini-batches of 600 s of 16 kHz audio (seeded noise through a decaying tail): 48 mono cuts of 10-15 s, padded to the longest as the
collation does, and 48 six-channel cuts of 12.5 s (600 s of six-channel audio).  Timed with HIP events around the whole call (stft + kernel + istft), the median of
`repeats` calls after 3 warm-up calls, and around the kernel launch alone with pass 2 on float64 FMAs and on the float64 matrix
instruction (HIPFEAT_WPE_UPDATE = fma | mfma; without it the library picks by K).  The baseline is what DereverbWPE runs per example -- the
algorithm of csrc/kernel_wpe.hpp as torch complex64 operations (matmul, linalg.solve), one example after the other -- on the same
device.  The ragged leg (`ragged_leg`) times HipDereverbWPE(audio, lengths=) -- three HIP launches, samples to samples -- against a loop
of per-cut calls and against the padded call, its three launches one by one, and both memory layouts of the spectra; its legs alternate.
Needs a GPU; there is no fallback."""
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


def timed_alternating(legs, repeats):
    """legs: name -> callable.  One call of each in turn per repeat, after 3 warm-up turns: the legs see the same machine state."""
    times = {name: [] for name in legs}
    for i in range(3 + repeats):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= 3:
                times[name].append(a.elapsed_time(b))
    return {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "repeats": repeats} for name, t in times.items()}


def ragged_leg(module, audio, lengths, repeats):
    """HipDereverbWPE(audio, lengths=) against the two things a user could do before it: a loop of per-cut calls (correct) and the padded
    call (wrong at the row ends; the speed floor).  Then the three launches of the ragged call one by one, with the spectra laid out bin-major
    ((F, frames)-contiguous per row: what is kept) and frame-major (torch.stft's layout)."""
    S = LA.signal_transforms
    a3 = audio if audio.ndim == 3 else audio[:, None]
    D, lens, window = a3.shape[1], torch.tensor(lengths), torch.blackman_window(512, device="cuda")
    lens_dev, frames_max = lens.to("cuda", torch.int32), 1 + max(lengths) // 128
    legs = {
        "ragged_call": lambda: module(audio, lengths=lens),
        "per_cut_loop": lambda: [module(audio[b : b + 1, ..., :n]) for b, n in enumerate(lengths)],
        "padded_call": lambda: module(audio),
    }
    for tag, bin_major in (("", True), ("_frame_major", False)):
        Y, fr = S._wpe_stft(a3, lens_dev, frames_max, 512, 128, window, bin_major)
        Z = torch.empty_strided(Y.shape, Y.stride(), dtype=Y.dtype, device="cuda")
        legs["stft" + tag] = lambda bin_major=bin_major: S._wpe_stft(a3, lens_dev, frames_max, 512, 128, window, bin_major)
        legs["core" + tag] = lambda Y=Y, Z=Z, fr=fr: LA.wpe_on_device(Y, channels=D, frames=fr, out=Z)
        legs["istft" + tag] = lambda Z=Z, fr=fr: S._wpe_istft(Z, fr, D, 512, 128, window, 128 * (frames_max - 1))
    r = timed_alternating(legs, repeats)
    z, z_lens = module(audio, lengths=lens)
    worst = 0.0
    for b in range(0, len(lengths), 12):  # the ragged rows against the per-cut calls (which run torch.stft / torch.istft)
        want = module(audio[b : b + 1, ..., : lengths[b]])[0]
        worst = max(worst, float((z[b, ..., : z_lens[b]] - want).norm() / want.norm()))
    r["rel_l2_ragged_vs_per_cut_worst_of_4_rows"] = worst
    r["speedup_ragged_vs_per_cut_loop"] = r["per_cut_loop"]["median_ms"] / r["ragged_call"]["median_ms"]
    r["ragged_over_padded_call"] = r["ragged_call"]["median_ms"] / r["padded_call"]["median_ms"]
    return r


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
        r["ragged"] = ragged_leg(module, audio, mono_len if audio.ndim == 2 else [audio.shape[-1]] * audio.shape[0], args.repeats)
        print(name, json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
