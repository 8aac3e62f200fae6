#!/usr/bin/env python3
"""The matrix-core resampler against the generic kernel at the ratios with many phases: 441:160 (44.1 -> 16 kHz), 441:320 (22.05 -> 16),
441:640 (11.025 -> 16), 147:80 (44.1 -> 24) and 160:441 (16 -> 44.1), on 256 cuts of 10 s resident on the device.

Per ratio, both kernels are created in the same process (one under HIPFEAT_RESAMPLE_GENERIC=1, one under HIPFEAT_RESAMPLE_MFMA=1, which
puts a ratio on the matrix-core kernel whatever the library's routing rule says about it) and launched alternately: 5 warm-ups each, then --launches
(default 50) timed launches each, HIP events around every single launch, median reported.  Reported per kernel: ms per launch, cuts/s,
2 * kw flop per output sample over the time as TFLOP/s and as a share of the 155 TF f32 MFMA rate; and whether the outputs are equal.

    python tools/bench_resample_rates.py [--launches 50] [--cuts 256] [--seconds 10] [--out profiles/resample_rates.json]
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d DIR -- python tools/bench_resample_rates.py --once 44100:16000

--once SRC:DST runs the matrix-core kernel of one ratio four times and exits: the command of a counter run (counters are
collected in a run of their own, without tracing); --pmc-json merges the counter figures a summary of that run gave into the result file.
"routed_kernel" is what the library picks for the ratio with neither variable set.

End-to-end leg ("minibatch_44k1"): one mini-batch of 45 host-resident cuts of 10 s at 44.1 kHz, a third each at speed 0.9 / 1.0 / 1.1
-> 80-dim fbank at 16 kHz.  Device route: FusedMiniBatch.features_of_tracks with 8-element tracks (pack -> 441:160 launch -> speed launch
-> feature launch).  Host route (what gpu_resample=False leaves on the CPU, lhotse itself is not needed): the same rate conversion as the
reference computes it -- torch conv1d of the zero-padded samples with the 160 x 475 bank at stride 441, cut by cut, torch's threads as the
environment sets them -- and then the speed + feature launches of the device route over the 16 kHz samples."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RATES = [(44100, 16000), (22050, 16000), (11025, 16000), (44100, 24000), (16000, 44100)]
MFMA_F32_TFLOPS = 155.0


def make(orig, new, force=None):
    """force: None (the library's routing), "GENERIC" or "MFMA" """
    from lhotse_amd import augmentation as A

    if force:
        os.environ["HIPFEAT_RESAMPLE_" + force] = "1"
    try:
        return A.HipResampleTensor(orig, new)
    finally:
        if force:
            os.environ.pop("HIPFEAT_RESAMPLE_" + force, None)


def minibatch_leg(dev, steps, cuts=45, seconds=10.0, src=44100, sr=16000):
    import time

    import lhotse_amd as LA
    from lhotse_amd import constants
    from lhotse_amd.augmentation import perturb_num_samples
    from lhotse_amd.input_strategies import FusedMiniBatch

    rng = np.random.RandomState(5)
    n = int(seconds * src)
    xs = [(rng.rand(n).astype(np.float32) - 0.5) for _ in range(cuts)]
    factors = [(0.9, 1.0, 1.1)[i % 3] for i in range(cuts)]
    n16 = int(np.ceil(np.float32(160 * n / 441)))
    wants = [min(perturb_num_samples(n16, f), int(np.ceil(np.float32(sr // 1600 * n16 / (round(sr * f) // 1600))))) if f != 1.0 else n16 for f in factors]
    fm = FusedMiniBatch(LA.HipFbank(LA.HipFbankConfig(device=str(dev))))
    kernel, width, orig, new = constants.sinc_resample_kernel(src, sr)
    bank = torch.from_numpy(kernel)[:, None, :]

    def device_route():
        return fm.features_of_tracks([[(x, f, 0, None, True, w, None, src)] for x, f, w in zip(xs, factors, wants)], wants, sr)[0]

    def host_resample(x):
        xp = torch.nn.functional.pad(torch.from_numpy(x)[None, None, :], (width, width + orig))
        return torch.nn.functional.conv1d(xp, bank, stride=orig).transpose(1, 2).reshape(-1)[:n16].numpy()

    def host_route():
        ys = [host_resample(x) for x in xs]
        return fm.features_of_tracks([[(y, f, 0, None, True, w)] for y, f, w in zip(ys, factors, wants)], wants, sr)[0]

    out = {"cuts": cuts, "seconds_per_cut": seconds, "source_rate": src, "factors": "0.9 / 1.0 / 1.1 by thirds", "host_threads": torch.get_num_threads()}
    a, b = device_route(), host_route()
    torch.cuda.synchronize()
    out["max_abs_feature_difference_between_routes"] = float((a - b).abs().max())
    for name, fn in (("device_route", device_route), ("host_resample_route", host_route), ("device_route_again", device_route)):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / steps
        out[name] = {"ms_per_minibatch": round(wall * 1e3, 2), "cuts_per_s": round(cuts / wall, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cuts", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_rates.json"))
    ap.add_argument("--once", default=None, metavar="SRC:DST")
    ap.add_argument("--no-minibatch", action="store_true", help="skip the end-to-end leg")
    ap.add_argument("--pmc-json", default=None, help="a json object {ratio: {counter: value}} to store under 'lds_counters'")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(11)

    def batch(orig):
        n = int(round(args.seconds * orig))
        x = torch.empty(args.cuts * n, device=dev).uniform_(-0.5, 0.5, generator=g)
        return x, np.arange(args.cuts, dtype=np.int64) * n, np.full(args.cuts, n, dtype=np.int64)

    if args.once:
        orig, new = (int(v) for v in args.once.split(":"))
        r = make(orig, new, "MFMA")
        x, offs, lens = batch(orig)
        for _ in range(4):
            r.run(x, offs, lens)
        torch.cuda.synchronize()
        print(json.dumps({"ratio": f"{r.orig}:{r.new}", "kernel": r.kernel_name}))
        return

    res = {"workload": f"{args.cuts} cuts of {args.seconds:g} s, device resident, one hipfeat_resample launch per timing",
           "method": f"HIP events around each launch, kernels alternating, {args.warmup} warm-ups, median of {args.launches}",
           "mfma_f32_peak_tflops": MFMA_F32_TFLOPS, "ratios": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for orig, new in RATES:
        routed, generic, mfma = make(orig, new), make(orig, new, "GENERIC"), make(orig, new, "MFMA")
        assert generic.kernel_name == "resample_generic" and mfma.kernel_name == "resample_mfma"
        kinds = {"generic": generic, "mfma": mfma}
        x, offs, lens = batch(orig)
        outs, ms = {}, {k: [] for k in kinds}
        for i in range(args.warmup + args.launches):
            for k, r in kinds.items():
                ev[0].record()
                outs[k] = r.run(x, offs, lens)
                ev[1].record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ms[k].append(ev[0].elapsed_time(ev[1]))
        out_samples = int(outs["generic"][2].sum())
        kw = routed.kernel.shape[1]
        entry = {"orig": routed.orig, "new": routed.new, "kw": int(kw), "bank_floats": int(routed.kernel.size), "routed_kernel": routed.kernel_name,
                 "output_samples": out_samples, "kernels": {}}
        for k in kinds:
            t = float(np.median(ms[k]))
            tf = 2.0 * kw * out_samples / t / 1e9
            entry["kernels"][k] = {"ms_per_launch": round(t, 4), "ms_min": round(float(np.min(ms[k])), 4), "ms_max": round(float(np.max(ms[k])), 4),
                                   "cuts_per_s": round(args.cuts / t * 1e3, 1), "tflops": round(tf, 2),
                                   "share_of_mfma_f32_peak": round(tf / MFMA_F32_TFLOPS, 4)}
        entry["outputs_equal"] = bool(torch.equal(outs["mfma"][0], outs["generic"][0]))
        entry["mfma_speedup_over_generic"] = round(entry["kernels"]["generic"]["ms_per_launch"] / entry["kernels"]["mfma"]["ms_per_launch"], 3)
        res["ratios"][f"{routed.orig}:{routed.new}"] = entry
        del outs, x
    if not args.no_minibatch:
        res["minibatch_44k1"] = minibatch_leg(dev, max(args.launches // 5, 5))
    if args.pmc_json:
        with open(args.pmc_json) as f:
            res["lds_counters"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
