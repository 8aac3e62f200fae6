#!/usr/bin/env python3
"""
TEST INFRASTRUCTURE -- generates tests/golden/stats.npz (+ stats.json): what the REFERENCE's own ``StatsAccumulator``
(lhotse/features/base.py:990-1033) holds after every update over the matrices of tests/_stats_ref.py::GOLDEN_CASES.

Needs the real lhotse (authoring container only):

    python tools/make_golden_stats.py

The matrices are drawn from fixed seeds (``_stats_ref.make_matrices``: the tests draw the same ones, nothing of them is stored).  The
cut of no frames is left out for the reference: its ``np.var`` of an empty matrix would turn every bin into NaN.  Per case and update k:
``<case>/<k>/total_sum``, ``total_unnorm_var``, ``norm_means``, ``norm_stds`` (float64); stats.json holds the frame counts.  Asserted
here for every case: the numpy restatement ``_stats_ref.ReferenceStatement`` equals the reference bit for bit, and the restatement of
the device's blocked order stays within the bar of tests/test_gpu_stats.py (other inputs are to be picked if one fails).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import _stats_ref as S
    from oracle.make_golden import import_reference

    import_reference()
    from lhotse.features.base import StatsAccumulator

    arrays, meta = {}, {"block_frames": S.BLOCK_FRAMES, "cases": {}}
    for name, (F, kw) in S.GOLDEN_CASES.items():
        mats = [m for m in S.make_matrices(F, **kw) if len(m)]
        ref, mine, dev = StatsAccumulator(feature_dim=F), S.ReferenceStatement(F), S.DeviceStatement(F)
        for k, m in enumerate(mats):
            ref.update(m.astype(np.float32))
            mine.update(m.astype(np.float32))
            dev.update(m.astype(np.float32))
            for key in ("total_sum", "total_unnorm_var", "norm_means", "norm_stds"):
                arrays[f"{name}/{k}/{key}"] = np.asarray(getattr(ref, key), dtype=np.float64)
                assert np.array_equal(getattr(mine, key), arrays[f"{name}/{k}/{key}"]), (name, k, key)
        f32 = [m.astype(np.float32) for m in mats]
        ref_err, dev_err = S.errors(ref.norm_means, ref.norm_stds, f32), S.errors(dev.norm_means, dev.norm_stds, f32)
        print(f"{name}: F {F} frames {ref.total_frames}  reference {ref_err[0]:.3g} / {ref_err[1]:.3g}  device statement {dev_err[0]:.3g} / {dev_err[1]:.3g}")
        assert all(d <= max(2.0 * r, 1e-13) for d, r in zip(dev_err, ref_err)), (name, "the device's order misses the bar: pick other inputs")
        meta["cases"][name] = {"feature_dim": F, "frames": [len(m) for m in mats], "total_frames": int(ref.total_frames)}
    out_dir = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(out_dir, "stats.npz"), **arrays)
    with open(os.path.join(out_dir, "stats.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("stats.npz", os.path.getsize(os.path.join(out_dir, "stats.npz")), "bytes")


if __name__ == "__main__":
    main()
