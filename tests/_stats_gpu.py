"""The helpers the GPU tests of the global feature statistics share (tests/test_gpu_stats.py, tests/test_gpu_stats_edges.py): packed
updates of a ``HipStatsAccumulator``, its state as bits, and the bar -- the device within ``max(2 x the reference statement's own error on
the same input, FLOOR)``, FLOOR = 1e-13 being the worst-case bound of a blocked float64 sum of 256 terms plus at most 700 merges at
u = 1.1e-16 on positive terms.  Test infrastructure: the product never imports this."""
import numpy as np
import torch

import _stats_ref as S

import lhotse_amd as LA

FLOOR = 1e-13


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_packed(F, mats, groups=None, acc=None):
    """One update per group of cuts (default: one update with all) on the packed device matrix -> the accumulator."""
    acc = LA.HipStatsAccumulator(F) if acc is None else acc
    for g in groups or [slice(0, len(mats))]:
        part = mats[g]
        acc.update(dev(np.concatenate(part)), [len(m) for m in part])
    return acc


def bits(acc):
    st = acc.state()
    return st["total_frames"], st["total_sum"].view(np.int64).copy(), st["total_unnorm_var"].view(np.int64).copy()


def same_bits(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def reference_over(F, mats):
    ref = S.ReferenceStatement(F)
    for m in mats:
        if len(m):
            ref.update(np.asarray(m, dtype=np.float32))
    return ref


def hold_to_the_bar(what, got, ref, mats):
    """``got`` / ``ref``: objects with norm_means / norm_stds (or dicts); ``mats``: the float32 inputs."""
    g = got if isinstance(got, dict) else got.get()
    r = ref if isinstance(ref, dict) else ref.get()
    mats = [np.asarray(m, dtype=np.float32) for m in mats]
    (dm, ds), (rm, rs) = S.errors(g["norm_means"], g["norm_stds"], mats), S.errors(r["norm_means"], r["norm_stds"], mats)
    print(f"[stats] {what}: device {dm:.3g} / {ds:.3g}  (reference statement {rm:.3g} / {rs:.3g})")
    assert dm <= max(2.0 * rm, FLOOR) and ds <= max(2.0 * rs, FLOOR), (what, dm, ds, rm, rs)
    for key in ("norm_means", "norm_stds"):  # the float32 casts: at most 1 ulp from the reference's
        a, b = g[key].astype(np.float32), r[key].astype(np.float32)
        assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64)).all(), (what, key)
