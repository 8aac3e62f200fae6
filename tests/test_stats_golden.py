"""CPU: the numpy restatement of ``StatsAccumulator`` (tests/_stats_ref.py::ReferenceStatement) equals what the reference's own class
held after every update (tests/golden/stats.npz, written by tools/make_golden_stats.py) bit for bit; the restatement of the device's
blocked order stays within the bar the GPU test holds the device to."""
import json
import os

import numpy as np
import pytest

import _stats_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "stats.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "stats.npz"))


@pytest.mark.parametrize("name", sorted(S.GOLDEN_CASES))
def test_the_reference_statement_equals_the_reference_bit_for_bit(golden, name):
    meta, arrays = golden
    F, kw = S.GOLDEN_CASES[name]
    assert meta["block_frames"] == S.BLOCK_FRAMES and meta["cases"][name]["feature_dim"] == F
    mats = [m.astype(np.float32) for m in S.make_matrices(F, **kw) if len(m)]
    assert [len(m) for m in mats] == meta["cases"][name]["frames"]
    acc = S.ReferenceStatement(F)
    for k, m in enumerate(mats):
        acc.update(m)
        for key in ("total_sum", "total_unnorm_var", "norm_means", "norm_stds"):
            want = arrays[f"{name}/{k}/{key}"]
            assert want.dtype == np.float64 and np.array_equal(getattr(acc, key), want), (name, k, key)
    assert acc.total_frames == meta["cases"][name]["total_frames"]


@pytest.mark.parametrize("name", sorted(S.GOLDEN_CASES))
def test_the_blocked_order_stays_within_the_bar(name):
    F, kw = S.GOLDEN_CASES[name]
    mats = [m.astype(np.float32) for m in S.make_matrices(F, **kw)]
    ref, dev = S.ReferenceStatement(F), S.DeviceStatement(F)
    for m in mats:
        dev.update(m)  # (the cut of no frames contributes nothing)
        if len(m):
            ref.update(m)
    assert dev.total_frames == ref.total_frames
    ref_err, dev_err = S.errors(ref.norm_means, ref.norm_stds, mats), S.errors(dev.norm_means, dev.norm_stds, mats)
    assert all(d <= max(2.0 * r, 1e-13) for d, r in zip(dev_err, ref_err)), (ref_err, dev_err)


def test_grouping_and_merging_of_the_statements():
    mats = [m for m in S.make_matrices(5) if len(m)]
    whole, a, b = S.ReferenceStatement(5), S.ReferenceStatement(5), S.ReferenceStatement(5)
    for m in mats:
        whole.update(m)
    for m in mats[:3]:
        a.update(m)
    for m in mats[3:]:
        b.update(m)
    a.merge(b)
    a.merge(S.ReferenceStatement(5))  # an empty state changes nothing
    assert a.total_frames == whole.total_frames
    np.testing.assert_allclose(a.norm_means, whole.norm_means, rtol=1e-14)
    np.testing.assert_allclose(a.norm_stds, whole.norm_stds, rtol=1e-13)
