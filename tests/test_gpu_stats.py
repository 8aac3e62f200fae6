"""GPU: global feature statistics on the device (``HipStatsAccumulator``, ``GlobalStatsPass``; csrc/kernel_stats.hpp).

Truth is numpy ``longdouble`` over the concatenated float32 inputs.  Errors are taken per statistic as the maximum over the bins of
``|value - truth| / scale`` (mean: ``scale = mean(|x|)`` of the bin; std: ``scale = std``), and the device must stay within
``max(2 x the reference statement's own error on the same input, 1e-13)`` -- 1e-13 being the worst-case bound of a blocked float64 sum of
256 terms plus at most 700 merges at u = 1.1e-16 on positive terms.  The float32 casts (what ``HipGlobalMVN`` stores) differ from the
reference's casts by at most 1 float32 ulp.  Every test prints the figures it asserts.

Shapes: F in {1, 3, 80, 257}; cuts of 1, 2, kStBlockFrames - 1, 0 (in the middle), kStBlockFrames, kStBlockFrames + 1 and
3 * kStBlockFrames + 5 frames (tests/_stats_ref.py::make_matrices).

Achieved on an MI355X, mean error / std error (the reference statement's own in brackets; also in DESIGN.md section 4.14):
    packed F 1      1.05e-16 / 1.34e-16  (1.05e-16 / 4.15e-17)      packed F 3      1.78e-17 / 8.35e-17  (1.78e-17 / 2.60e-16)
    packed F 80     9.97e-17 / 2.06e-16  (9.97e-17 / 5.76e-16)      packed F 257    1.08e-16 / 2.53e-16  (1.08e-16 / 5.66e-16)
    binary16 F 80   1.09e-16 / 1.83e-16  (1.09e-16 / 6.88e-16)      offset 1e4      9.05e-17 / 2.38e-12  (9.05e-17 / 2.36e-12)
    20 cuts         1.09e-16 / 2.51e-16  (1.09e-16 / 4.23e-16)      halves merged   9.97e-17 / 2.30e-16  (9.97e-17 / 5.76e-16)
    add_waveforms   9.60e-17 / 2.28e-16  (9.60e-17 / 3.24e-16)      add_features    8.92e-17 / 1.65e-16  (8.92e-17 / 2.70e-16)
    binary16 F 257  1.10e-16 / 2.16e-16  (1.10e-16 / 1.56e-15)
"""
import json
import os

import numpy as np
import pytest
import torch

import _stats_ref as S
from _stats_gpu import bits, dev, hold_to_the_bar, reference_over, run_packed, same_bits

import lhotse_amd as LA
from lhotse_amd import _lib

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIMS = (1, 3, 80, 257)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "stats.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, "stats.npz"))


@pytest.fixture(scope="module")
def clean():
    """Per F: the matrices, the packed float32 run (its bits) and the reference statement -- computed once, shared, never changed."""
    out = {}
    for F in DIMS:
        mats = S.make_matrices(F)
        acc = run_packed(F, mats)
        out[F] = (mats, bits(acc), acc.get(), reference_over(F, mats))
    return out


@pytest.mark.parametrize("F", DIMS)
def test_packed_float32_against_the_golden_and_the_truth(clean, golden, F):
    mats, b, got, ref = clean[F]
    meta, arrays = golden
    name = f"f{F}"
    last = len(meta["cases"][name]["frames"]) - 1
    gold = {k: arrays[f"{name}/{last}/{k}"] for k in ("norm_means", "norm_stds")}
    assert b[0] == meta["cases"][name]["total_frames"] == sum(len(m) for m in mats)
    assert np.array_equal(ref.norm_means, gold["norm_means"]) and np.array_equal(ref.norm_stds, gold["norm_stds"])
    hold_to_the_bar(f"packed F {F}", got, gold, mats)


@pytest.mark.parametrize("F", DIMS)
def test_a_padded_batch_with_a_row_gap_and_descending_rows_gives_the_same_bits(clean, F):
    mats, want, _, _ = clean[F]
    B, Tmax, stride = len(mats), max(len(m) for m in mats), F + 3
    buf = np.full((B, Tmax, stride), np.nan, dtype=np.float32)  # padding rows and the gap behind every frame hold NaN
    for b, m in enumerate(mats):
        buf[B - 1 - b, : len(m), :F] = m  # cut b lies in row B - 1 - b: descending first rows
    x = dev(buf)[:, :, :F]
    assert x.stride() == (Tmax * stride, stride, 1)
    acc = LA.HipStatsAccumulator(F)
    acc.update(x, [len(m) for m in mats], first_row=[(B - 1 - b) * Tmax for b in range(B)])
    assert same_bits(bits(acc), want)
    # ... and the contiguous (B, Tmax, F) tensor with the default first rows, in batch order
    acc2 = LA.HipStatsAccumulator(F)
    tight = np.full((B, Tmax, F), np.nan, dtype=np.float32)
    for b, m in enumerate(mats):
        tight[b, : len(m)] = m
    acc2.update(dev(tight), torch.tensor([len(m) for m in mats]))
    assert same_bits(bits(acc2), want)


def test_binary16_input_with_subnormals_and_the_largest_values_at_any_2_byte_boundary():
    F = 80
    mats = S.make_matrices(F, half=True)
    flat = np.concatenate(mats)
    assert flat.dtype == np.float16 and (np.abs(flat.astype(np.float32)) == 65504.0).any() and ((flat != 0) & (np.abs(flat.astype(np.float32)) < 6.1e-5)).any()
    frames = [len(m) for m in mats]
    acc = LA.HipStatsAccumulator(F)
    acc.update(dev(flat), frames)
    wide = [m.astype(np.float32) for m in mats]
    hold_to_the_bar("binary16 F 80", acc, reference_over(F, wide), wide)
    # a base pointer that is 2-byte but not 16-byte aligned: the same bits
    room = torch.zeros(flat.size + 8, dtype=torch.float16, device="cuda")
    for shift in (1, 3):
        view = room[shift: shift + flat.size].view(len(flat), F)
        view.copy_(dev(flat))
        assert view.data_ptr() % 16 == 2 * shift
        other = LA.HipStatsAccumulator(F)
        other.update(view, frames)
        assert same_bits(bits(other), bits(acc)), shift
    # ... and so does the float32 widening of the same values, bin for bin (binary16 widens exactly)
    again = run_packed(F, wide)
    assert same_bits(bits(again), bits(acc))
    # F = 257 (three tiles of 128 bins, the last lane with ONE bin): rows 264 elements apart take 16-byte loads up to bin 255 and an
    # element load for bin 256; the packed matrix (rows 514 bytes apart) is read element by element.  The same bits, and within the bar.
    F = 257
    mats = S.make_matrices(F, half=True)
    flat, frames = np.concatenate(mats), [len(m) for m in mats]
    gapped = np.full((len(flat), 264), np.nan, dtype=np.float16)
    gapped[:, :F] = flat
    a, b = LA.HipStatsAccumulator(F), LA.HipStatsAccumulator(F)
    a.update(dev(gapped)[:, :F], frames)
    b.update(dev(flat), frames)
    assert same_bits(bits(a), bits(b))
    wide = [m.astype(np.float32) for m in mats]
    hold_to_the_bar("binary16 F 257", a, reference_over(F, wide), wide)


def test_an_offset_of_1e4_with_a_std_of_1e_2(golden):
    meta, arrays = golden
    F, kw = S.GOLDEN_CASES["offset80"]
    mats = S.make_matrices(F, **kw)
    ref = reference_over(F, mats)
    last = len(meta["cases"]["offset80"]["frames"]) - 1
    assert np.array_equal(ref.norm_stds, arrays[f"offset80/{last}/norm_stds"])
    assert 5e-3 < ref.norm_stds.min() and ref.norm_stds.max() < 2e-2 and abs(ref.norm_means.mean() - 1e4) < 1.0
    hold_to_the_bar("offset 1e4, std 1e-2", run_packed(F, mats), ref, mats)  # (a sum-of-squares formulation errs by ~1e-4 here)


def test_inf_and_nan_stay_in_their_own_bins(clean):
    F = 80
    mats, want, _, _ = clean[F]
    dirty = [m.copy() for m in mats]
    dirty[4][3, 10] = np.inf
    dirty[5][7, 20] = np.nan
    n, s, v = bits(run_packed(F, dirty))
    others = np.ones(F, dtype=bool)
    others[[10, 20]] = False
    assert n == want[0] and np.array_equal(s[others], want[1][others]) and np.array_equal(v[others], want[2][others])
    s, v = s.view(np.float64), v.view(np.float64)
    assert s[10] == np.inf and np.isnan(v[10]) and np.isnan(s[20]) and np.isnan(v[20])


def test_order_and_grouping_do_not_change_a_bit():
    F = 80
    mats = (S.make_matrices(F, seed=1) + S.make_matrices(F, seed=2) + S.make_matrices(F, seed=3))[:20]
    assert len(mats) == 20 and any(len(m) == 0 for m in mats)
    whole = bits(run_packed(F, mats))
    per_cut = [slice(i, i + 1) for i in range(20)]
    # twenty updates enqueued without a host wait between them cycle the 16 staging slots
    assert same_bits(bits(run_packed(F, mats, per_cut)), whole)
    assert same_bits(bits(run_packed(F, mats, [slice(0, 3), slice(3, 4), slice(4, 20)])), whole)
    assert same_bits(bits(run_packed(F, mats)), whole) and same_bits(bits(run_packed(F, mats, per_cut)), whole)  # two runs of the whole sequence
    ref = reference_over(F, mats)
    hold_to_the_bar("20 cuts", run_packed(F, mats), ref, mats)


def test_merge_and_reset(clean):
    F = 80
    mats, want, _, ref = clean[F]
    a, b = run_packed(F, mats[:4]), run_packed(F, mats[4:])
    a.merge(b)
    assert a.total_frames == want[0]
    hold_to_the_bar("two halves merged", a, ref, mats)
    before = bits(a)
    a.merge(LA.HipStatsAccumulator(F))  # an empty state changes nothing
    a.merge({"total_frames": 0, "total_sum": np.zeros(F), "total_unnorm_var": np.zeros(F)})
    assert same_bits(bits(a), before)
    # merging into an empty accumulator assigns
    c = LA.HipStatsAccumulator(F)
    c.merge(b.state())
    assert same_bits(bits(c), bits(b))
    a.reset()
    assert a.total_frames == 0 and not a.total_sum.any() and not a.total_unnorm_var.any()
    assert same_bits(bits(run_packed(F, mats, acc=a)), want)  # reset, then the same updates: the same bits


def test_the_global_stats_pass_over_waveforms_and_stored_features(tmp_path):
    rng = np.random.RandomState(11)
    waves = [(rng.rand(n).astype(np.float32) - 0.5) for n in (4800, 7000, 9999, 12345, 16000, 19200)]  # 0.3 ... 1.2 s at 16 kHz
    ex = LA.HipFbank()
    gp = LA.GlobalStatsPass(ex)
    gp.add_waveforms(waves, 16000)
    feats = ex.extract_batch([dev(w) for w in waves], 16000)
    assert all(f.device.type == "cuda" for f in feats)
    acc = LA.HipStatsAccumulator(80)
    for f in feats:
        acc.update(f)
    assert same_bits(bits(gp.accumulator), bits(acc))
    host = [f.cpu().numpy() for f in feats]
    hold_to_the_bar("add_waveforms", gp.result(), reference_over(80, host), host)
    # stored binary16 features: written by HipArchiveF16Writer, read back as stored, uploaded once
    with LA.HipArchiveF16Writer(tmp_path / "feats") as w:
        keys = w.write_packed(np.concatenate(host), [len(h) for h in host])
        path = w.storage_path
    reader = LA.HipArchiveReader(path)
    stored = [reader.read_raw(k) for k in keys]
    assert all(m.dtype == np.float16 for m in stored)
    sp = LA.GlobalStatsPass(80)
    sp.add_features(stored[:2])
    sp.add_features(stored[2:])
    wide = [m.astype(np.float32) for m in stored]
    hold_to_the_bar("add_features (hip_archive_f16)", sp.result(), reference_over(80, wide), wide)
    with pytest.raises(ValueError):
        sp.add_waveforms(waves, 16000)  # a pass without an extractor


def test_refusals_reach_python_and_leave_the_state_as_it_was(clean):
    F = 80
    mats, want, _, _ = clean[F]
    acc = run_packed(F, mats)
    x = dev(mats[-1])

    def refused(status, *args):
        with pytest.raises(_lib.HipFeatError) as e:
            acc.lib.check("hipfeat_stats_update", acc.handle, *args, int(torch.cuda.current_stream().cuda_stream))
        assert e.value.status == status and same_bits(bits(acc), want)

    n, one = _lib.i64([len(x)]), _lib.i64([0])
    refused(_lib.ERR_INVALID, x.data_ptr(), x.numel() - 1, 0, 1, None, _lib.addr(n), F)          # the last element lies beyond the buffer
    refused(_lib.ERR_INVALID, x.data_ptr(), x.numel(), 0, 1, None, _lib.addr(_lib.i64([-1])), F)  # negative frames
    refused(_lib.ERR_INVALID, x.data_ptr(), x.numel(), 0, 1, _lib.addr(_lib.i64([-1])), _lib.addr(n), F)  # a negative row
    refused(_lib.ERR_INVALID, x.data_ptr(), x.numel(), 0, 1, None, _lib.addr(n), F - 1)           # stride < F
    refused(_lib.ERR_INVALID, x.data_ptr(), x.numel(), 2, 1, None, _lib.addr(n), F)               # an unknown type
    refused(_lib.ERR_INVALID, x.data_ptr() + 2, x.numel() - 1, 0, 1, None, _lib.addr(n), F)       # a base pointer off its element alignment
    refused(_lib.ERR_INVALID, x.data_ptr(), x.numel(), 0, 0, None, _lib.addr(n), F)               # no cuts
    refused(_lib.ERR_UNSUPPORTED, x.data_ptr(), 2 ** 40, 0, 9, None, _lib.addr(_lib.i64([2 ** 29] * 9)), F)  # too many blocks for one launch
    assert one[0] == 0
    with pytest.raises(_lib.HipFeatError) as e:
        acc.update(torch.from_numpy(mats[-1]))  # a CPU tensor: no fallback
    assert e.value.status == _lib.ERR_INVALID and "there is no CPU fallback" in str(e.value)
    with pytest.raises(TypeError):
        acc.update(x.double())
    with pytest.raises(ValueError):
        acc.update(x[:, :5])
    with pytest.raises(ValueError):
        acc.update(x.view(1, len(x), F))  # a padded batch without num_frames
    assert same_bits(bits(acc), want)
    assert LA.get_or_create_stats("cuda", F) is LA.get_or_create_stats(None, F) and LA.get_or_create_stats("cuda", 3) is not LA.get_or_create_stats("cuda", F)
