"""GPU: the global-statistics launches (csrc/kernel_stats.hpp) at the edges tests/test_gpu_stats.py does not reach: feature dimensions at
the lane's width and at the column tile (64 float32 / 128 binary16 bins), cuts at the row-lane count (15, 16, 17 frames) and one frame short
of a block (255), cuts of no frames first, last, two in a row and alone in an update, a float32 base off its 16-byte boundary, and an update
of more work items than the partial launch has workgroups (every workgroup takes a second item).

Which loads a layout takes (16-byte loads only where base and row stride keep every lane's group on a 16-byte boundary, and then only for
a group that lies wholly inside the frame) and how many work items an update plans are pinned on the CPU by the first test here, through
tests/native/stats_tables_capi.cpp; it needs no device.  The bar is that of tests/test_gpu_stats.py (tests/_stats_gpu.py): the device within
max(2 x the reference statement's own error, 1e-13) of the longdouble truth; every other check is for equal bits.

Measured on an MI355X, mean error / std error (the reference statement's own in brackets):
    F 4 ... 129 float32   5.3e-17 ... 1.05e-16 / 1.08e-16 ... 2.41e-16  (the same / 2.5e-16 ... 2.1e-15)
    F 8 ... 129 binary16  5.3e-17 ... 1.05e-16 / 1.51e-16 ... 2.29e-16  (the same / 3.7e-16 ... 7.9e-16)
    zero-frame cuts       1.07e-16 / 2.11e-16 float32, 1.09e-16 / 2.46e-16 binary16  (1.07e-16 / 5.38e-16, 1.09e-16 / 7.48e-16)
    700 cuts, F 257       1.10e-16 / 1.56e-15 float32 (3500 work items), 1.09e-16 / 1.98e-15 binary16 (2100)  (the reference: the same figures)
Time (pytest's own): with tests/test_gpu_featmix_edges.py in one process 3.2 s for the 71 tests of both; the slowest test here takes
0.06 s.  The GPU suite: 1016 tests in 201.7 s, the parent's 946 tests in 194.5 s.
"""
import numpy as np
import pytest
import torch

from _stats_gpu import bits, dev, hold_to_the_bar, reference_over, run_packed, same_bits

import lhotse_amd as LA

from test_gpu_mix import MAX_WORKGROUPS  # 1792, pinned to items_grid (csrc/hipfeat.hip) by tests/test_mix_abi.py
from test_stats_host import F16, F32, OK, plan, shim  # noqa: F401  (shim: the module-scoped fixture that builds the C entry points)

gpu = pytest.mark.gpu
DIMS = (4, 5, 7, 8, 9, 64, 65, 128, 129)
HALF_DIMS = (8, 9, 128, 129)
LENGTHS = (15, 16, 17, 255, 0, 1)  # kStRowLanes - 1, kStRowLanes, kStRowLanes + 1, kStBlockFrames - 1, none, one
TRIP_F, TRIP_CUTS, TRIP_GROUP = 257, 700, 300
CASES = [(F, False) for F in DIMS] + [(F, True) for F in HALF_DIMS]


def matrices(F, lengths, half=False, seed=0):
    rng = np.random.RandomState(seed + 1000 * F + int(half))
    mats = [(rng.standard_normal((n, F)) * 2.5 - 8.0).astype(np.float32) for n in lengths]
    return [m.astype(np.float16) for m in mats] if half else mats


def strides(F, half):
    """The row strides of the gapped layouts: a gap of 3 elements, and the gap up to the next multiple of a 16-byte group behind F."""
    group = 8 if half else 4
    return F + 3, F + (group - F % group)


def trip_lengths():
    return [1 + i % 3 for i in range(TRIP_CUTS)]


def test_the_layouts_take_the_loads_and_plan_the_items_the_cases_are_built_for(shim):  # noqa: F811
    assert shim.st_row_lanes() == 16 and shim.st_block_frames() == 256
    for F, half in CASES:
        dtype, group = (F16, 8) if half else (F32, 4)
        lengths = list(LENGTHS)
        st, info, table, msg = plan(shim, F, lengths, dtype=dtype)
        assert st == OK and info[1] == 5 and info[3] == 5 * -(-F // (16 * group)), msg  # one block per cut that has frames
        assert info[4] == (1 if F % group == 0 else 0)  # packed: 16-byte loads only where a frame is whole groups
        s3, s16 = strides(F, half)
        assert plan(shim, F, lengths, stride=s3, dtype=dtype)[1][4] == (1 if s3 % group == 0 else 0)
        assert s16 % group == 0 and s16 > F and plan(shim, F, lengths, stride=s16, dtype=dtype)[1][4] == 1
        if not half:  # a 16-byte stride from a base 4, 8, 12 bytes off: element loads
            assert [plan(shim, F, lengths, stride=s16, base=4096 + k)[1][4] for k in (0, 4, 8, 12)] == [1, 0, 0, 0]
    # over the cases, 16-byte loads meet a last group that the frame cuts (F is no multiple of the group) and one that it does not
    assert {F % 4 == 0 for F in DIMS} == {F % 8 == 0 for F in HALF_DIMS} == {True, False}
    assert {-(-F // 64) for F in DIMS} == {1, 2, 3} and {-(-F // 128) for F in HALF_DIMS} == {1, 2}  # 64 | 65 and 128 | 129: a further tile of one bin
    # the second trip: 700 blocks x 5 / 3 tiles of bins; in updates of 300 cuts no workgroup takes a second item
    lens = trip_lengths()
    assert len(lens) == TRIP_CUTS <= 700 and set(lens) == {1, 2, 3}
    for dtype, items in ((F32, 3500), (F16, 2100)):
        assert plan(shim, TRIP_F, lens, dtype=dtype)[1][3] == items > MAX_WORKGROUPS
        tiles = 3 if dtype == F16 else 5
        assert max(plan(shim, TRIP_F, lens[i: i + TRIP_GROUP], dtype=dtype)[1][3] for i in range(0, TRIP_CUTS, TRIP_GROUP)) == TRIP_GROUP * tiles <= MAX_WORKGROUPS


@gpu
@pytest.mark.parametrize("F,half", CASES, ids=[f"F{F}-{'f16' if h else 'f32'}" for F, h in CASES])
def test_dims_at_the_lane_and_tile_edges_with_cuts_at_the_row_lane_edges(F, half):
    mats = matrices(F, LENGTHS, half)
    frames = [len(m) for m in mats]
    wide = [m.astype(np.float32) for m in mats]
    acc = run_packed(F, mats)
    want = bits(acc)
    assert want[0] == sum(LENGTHS)
    hold_to_the_bar(f"edges F {F} {'binary16' if half else 'float32'}", acc, reference_over(F, wide), wide)
    flat = np.concatenate(mats)
    for stride in strides(F, half):  # rows further apart than F: the gap holds NaN and is never read
        buf = np.full((len(flat), stride), np.nan, dtype=flat.dtype)
        buf[:, :F] = flat
        x = dev(buf)[:, :F]
        assert x.stride() == (stride, 1) and x.data_ptr() % 16 == 0
        other = LA.HipStatsAccumulator(F)
        other.update(x, frames)
        assert same_bits(bits(other), want), (F, half, stride)
    if not half:  # the same rows, 16 bytes apart or more, from a base 4, 8 and 12 bytes off a 16-byte boundary
        stride = strides(F, half)[1]
        room = torch.full((len(flat) * stride + 4,), float("nan"), dtype=torch.float32, device="cuda")
        for shift in (1, 2, 3):
            room.fill_(float("nan"))
            view = room[shift: shift + len(flat) * stride].view(len(flat), stride)[:, :F]
            view.copy_(dev(flat))
            assert view.data_ptr() % 16 == 4 * shift and (stride * 4) % 16 == 0
            other = LA.HipStatsAccumulator(F)
            other.update(view, frames)
            assert same_bits(bits(other), want), (F, shift)


@gpu
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_cuts_of_no_frames_first_last_two_in_a_row_and_alone_in_an_update(half):
    F = 80
    a, b, c, m0 = matrices(F, (17, 300, 5, 40), half, seed=3)
    z = a[:0]
    wide = [m.astype(np.float32) for m in (a, b, c)]
    want = bits(run_packed(F, [a, b, c]))
    for name, mats in (("first", [z, a, b, c]), ("last", [a, b, c, z]), ("two in a row", [a, z, z, b, c]), ("everywhere", [z, z, a, z, b, z, z, c, z])):
        assert same_bits(bits(run_packed(F, mats)), want), name
        # ... and on a state that already holds frames
        assert same_bits(bits(run_packed(F, mats, acc=run_packed(F, [m0]))), bits(run_packed(F, [a, b, c], acc=run_packed(F, [m0])))), name
    hold_to_the_bar(f"zero-frame cuts {'binary16' if half else 'float32'}", run_packed(F, [z, a, z, z, b, c, z]), reference_over(F, wide), wide)
    # an update of nothing but a cut of no frames, between two updates: every bit and total_frames stay
    acc = run_packed(F, [a])
    before = bits(acc)
    acc.update(dev(z), [0])
    assert same_bits(bits(acc), before)
    acc.update(dev(b), [0], first_row=[7])  # rows that are there, none of them taken
    acc.update(dev(np.stack([b[:9], b[9:18]])), [0, 0])  # a padded batch of two cuts of no frames
    assert same_bits(bits(acc), before) and acc.total_frames == len(a)
    acc.update(dev(np.concatenate([b, c])), [len(b), len(c)])
    assert same_bits(bits(acc), bits(run_packed(F, [a, b, c], [slice(0, 1), slice(1, 3)])))
    assert same_bits(bits(acc), want)  # (grouping does not change a bit)


@gpu
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_more_work_items_than_workgroups(half):
    F = TRIP_F
    mats = matrices(F, trip_lengths(), half, seed=5)
    wide = [m.astype(np.float32) for m in mats]
    whole = run_packed(F, mats)  # 3500 (float32) / 2100 (binary16) work items: every workgroup of the partial launch takes a second one
    groups = [slice(i, min(i + TRIP_GROUP, TRIP_CUTS)) for i in range(0, TRIP_CUTS, TRIP_GROUP)]
    parts = run_packed(F, mats, groups)  # at most 1500 items per update: one item per workgroup
    assert same_bits(bits(whole), bits(parts)) and bits(whole)[0] == sum(trip_lengths())
    assert same_bits(bits(run_packed(F, mats)), bits(whole)), "two runs differ"
    hold_to_the_bar(f"700 cuts F 257 {'binary16' if half else 'float32'}", whole, reference_over(F, wide), wide)
