"""CPU: the placement helper of the large-offset GPU tests (tests/_large_buffers.py) -- the far placement puts its items where it says
(astride and behind byte offset 2^31, byte offset 2^32 and element index 2^31), nothing overlaps, everything fits the buffers, and the
near twin differs from it in nothing but the offsets' upper bits."""
import numpy as np
import pytest

import _large_buffers as LB

# (lengths of the seven items, unit): waveforms at 8 / 16 / 48 kHz, arena items, output rows of every stride the GPU module uses
SEVEN = [
    ([6401, 8801, 11201, 13601, 16001, 19201, 22401], 1),
    ([19201, 26401, 33601, 40801, 48001, 57601, 67201], 1),
    ([2, 3, 4, 5, 70001, 255, 4099], 1),
    ([90001] * 7, 1),
    ([40, 55, 70, 85, 100, 120, 140], 80),
    ([40, 55, 70, 85, 100, 120, 140], 83),
    ([40, 55, 70, 85, 100, 120, 140], 257),
    ([2, 2, 3, 2, 5, 2, 2], 13),
    ([40, 55, 70, 85, 100, 120, 140], 128),  # a stride that divides the marks
]


@pytest.mark.parametrize("lengths,unit", SEVEN)
def test_seven_items_straddle_and_follow_every_mark(lengths, unit):
    p = LB.place(lengths, unit)
    LB.check(p)
    assert p.roles == ["control"] + ["straddle", "behind"] * 3 and p.marks == [0] + [m for m in LB.MARKS for _ in (0, 1)]
    assert p.lengths == lengths
    for o, n, role, mark in zip(p.far, p.lengths, p.roles, p.marks):
        first, last = o * unit, (o + n) * unit - 1
        if role == "straddle":
            assert first < mark <= last and abs((mark - first) - (last - mark)) <= 2 * unit + 1  # about half of it on either side
            assert unit > 1 or o % 2 == 1
        if role == "behind":
            assert first > mark and first - mark <= (max(lengths) + LB.GAP + 8) * unit  # wholly above the mark, and close to it
    # the twin: a few hundred thousand elements at the most, same order, same alignment
    assert p.near_size <= sum(lengths) + 7 * (LB.GAP + 4) and p.near_size * unit < 2 ** 24
    assert [a % 4 for a in p.far] == [b % 4 for b in p.near] and sorted(p.near) == p.near


@pytest.mark.parametrize("length,unit", [(16001, 1), (48001, 1), (1, 1), (100, 80), (100, 83), (100, 257), (100, 81), (100, 128)])
def test_four_equal_items_start_right_behind_the_marks(length, unit):
    p = LB.place_behind(length, unit)
    LB.check(p)
    assert p.roles == ["control", "behind", "behind", "behind"] and p.far[0] == LB.CONTROL
    for k, (o, mark) in enumerate(zip(p.far[1:], LB.MARKS)):
        assert mark < o * unit <= mark + (k + 2) * unit
        if unit == 1:
            assert o == mark + k + 1  # 1, 2 and 3 elements behind: the three alignments that are not 16-byte aligned
    assert p.near_size <= 4 * (length + LB.GAP + 4)


def test_the_checks_catch_a_wrong_placement():
    p = LB.place([6401, 8801, 11201, 13601, 16001, 19201, 22401])
    with pytest.raises(AssertionError):  # does not fit a buffer that ends at 2^31
        LB.check(p, size=2 ** 31)
    moved = p._replace(far=[p.far[0], p.far[1] + 8801] + p.far[2:])
    with pytest.raises(AssertionError):  # no longer astride 2^29 (and on top of its neighbour)
        LB.check(moved)
    with pytest.raises(AssertionError):  # a twin at another alignment
        LB.check(p._replace(near=[p.near[0], p.near[1] + 1] + p.near[2:]))
    with pytest.raises(AssertionError):  # two items on top of each other
        LB.check(p._replace(far=p.far[:6] + [p.far[5] + 3]))


def test_everything_the_gpu_module_places_fits_its_buffers():
    assert LB.BUFFER_ELEMS == 2 ** 31 + 2 ** 24 and LB.MARKS == (2 ** 29, 2 ** 30, 2 ** 31)
    worst = LB.place([67201] * 7)  # 1.4 s at 48 kHz
    assert max(o + n for o, n in zip(worst.far, worst.lengths)) < 2 ** 31 + 2 ** 18
    rows = LB.place([140] * 7, 257)  # 1.4 s of 257-column rows
    assert max((o + n) * 257 for o, n in zip(rows.far, rows.lengths)) < 2 ** 31 + 2 ** 18
    # byte offsets, as the kernels form them: the items behind a mark have a non-zero upper dword (2^30, 2^31) or sign bit (2^29)
    p = LB.place_behind(16001)
    lo = [np.uint32((4 * o) & 0xFFFFFFFF) for o in p.far]
    assert [int(x) for x in lo[1:]] == [2 ** 31 + 4, 8, 12] and [(4 * o) >> 32 for o in p.far] == [0, 0, 1, 2]
