"""Test infrastructure: where to put a handful of items inside a buffer of more than 2^31 elements so that every 32-bit truncation of an
element or byte offset shows -- and the same items packed into a small buffer (the "near twin"), whose results the far ones must equal
bit for bit.  Pure integer arithmetic: checked on the CPU by tests/test_large_buffers.py, used on the GPU by
tests/test_gpu_large_offsets.py.

The marks, in float32 elements:

    2^29   byte offset 2^31: a signed 32-bit byte offset wraps
    2^30   byte offset 2^32: an unsigned 32-bit byte offset wraps
    2^31   a signed 32-bit element index wraps

``place(lengths)`` (seven items): a control item at offset 3; per mark one item that STRADDLES it (it starts about half its length
before the mark, at an odd offset) and one item BEHIND it.  Items must not overlap, and the straddling item covers the elements right
behind its mark, so the item behind a mark starts behind the straddling item: 1, 2 or 3 elements (2^29: 1, 2^30: 2, 2^31: 3) behind
the first 16-byte boundary that leaves ``GAP`` free elements after it.  ``place_behind(length)`` (four equal items, the uniform batch)
has no straddling items: the control item at offset 3 and one item that starts exactly 1 / 2 / 3 elements behind each mark.

The same functions place OUTPUT ROWS: with ``unit = row stride`` everything is counted in rows, a mark is the row that holds float index
2^29 / 2^30 / 2^31 of the output, and "straddles" / "behind" are judged in floats (``check``).
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence

MARKS = (2 ** 29, 2 ** 30, 2 ** 31)
BUFFER_ELEMS = 2 ** 31 + 2 ** 24  # the two buffers of the GPU module, in float32 elements
CONTROL = 3
GAP = 5  # free elements (rows) between neighbours of the near twin, and between a straddling item and the item behind its mark
ROLES = ("control", "straddle", "behind")


class Placement(NamedTuple):
    far: List[int]    # first element (row) of every item in the large buffer
    near: List[int]   # ... in the near twin: same order, same offsets modulo 4
    lengths: List[int]
    roles: List[str]  # "control" | "straddle" | "behind"
    marks: List[int]  # per item the mark it belongs to in ELEMENTS (0 for the control item)
    unit: int         # elements per counted unit (1: elements; a row stride: rows)
    near_size: int    # units the near twin needs


def _twin(far: Sequence[int], lengths: Sequence[int]) -> List[int]:
    near, pos = [], CONTROL - GAP
    for o, n in zip(far, lengths):
        p = pos + GAP
        p += (o - p) % 4
        near.append(p)
        pos = p + n
    return near


def _finish(far, lengths, roles, marks, unit) -> Placement:
    near = _twin(far, lengths)
    return Placement(list(far), near, [int(n) for n in lengths], list(roles), list(marks), int(unit), near[-1] + int(lengths[-1]) + GAP)


def place(lengths: Sequence[int], unit: int = 1) -> Placement:
    """Seven items: control, then (straddle, behind) for 2^29, 2^30 and 2^31."""
    assert len(lengths) == 7 and all(int(n) >= 2 for n in lengths) and unit >= 1
    far, roles, marks = [CONTROL], ["control"], [0]
    for k, mark in enumerate(MARKS):
        n_s, n_b = int(lengths[1 + 2 * k]), int(lengths[2 + 2 * k])
        at = mark // unit  # the unit that holds element `mark`
        start = at - n_s // 2
        if unit == 1 and start % 2 == 0:
            start -= 1  # an odd offset: never on an 8- or 16-byte boundary
        if unit > 1 and n_s // 2 == 0:
            start = at - 1
        far.append(start), roles.append("straddle"), marks.append(mark)
        end = start + n_s + GAP
        behind = ((end + 3) & ~3) + (k + 1)
        far.append(behind), roles.append("behind"), marks.append(mark)
    return _finish(far, lengths, roles, marks, unit)


def place_behind(length: int, unit: int = 1) -> Placement:
    """Four equal items (a uniform batch): control, then one that starts 1 / 2 / 3 units behind the unit that holds each mark."""
    assert int(length) >= 1 and unit >= 1
    far = [CONTROL] + [mark // unit + k + 1 for k, mark in enumerate(MARKS)]
    return _finish(far, [int(length)] * 4, ["control"] + ["behind"] * 3, [0] + list(MARKS), unit)


def check(p: Placement, size: int = BUFFER_ELEMS) -> None:
    """Every property the GPU tests rely on; raises AssertionError."""
    u = p.unit
    assert len(p.far) == len(p.near) == len(p.lengths) == len(p.roles) == len(p.marks)
    assert p.roles[0] == "control" and p.far[0] == CONTROL
    for o, n, role, mark in zip(p.far, p.lengths, p.roles, p.marks):
        first, end = o * u, (o + n) * u  # in elements
        assert 0 <= first and end <= size, (role, mark, first, end, size)
        if role == "straddle":
            assert first < mark < end, (mark, first, end)  # it holds elements mark - 1 and mark: the wrap lies inside it
            assert u > 1 or o % 2 == 1
        elif role == "behind":
            assert first > mark, (mark, first)
        else:
            assert end < MARKS[0]
    for which in (p.far, p.near):
        spans = sorted(zip(which, p.lengths))
        assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])), "two items overlap"
        assert [o for o, _ in spans] == list(which), "the order changed"
    assert all(a % 4 == b % 4 for a, b in zip(p.far, p.near))
    assert p.near[0] == CONTROL and p.near[-1] + p.lengths[-1] <= p.near_size
    for k, mark in enumerate(MARKS):  # each mark has its item(s), and the items behind the marks cover the three odd alignments
        assert sum(1 for r, m in zip(p.roles, p.marks) if m == mark and r == "behind") == 1
    if u == 1:
        assert sorted(o % 4 for o, r in zip(p.far, p.roles) if r == "behind") == [1, 2, 3]
