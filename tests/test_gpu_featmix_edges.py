"""GPU: the feature-mix launches (csrc/kernel_featmix.hpp) at their tile, group and block edges: the cases of tests/_featmix_cases.py, whose
geometry tests/test_featmix_edges_reference.py pins on the CPU.

``out`` is a slice at element ``GUARD + out_offset`` (out_offset 0 ... 3) of a tensor poisoned with 0x5A5A5A5A, so that a row starts 0 ... 3
elements behind a 16-byte boundary; every element outside the slice and the whole arena must come back untouched, and ``info[2]`` /
``info[3]`` of the plan must be the energy and fold items the case claims.

Per case, over EVERY element of every row: copy-form rows bit-equal to the numpy statement; every element outside a cut's frames bit-equal
to float32(log(1e-10)); fold-form elements within ``R.bar(truth) + R.carried(cut)`` of the float64 truth (tests/_featmix_ref.py: the
derived bound, no new tolerance).  And without a tolerance: the repeated frame is bit-equal to the frame in front of it; every row of a
batch is bit-equal to its cut run alone (B = 1, the same row length, an out_offset that gives it the same head); the runs at all of the
case's out_offsets are bit-equal; so is a second run.  For the batch of 2048 energy items each cut alone plans 256, so its bits against
the batch's row are the check on a workgroup's second energy item.

Measured on an MI355X, per group the fold element closest to its bound, |out - truth| / bound there:
    rep     7.08e-08 / 3.06e-07  (rep_fold_F257_254)        rowlen  1.64e-07 / 3.65e-07  (rowlen_8191)
    sweep   1.38e-07 / 3.65e-07  (sweep_F1_head2)           energy  1.35e-07 / 3.65e-07  (energy_F64_257_f16)
    trip    5.54e-08 / 1.16e-06  (2048 energy items, 8 fold items as planned; each cut alone 256 and 1)
    tables  1.31e-07 / 3.59e-07  (the reference of 3 partials in 256 tracks: 258 energy items, 10 fold items)
Time (pytest's own): this module alone 2.6 s (53 cases; the slowest, 0.18 s, is the first launch of the process); with
tests/test_gpu_stats_edges.py in one process 3.2 s.  The GPU suite: 1016 tests in 201.7 s, the parent's 946 tests in 194.5 s.
"""
import numpy as np
import pytest
import torch

import _featmix_cases as C
import _featmix_ref as R

from lhotse_amd import augmentation as A
from lhotse_amd.augmentation import FEATMIX_COPY as COPY

pytestmark = pytest.mark.gpu
GUARD = 64
POISON = 0x5A5A5A5A
LOG_EPS_BITS = np.float32(R.LOG_EPSILON).view(np.uint32)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(d_arena, host, cuts, F, row_frames, out_offset, claims=None):
    """One plan and one run into ``whole[GUARD + out_offset:]`` -> the (B, T, F) result as numpy."""
    lay = A.featmix_layout(len(host), cuts, F, row_frames)
    B, T = len(cuts), lay["row_frames"]
    n = B * T * F
    whole = torch.full((GUARD + 4 + n + GUARD,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    assert whole.data_ptr() % 16 == 0 and GUARD % 4 == 0
    out = whole[GUARD + out_offset: GUARD + out_offset + n]
    mixer = A.get_or_create_featmixer("cuda")
    ticket, info = mixer.plan(lay)
    mixer.run(ticket, d_arena, out)
    torch.cuda.synchronize()
    if claims is not None:
        assert [int(info[2]), int(info[3])] == [claims["energy_items"], claims["fold_items"]], (info, claims["energy_items"], claims["fold_items"])
    bits = whole.view(torch.int32).cpu().numpy()
    assert (bits[: GUARD + out_offset] == POISON).all() and (bits[GUARD + out_offset + n:] == POISON).all(), "an element outside out was written"
    assert np.array_equal(d_arena.cpu().numpy(), host), "the arena was written"
    return bits[GUARD + out_offset: GUARD + out_offset + n].view(np.float32).reshape(B, T, F).copy()


def check(case, got, truth):
    """Every element of every row against the statement -> (worst fold error, the bound there)."""
    worst = (0.0, 0.0, -np.inf)
    for b, c in enumerate(case.cuts):
        want32 = truth[b].astype(np.float32)
        if c.form == COPY:
            assert np.array_equal(u32(got[b]), u32(want32)), (case.name, b)
            continue
        inside = np.zeros(case.row_frames, dtype=bool)
        inside[c.dst_first: c.dst_first + c.num_frames] = True
        assert (u32(got[b][~inside]) == LOG_EPS_BITS).all(), (case.name, b, "outside the cut's frames")
        if not inside.any():
            continue
        err = np.abs(got[b][inside].astype(np.float64) - truth[b][inside])
        bound = R.bar(truth[b][inside]) + R.carried(c)[:, None]
        k = int(np.argmax(err - bound))
        if (err - bound).ravel()[k] > worst[2]:
            worst = (float(err.ravel()[k]), float(bound.ravel()[k]), float((err - bound).ravel()[k]))
        assert (err <= bound).all(), (case.name, b, err.ravel()[k], bound.ravel()[k])
    return worst[:2]


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_case(case):
    F, T, host = case.F, case.row_frames, case.host
    d_arena = torch.from_numpy(host).cuda()
    geo = {o: C.geometry(case.cuts, F, T, o) for o in range(4)}
    first = case.offsets[0]
    got = run(d_arena, host, case.cuts, F, T, first, geo[first])
    err, bound = check(case, got, R.batch(host, case.cuts, F, T))
    print(f"[featmix edges] {case.group} {case.name}: energy items {geo[first]['energy_items']}, fold items {geo[first]['fold_items']}, "
          f"worst fold |out - truth| = {err:.3e} (bound there {bound:.3e})")
    # the repeated frame is the frame in front of it, bit for bit
    for b, (c, r) in enumerate(zip(case.cuts, geo[first]["rows"])):
        if r["rep"] is not None:
            last = c.dst_first + c.num_frames - 1
            assert r["rep"] == last * F and np.array_equal(u32(got[b][last]), u32(got[b][last - 1])), (case.name, b)
    # a second run, and the other out_offsets: the same bits
    assert np.array_equal(u32(run(d_arena, host, case.cuts, F, T, first, geo[first])), u32(got)), (case.name, "two runs differ")
    for o in case.offsets[1:]:
        assert np.array_equal(u32(run(d_arena, host, case.cuts, F, T, o, geo[o])), u32(got)), (case.name, "out_offset", o)
    # every row is its cut run alone at the same head
    if len(case.cuts) > 1:
        for b, (c, r) in enumerate(zip(case.cuts, geo[first]["rows"])):
            alone = run(d_arena, host, [c], F, T, r["head"], C.geometry([c], F, T, r["head"]))
            assert np.array_equal(u32(alone[0]), u32(got[b])), (case.name, "row", b, "differs from its cut run alone")
