"""Edge-shape cases for hipfeat_specaug / hipfeat_global_mvn, shared by tests/test_specaug_edges_reference.py (CPU) and
tests/test_gpu_specaug_edges.py (GPU).

A specaug case is ``(name, x, seg_rounds, masks, claims)``: the input batch, rounds of warp segment records, mask records, and the
geometry the case exists for.  ``claims`` comes from ``geometry``: the launch arithmetic of hipfeat_specaug and the (row, column) walk
of specaug_warp_kernel restated here in Python, never read back from the library.  Builders that exist for one regime also say which
one by hand (``expect``); the CPU module holds the two against each other and simulates the walk.

Data is ``randn * 3 - 8`` like oracle.make_golden_specaug.make_input unless a case says otherwise.
"""
import zlib

import numpy as np

from lhotse_amd._lib import MASK_DTYPE, WARP_SEGMENT_DTYPE

TILE_ELEMS = 8192   # hipfeat_specaug: rows_per_tile = max(1, min(T, 8192 / F))
BLOCK = 256         # lanes of one block of specaug_warp_kernel

# the walk regime every feature dimension of the walk cases stands for, stated by hand
FLOAT4_WALK = {4: "divides", 12: "remainder", 256: "divides", 516: "half", 1020: "half", 1024: "equal", 1028: "wide", 8192: "wide", 8196: "wide"}
SCALAR_WALK = {1: "divides", 2: "divides", 3: "remainder", 5: "remainder", 255: "half", 257: "wide", 513: "wide", 8193: "wide"}
REGIMES = ("remainder", "divides", "equal", "half", "wide")


def geometry(T, F, aligned=True):
    """What hipfeat_specaug launches for a (B, T, F) batch whose buffers are (not) 16-byte aligned."""
    V = 4 if (F % 4 == 0 and aligned) else 1
    FV = F // V
    drr = BLOCK // FV
    dcc = BLOCK - drr * FV
    if FV > BLOCK:
        regime = "wide"        # drr == 0, dcc == 256
    elif FV == BLOCK:
        regime = "equal"       # drr == 1, dcc == 0
    elif dcc == 0:
        regime = "divides"     # FV divides 256
    elif drr == 1:
        regime = "half"        # 128 < FV < 256
    else:
        regime = "remainder"   # FV < 128 with a remainder
    rows_per_tile = max(1, min(T, TILE_ELEMS // F))
    tiles = -(-T // rows_per_tile)
    return dict(T=T, F=F, V=V, FV=FV, route="float4" if V == 4 else "scalar", drr=drr, dcc=dcc, regime=regime, rows_per_tile=rows_per_tile,
                tiles=tiles, last_tile_rows=T - (tiles - 1) * rows_per_tile, lane_trips=-(-rows_per_tile * FV // BLOCK))


def walk(nrows, FV):
    """specaug_warp_kernel's loop over one tile, lane by lane: the (row, column) every trip visits."""
    drr = BLOCK // FV
    dcc = BLOCK - drr * FV
    seen = []
    for lane in range(BLOCK):
        rr = lane // FV
        cc = lane - rr * FV
        i = lane
        while i < nrows * FV:
            if cc >= FV:
                cc -= FV
                rr += 1
            seen.append((rr, cc))
            i, rr, cc = i + BLOCK, rr + drr, cc + dcc
    return seen


def data(name, shape, level=-8.0):
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    return (rng.randn(*shape) * 3.0 + level).astype(np.float32)


def segs(*rows):
    return np.array(list(rows), dtype=WARP_SEGMENT_DTYPE)


def masks_of(*rows):
    return np.array(list(rows), dtype=MASK_DTYPE)


def _case(name, x, seg_rounds, masks, aligned=True, **expect):
    claims = geometry(x.shape[1], x.shape[2], aligned)
    claims["expect"] = expect
    return name, x, seg_rounds, masks, claims


# ---- 1. walk regimes ----------------------------------------------------------------------------------------------------------------
def _walk_case(F, route):
    g = geometry(1, F, route == "float4")
    rpt = max(1, TILE_ELEMS // F)
    T = 2 * rpt + 1
    name = f"walk-{route}-F{F}"
    x = data(name, (2, T, F))
    if rpt == 1:  # T == 3: rows 0 | 1 | 2 are three tiles
        sg = segs((0, 0, 3, 1, 2), (1, 0, 2, 1, 1))                  # astride both boundaries; astride the first, row 2 in no segment
    else:
        a = min(rpt // 2, 20)
        sg = segs((0, rpt - a, 2 * a, a + 1, a - 1), (1, rpt - a, 2 * a, a - 1, a + 1))   # rows [rpt - a, rpt + a): astride row rpt
    lo = F // 3
    hi = min(F, lo + max(1, F // 4))
    mk = [(1, 1, 2 * rpt - min(rpt, 2), 2 * rpt + 1), (1, 2, lo, hi)]  # time mask astride row 2 * rpt (the one-row last tile), a feature mask
    if F >= 2:
        mk.append((0, 2, lo, hi))
    expect = dict(route=route, regime=(FLOAT4_WALK if route == "float4" else SCALAR_WALK)[F], last_tile_rows=1, tiles=3)
    assert g["route"] == route
    return _case(name, x, [sg], masks_of(*mk), aligned=True, **expect)


def walk_cases():
    return [_walk_case(F, "float4") for F in FLOAT4_WALK] + [_walk_case(F, "scalar") for F in SCALAR_WALK]


# ---- 2. base alignment --------------------------------------------------------------------------------------------------------------
ALIGN_OFFSETS = [(0, 0), (1, 0), (0, 3), (1, 3)]  # (input, output) offsets in floats from a 16-byte boundary


def alignment_case(F, in_off, out_off):
    """The same batch and descriptors for every offset pair: only the route differs."""
    T = 2 * (TILE_ELEMS // F) + 5
    x = data(f"align-F{F}", (2, T, F))
    sg = segs((0, 3, T - 6, T // 2, T // 2 - 5), (1, 0, T, T // 3, T // 3 + 4))
    mk = masks_of((0, 1, 7, 11), (0, 2, F - 9, F), (1, 2, 0, 5), (1, 1, T - 2, T))
    aligned = in_off % 4 == 0 and out_off % 4 == 0
    return _case(f"align-F{F}-in{in_off}-out{out_off}", x, [sg], mk, aligned=aligned, route="float4" if aligned else "scalar")


def alignment_cases():
    return [alignment_case(F, i, o) for F in (80, 1028) for i, o in ALIGN_OFFSETS]


# ---- 3. extreme segments ------------------------------------------------------------------------------------------------------------
def extreme_cases():
    out = []

    def add(name, shape, *rows, **expect):
        out.append(_case(name, data(name, shape), [segs(*rows)], masks_of(), **expect))

    add("seg-two-rows", (1, 10, 12), (0, 4, 2, 1, 1))
    add("seg-center1-warped-max", (1, 3004, 12), (0, 2, 3000, 1, 2999))      # a one-row source under 2999 output rows, 2999 rows under one
    add("seg-center-max-warped1", (1, 3004, 12), (0, 2, 3000, 2999, 1))
    add("seg-three-rows", (2, 9, 12), (0, 1, 3, 2, 1), (1, 5, 3, 1, 2))
    add("seg-whole-sequence", (1, 100, 12), (0, 0, 100, 40, 55))
    add("seg-ends-at-T", (1, 100, 12), (0, 30, 70, 30, 20))
    add("seg-touching", (1, 100, 12), (0, 10, 30, 10, 15), (0, 40, 25, 12, 9))
    # F = 80: 102 rows per tile; [102, 162) begins on the first boundary, [150, 204) of the other sequence ends on the second
    add("seg-on-tile-boundaries", (2, 250, 80), (0, 102, 60, 20, 31), (1, 150, 54, 30, 22), rows_per_tile=102)
    forty = [(0, 5 * i + (i % 2), 4, 1 + i % 3, 1 + (i // 3) % 3) for i in range(40)]  # gaps of one or no row between them, none in sequence 1
    add("seg-forty-in-one-sequence", (2, 203, 12), *forty)
    add("seg-3000-rows", (2, 3000, 12), (0, 0, 3000, 1500, 1420), (1, 0, 3000, 1500, 1580), tiles=5)
    return out


IDENTITY_LENGTHS = (2, 103, 1000)


def identity_case(n):
    """warped == center: scale 1, t == 0, weights (0, 1, 0, 0): the segment's bits come back."""
    name = f"seg-identity-n{n}"
    return _case(name, data(name, (1, n + 7, 12)), [segs((0, 5, n, max(1, n // 3), max(1, n // 3)))], masks_of())


# ---- 4. three rounds ----------------------------------------------------------------------------------------------------------------
def rounds_case():
    name = "three-rounds"
    x = data(name, (3, 300, 40))
    r0 = segs((0, 0, 200, 80, 95), (1, 10, 100, 40, 31), (2, 0, 300, 150, 120))
    r1 = segs((0, 100, 200, 90, 70), (1, 50, 200, 100, 117))
    r2 = segs((0, 50, 180, 60, 75), (1, 0, 300, 33, 20))
    mk = masks_of((0, 1, 40, 70), (0, 2, 3, 9), (1, 2, 30, 40), (1, 1, 290, 300), (1, 1, 0, 4))
    return _case(name, x, [r0, r1, r2], mk)


# ---- 5. masks -----------------------------------------------------------------------------------------------------------------------
def mask_cases():
    out = []

    def add(name, shape, sg, *rows, **expect):
        out.append(_case(name, data(name, shape), [segs(*sg)], masks_of(*rows), **expect))

    T, F = 50, 20
    one = [(0, 5, 40, 20, 14)]
    add("mask-end-beyond", (1, T, F), one, (0, 1, 40, T + 5), (0, 2, 15, F + 5))
    add("mask-begin-at-size", (1, T, F), one, (0, 1, T, T + 3), (0, 2, F, F + 2))
    add("mask-begin-at-size-and-a-real-one", (1, T, F), one, (0, 1, T, T), (0, 2, F, F), (0, 1, 3, 9))
    add("mask-empty", (1, T, F), one, (0, 1, 10, 10), (0, 2, 5, 5))
    add("mask-empty-and-a-real-one", (1, T, F), one, (0, 1, 10, 10), (0, 2, 5, 5), (0, 2, 6, 8))
    add("mask-all-rows", (2, T, F), one + [(1, 0, T, 30, 22)], (0, 1, 0, T), (1, 1, 0, T + 5))
    add("mask-features-only", (2, T, F), one, (0, 2, 0, 3), (0, 2, 17, F), (1, 2, 9, 10))
    add("mask-columns-second-trip", (2, 30, 700), [(0, 2, 20, 8, 13)], (0, 2, 250, 600), (1, 2, 250, 600), (1, 1, 4, 6))
    add("mask-rows-second-trip", (2, 1025, 16), [(0, 100, 600, 300, 280)], (0, 1, 200, 500), (1, 1, 200, 500), (1, 2, 3, 5),
        rows_per_tile=512, last_tile_rows=1)
    return out


def between_case():
    """Sequence 1 has no masks, its neighbours do: it must equal the warp-only run bit for bit."""
    name = "mask-none-between-two"
    x = data(name, (3, 120, 24))
    sg = segs((0, 0, 120, 50, 60), (1, 10, 100, 40, 52), (2, 20, 80, 30, 21))
    mk = masks_of((0, 1, 10, 30), (0, 2, 4, 9), (2, 2, 0, 24), (2, 1, 100, 110))
    return _case(name, x, [sg], mk)


# ---- 6. which mean ------------------------------------------------------------------------------------------------------------------
def mean_cases():
    out = []
    name = "mean-three-levels"   # the batch mean is nowhere near any sequence's
    x = np.concatenate([data(name + str(lv), (1, 150, 24), level=lv) for lv in (-8.0, 50.0, -300.0)], axis=0)
    sg = segs((0, 0, 150, 70, 60), (1, 5, 100, 50, 61), (2, 40, 110, 50, 44))
    mk = masks_of((0, 1, 20, 40), (0, 2, 5, 8), (1, 1, 100, 130), (1, 2, 0, 4), (2, 1, 0, 10), (2, 2, 20, 24))
    out.append(_case(name, x, [sg], mk))
    name = "mean-moves-with-the-warp"   # 100 rows of 0 and 100 rows of 100, the first half squeezed into 30 rows: the mean goes from 50 to 85
    x = np.zeros((1, 200, 8), dtype=np.float32)
    x[0, 100:] = 100.0
    x += data(name, x.shape, level=0.0) * np.float32(0.01)
    out.append(_case(name, x, [segs((0, 0, 200, 100, 30))], masks_of((0, 1, 10, 20), (0, 2, 6, 8), (0, 1, 150, 160))))
    name = "mean-counts-the-masked-rows"   # the masked rows lie 48 above the rest: a mean of the unmasked part is 8 lower
    x = data(name, (1, 120, 16))
    x[0, 50:70] += np.float32(48.0)
    out.append(_case(name, x, [segs((0, 0, 40, 20, 25))], masks_of((0, 1, 50, 70))))
    return out


def all_cases():
    return (walk_cases() + alignment_cases() + extreme_cases() + [identity_case(n) for n in IDENTITY_LENGTHS] + [rounds_case()] + mask_cases()
            + [between_case()] + mean_cases())


def resample_pairs(cases):
    """Every (in_len, out_len) that the cases hand to the bicubic resampler."""
    pairs = set()
    for _, _, seg_rounds, _, _ in cases:
        for rnd in seg_rounds:
            for s in rnd:
                n, c, w = int(s["num_frames"]), int(s["center"]), int(s["warped"])
                pairs.add((c, w))
                pairs.add((n - c, n - w))
    return sorted(pairs)


def regions(x, seg_rounds, masks):
    """(in_segment[B, T], masked[B, T, F]) as booleans, with the kernel's clamping of mask ends."""
    B, T, F = x.shape
    in_seg = np.zeros((B, T), dtype=bool)
    for rnd in seg_rounds:
        for s in rnd:
            in_seg[int(s["sequence"]), int(s["start"]) : int(s["start"]) + int(s["num_frames"])] = True
    masked = np.zeros((B, T, F), dtype=bool)
    for m in masks:
        b, lo, hi = int(m["sequence"]), int(m["begin"]), int(m["end"])
        if int(m["axis"]) == 1:
            masked[b, lo:hi, :] = True
        else:
            masked[b, :, lo:hi] = True
    return in_seg, masked


# ---- 8. GlobalMVN -------------------------------------------------------------------------------------------------------------------
F32_MAX = np.finfo(np.float32).max
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, F32_MAX, -F32_MAX, 1e-40, -1e-45, 1.1754942e-38, 1e-30, -1e-30, 3e38], dtype=np.float32)


def _mvn_stats(F, rng, shift=0):
    """Column kinds, cycling: std 0 | negative | inf | mean 0 with a huge std (subnormal quotients of the 1e-30 entries) | mean 0 with a
    tiny std (subnormal products) | three ordinary ones."""
    means = (rng.randn(F) - 7).astype(np.float32)
    stds = (rng.rand(F) * 3 + 0.5).astype(np.float32)
    for c in range(F):
        kind = (c + shift) % 8
        if kind == 0:
            stds[c] = 0.0
        elif kind == 1:
            stds[c] = -stds[c]
        elif kind == 2:
            stds[c] = np.inf
        elif kind == 3:
            means[c], stds[c] = 0.0, 3e9
        elif kind == 4:
            means[c], stds[c] = -0.0, 7e-10   # (-0 * s + -0 keeps its sign)
    return means, stds


def mvn_cases():
    """(name, x[rows, F], means, stds); a third of x is drawn from SPECIALS."""
    out = []
    shapes = [(1, 1, s) for s in range(6)] + [(64, 1, s) for s in range(6)] + [(1, 3, 0), (50, 3, 0), (50, 3, 3), (1, 80, 0), (37, 80, 0), (1, 257, 0), (8161, 257, 0)]
    for rows, F, shift in shapes:
        name = f"mvn-{rows}x{F}-k{shift}"
        rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
        x = (rng.randn(rows, F) * 4 - 6).astype(np.float32)
        pick = rng.rand(rows, F) < 1.0 / 3.0
        x[pick] = SPECIALS[rng.randint(0, len(SPECIALS), size=int(pick.sum()))]
        means, stds = _mvn_stats(F, rng, shift)
        out.append((name, x, means, stds))
    return out


def same_bits_nan_by_position(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
