"""CPU: the ground under tests/test_gpu_specaug_edges.py.

1. the geometry every edge case claims (route, walk regime, rows per tile, tiles, rows of the last tile, lane-loop trips) is what the
   launch arithmetic of hipfeat_specaug gives for its shape, the cases cover every regime, and specaug_warp_kernel's carry walk -- restated
   in tests/_specaug_cases.py -- visits every (row, column) of a tile exactly once in each of them;
2. oracle.specaug_ref.bicubic_rows is torch's F.interpolate(mode="bicubic", align_corners=False) at every (in_len, out_len) the cases use,
   at the bar of tests/test_specaug_oracle.py::test_bicubic_rows_is_torch_interpolate;
3. resampling to the same length returns the input's bits;
4. oracle.specaug_ref.global_mvn is torch's two CPU ops bit for bit on the non-finite / subnormal inputs, NaNs position for position."""
import numpy as np
import pytest
import torch

import _specaug_cases as C
from oracle import specaug_ref as R

CASES = C.all_cases()
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_claims_hold(case):
    name, x, seg_rounds, masks, claims = case
    B, T, F = x.shape
    assert B <= 3 and x.dtype == np.float32
    assert claims["T"] == T and claims["F"] == F
    V, FV = claims["V"], claims["FV"]
    assert (claims["route"] == "float4") == (V == 4) and FV * V == F and (V == 1 or F % 4 == 0)
    # the regime is a statement about (drr, dcc)
    drr, dcc = claims["drr"], claims["dcc"]
    assert drr * FV + dcc == 256 and 0 <= dcc < max(FV, 257)
    assert {
        "wide": drr == 0 and dcc == 256 and FV > 256,
        "equal": drr == 1 and dcc == 0 and FV == 256,
        "divides": dcc == 0 and FV < 256 and 256 % FV == 0,
        "half": drr == 1 and 0 < dcc and 128 < FV < 256,
        "remainder": drr >= 2 and 0 < dcc < FV,
    }[claims["regime"]], claims
    rpt, tiles = claims["rows_per_tile"], claims["tiles"]
    assert 1 <= rpt <= T and (rpt * F <= 8192 or rpt == 1) and ((rpt + 1) * F > 8192 or rpt == T)
    assert (tiles - 1) * rpt < T <= tiles * rpt and claims["last_tile_rows"] == T - (tiles - 1) * rpt >= 1
    assert (claims["lane_trips"] - 1) * 256 < rpt * FV <= claims["lane_trips"] * 256
    for key, value in claims["expect"].items():  # what the builder says the case is for
        assert claims[key] == value, (name, key, claims[key], value)
    # descriptors are what hipfeat_specaug accepts: segments inside the sequence, none overlapping within a round
    for rnd in seg_rounds:
        for s in rnd:
            n = int(s["num_frames"])
            assert 0 <= s["sequence"] < B and s["start"] >= 0 and n >= 2 and s["start"] + n <= T and 1 <= s["center"] < n and 1 <= s["warped"] < n
        for b in range(B):
            spans = sorted((int(s["start"]), int(s["start"]) + int(s["num_frames"])) for s in rnd if s["sequence"] == b)
            assert all(a[1] <= b_[0] for a, b_ in zip(spans, spans[1:])), (name, spans)
    for m in masks:
        assert 0 <= m["sequence"] < B and m["axis"] in (1, 2) and 0 <= m["begin"] <= m["end"]


def test_the_cases_cover_every_regime():
    by_name = {c[0]: c[4] for c in CASES}
    walk = [c[4] for c in C.walk_cases()]
    assert {g["regime"] for g in walk if g["route"] == "float4"} == set(C.REGIMES)
    assert {g["F"] for g in walk if g["route"] == "float4"} == {4, 12, 256, 516, 1020, 1024, 1028, 8192, 8196}
    assert {g["F"] for g in walk if g["route"] == "scalar"} == {1, 2, 3, 5, 255, 257, 513, 8193}
    assert any(g["route"] == "scalar" and g["regime"] == "wide" for g in walk)
    for g in walk:
        assert g["T"] == 2 * g["rows_per_tile"] + 1 and g["tiles"] == 3 and g["last_tile_rows"] == 1 and g["lane_trips"] >= 2, g
    assert by_name["walk-float4-F8192"]["rows_per_tile"] == 1 and 8192 // 8192 == 1      # one row fills the tile
    assert by_name["walk-float4-F8196"]["rows_per_tile"] == 1 and 8192 // 8196 == 0      # the clamp to one row
    assert by_name["walk-scalar-F8193"]["rows_per_tile"] == 1
    assert any(g["rows_per_tile"] > 256 for g in walk) and by_name["mask-rows-second-trip"]["rows_per_tile"] == 512
    assert max(x.size for _, x, _, _, _ in C.walk_cases()) == 2 * 3 * 8196 and max(x.size for _, x, _, _, _ in CASES) <= 1 << 17
    # a multiple-of-4 feature dimension on the scalar route, in two walk regimes
    assert {(g["F"], g["route"]) for g in (c[4] for c in C.alignment_cases())} == {(80, "float4"), (80, "scalar"), (1028, "float4"), (1028, "scalar")}
    assert by_name["align-F1028-in1-out0"]["regime"] == "wide" and by_name["align-F1028-in0-out0"]["regime"] == "wide"
    assert by_name["align-F80-in0-out3"]["regime"] == "remainder" and by_name["align-F80-in0-out0"]["regime"] == "remainder"
    # segment boundaries on tile boundaries
    g = by_name["seg-on-tile-boundaries"]
    sg = {int(s["sequence"]): s for s in dict((c[0], c[2]) for c in CASES)["seg-on-tile-boundaries"][0]}
    assert sg[0]["start"] % g["rows_per_tile"] == 0 and (sg[1]["start"] + sg[1]["num_frames"]) % g["rows_per_tile"] == 0


@pytest.mark.parametrize("FV", sorted({c[4]["FV"] for c in CASES} | {128, 129, 255, 256, 257}))
def test_the_carry_walk_visits_every_element_once(FV):
    """One carry per trip is enough in every regime: the restated loop of specaug_warp_kernel enumerates the tile exactly."""
    for nrows in {1, 2, 3, -(-700 // FV), -(-700 // FV) + 1}:
        seen = C.walk(nrows, FV)
        assert sorted(seen) == [(r, c) for r in range(nrows) for c in range(FV)], (FV, nrows)


PAIRS = sorted(set(C.resample_pairs(CASES)) | {(1, 1), (2, 1), (1, 2), (1, 2999), (2999, 1), (1, 7), (7, 1)})


def test_the_pairs_include_the_degenerate_ones():
    used = set(C.resample_pairs(CASES))
    assert {(1, 1), (2, 1), (1, 2), (1, 2999), (2999, 1), (1500, 1420), (1500, 1580)} <= used
    assert any(i == 1 and o > 1 for i, o in used) and any(o == 1 and i > 1 for i, o in used)


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{i}-to-{o}" for i, o in PAIRS])
def test_bicubic_rows_is_torch_interpolate_at_the_new_shapes(pair):
    in_len, out_len = pair
    x = C.data(f"pair-{in_len}-{out_len}", (in_len, 7))
    ref = torch.nn.functional.interpolate(torch.from_numpy(x)[None, None], size=(out_len, 7), mode="bicubic", align_corners=False)[0, 0].numpy()
    got = R.bicubic_rows(x, out_len)
    assert np.abs(got - ref).max() <= 5e-6 * max(1.0, np.abs(ref).max()), (pair, np.abs(got - ref).max())


@pytest.mark.parametrize("n", [1, 2, 3, 103, 1000, 3000])
def test_bicubic_rows_to_the_same_length_is_the_identity(n):
    x = C.data(f"identity-{n}", (n, 12))
    assert np.array_equal(R.bicubic_rows(x, n).view(np.uint32), x.view(np.uint32))
    if n >= 2:  # and so is a whole warp with warped == center
        assert np.array_equal(R.time_warp(x, max(1, n // 3), max(1, n // 3)).view(np.uint32), x.view(np.uint32))


MVN = C.mvn_cases()


@pytest.mark.parametrize("case", MVN, ids=[c[0] for c in MVN])
def test_global_mvn_restatement_is_torch_bit_for_bit(case):
    name, x, means, stds = case
    tx, tm, ts = (torch.from_numpy(a) for a in (x, means, stds))
    with np.errstate(all="ignore"):
        fwd, inv = R.global_mvn(x, means, stds), R.global_mvn(x, means, stds, inverse=True)
    assert C.same_bits_nan_by_position(fwd, ((tx - tm) / ts).numpy())
    assert C.same_bits_nan_by_position(inv, (tx * ts + tm).numpy())


def test_the_mvn_inputs_reach_the_edges():
    """NaN, both infinities and subnormal quotients / products do come out of the reference on these inputs."""
    F = {c[1].shape[1] for c in MVN}
    assert F == {1, 3, 80, 257} and any(c[1].shape[0] == 1 for c in MVN)
    assert any(c[1].size > 8192 * 256 for c in MVN)  # a second grid-stride trip of global_mvn_kernel (8192 blocks of 256 lanes)
    tiny = np.finfo(np.float32).tiny
    for name, x, means, stds in MVN:
        if x.shape[0] < 37 or x.shape[1] < 8:  # (fewer than 8 columns hold only some of the kinds of _mvn_stats)
            continue
        with np.errstate(all="ignore"):
            fwd, inv = R.global_mvn(x, means, stds), R.global_mvn(x, means, stds, inverse=True)
        for y in (fwd, inv):
            assert np.isnan(y).any() and np.isposinf(y).any() and np.isneginf(y).any(), name
            assert ((np.abs(y) > 0) & (np.abs(y) < tiny)).any(), name
            assert (np.signbit(y) & (y == 0)).any(), name
        assert (stds == 0).any() and (stds < 0).any() and np.isinf(stds).any()
