"""CPU: the cases of tests/_featmix_cases.py are what they claim to be.  Every claim (tiles per row, lo / hi / rep of every cut, energy items
per track, total energy and fold items) is held to ``build_featmix_plan`` / ``fm_tiles`` through tests/native/featmix_tables_capi.cpp, the
literals of every case to the restated geometry, and the set as a whole to the list of paths it was built to enter -- so that a case
cannot drift out of its regime unnoticed.  The float32 model of the launch stays within the derived bar of the float64 truth on every
fold-form cut: the bar is reachable by the arithmetic it allows.

One condition of the list cannot hold as it was first worded: a row that starts 3 elements behind a 16-byte boundary never has a planned
tile without an element (``fm_tiles`` plans a further tile from row_len = 4096 k - 2 on, and 3 + 4096 k - 2 > 4096 k); "planned but empty"
is therefore asserted for the heads 0, 1 and 2, and "never" for head 3."""
import numpy as np
import pytest

import _featmix_cases as C
import _featmix_ref as R

from lhotse_amd import augmentation as A
from lhotse_amd.augmentation import FEATMIX_COPY as COPY, FEATMIX_FOLD as FOLD

from test_featmix_abi import OK, raw_plan, shim  # noqa: F401  (shim: the module-scoped fixture that builds the C entry points)
from test_gpu_mix import MAX_WORKGROUPS  # 1792, pinned to items_grid (csrc/hipfeat.hip) by tests/test_mix_abi.py

BY_GROUP = {g: [c for c in C.CASES if c.group == g] for g in ("rep", "rowlen", "sweep", "energy", "trip", "tables")}


def geometries(cases):
    """(case, out_offset, geometry) of every run of the cases."""
    return [(c, o, C.geometry(c.cuts, c.F, c.row_frames, o)) for c in cases for o in c.offsets]


def test_the_case_names_are_unique_and_every_group_has_cases():
    assert len({c.name for c in C.CASES}) == len(C.CASES) and all(BY_GROUP.values())
    assert all(set(c.offsets) <= {0, 1, 2, 3} and set(c.expect) <= set(c.offsets) for c in C.CASES)
    assert max(len(c.host) for c in C.CASES) < 1 << 20  # the largest arena: the two tracks of 49153 elements


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_every_claim_is_what_the_plan_says(shim, case):  # noqa: F811
    assert shim.ft_tile() == C.TILE == A.FEATMIX_TILE and shim.ft_energy_block() == C.ENERGY_BLOCK == A.FEATMIX_ENERGY_BLOCK
    lay = A.featmix_layout(len(case.host), case.cuts, case.F, case.row_frames)
    st, info, ct, tt, msg = raw_plan(shim, lay)
    assert st == OK, msg
    F = case.F
    for o in case.offsets:
        g = C.geometry(case.cuts, F, case.row_frames, o)
        for key, want in case.expect.get(o, {}).items():  # the literals the case was built for
            assert C.claim(g, key) == want, (case.name, o, key, C.claim(g, key), want)
        assert g["tiles"] == shim.ft_tiles(case.row_frames * F) and g["row_len"] == case.row_frames * F
        assert [g["energy_items"], g["fold_items"]] == info[2:].tolist(), (case.name, g["energy_items"], g["fold_items"], info)
        assert [e for r in g["rows"] for e in r["energy"]] == tt["part_count"].tolist()
        for r, cd, c in zip(g["rows"], ct, case.cuts):
            assert r["lo"] == cd["dst_first"] * F and r["hi"] == r["lo"] + cd["num_frames"] * F
            if c.form == FOLD:  # (the kernel's own rule: one frame more than the mix)
                assert r["rep"] == (r["lo"] + cd["mix_frames"] * F if cd["num_frames"] > cd["mix_frames"] else None)
            else:
                t = tt[cd["track_first"]]
                assert r["rep"] == (r["lo"] + t["rows"] * F if t["src_off"] >= 0 and 0 < t["rows"] < t["frames"] else None)
            assert 0 <= r["head"] < 4 and (r["tile_hi"] is None or r["tile_hi"] < g["tiles"])
            # the tiles cover the row, and the last one holds an element at the largest head (the kernel's skip is the only empty one)
            assert g["tiles"] * C.TILE >= r["head"] + g["row_len"] and r["last_tile"] <= C.TILE and (r["head"] < 3 or r["last_tile"] >= 1)


def test_the_repeated_and_the_dropped_frame_lie_on_every_side_of_a_tile_boundary():
    gs = geometries(BY_GROUP["rep"])
    for form in (FOLD, COPY):
        mine = [(c, o, g["rows"][0]) for c, o, g in gs if c.cuts[0].form == form and g["rows"][0]["rep"] is not None]
        behind23 = {r["rep_behind"] for c, o, r in mine if c.F == 23 and r["rep"] == 4094}
        assert behind23 == {21, 22, 23, 0}  # the second tile starts 2, 1 and 0 elements behind rep, and 1 in front of it
        # exactly one element of the repeated frame, its last bin, is all the second tile holds
        assert any(r["rep_behind"] == 1 and r["last_tile"] == 1 and c.F == 23 for c, o, r in mine)
        assert any(c.F == 1 and r["rep_behind"] == 1 for c, o, r in mine) and any(c.F == 1 and r["rep_behind"] == 0 and r["tile_rep"] == 1 for c, o, r in mine)
        assert any(c.F == 257 and 0 < r["rep_behind"] < 257 for c, o, r in mine)
        # F = 257: the repeated frame ends ON a boundary (the tile behind it is planned and empty), one frame in front of which rep lies
        assert any(c.F == 257 and (r["head"] + r["rep"] + 257) % C.TILE == 0 and r["last_tile"] == 0 for c, o, r in mine)
    # two tracks: the long one ends at rep, the short one more than F elements in front of the first tile that starts at or behind rep
    reached = 0
    for c, o, g in gs:
        cut, r = c.cuts[0], g["rows"][0]
        if cut.form == FOLD and r["rep"] is not None and r["rep_behind"] > 0:
            start = min(t * C.TILE - r["head"] for t in range(g["tiles"]) if t * C.TILE - r["head"] >= r["rep"])
            ends = [r["lo"] + (t.first + t.frames) * c.F for t in cut.tracks]
            assert ends[0] == r["rep"] and ends[1] < start - c.F
            reached += 1
    assert reached >= 8
    drops = [(o, g["rows"][0]) for c, o, g in gs if c.name.startswith("drop_")]
    assert all(r["rep"] is None for o, r in drops) and {(r["head"] + r["hi"]) // C.TILE for o, r in drops if r["hi"] == 4094} == {0, 1}
    assert {r["tile_hi"] for o, r in drops} == {0, 1}


def test_row_lengths_put_the_row_end_on_every_side_of_a_tile_for_every_head():
    gs = geometries(BY_GROUP["rowlen"])
    assert {c.row_frames for c, o, g in gs} == set(C.ROW_FRAMES) and all(c.F == 1 and len(c.cuts) == 3 for c, o, g in gs)
    assert all([cut.form for cut in c.cuts] == [FOLD, COPY, COPY] and c.cuts[2].num_frames == 0 for c, o, g in gs)
    rows = [(g["row_len"], r) for c, o, g in gs for r in g["rows"]]
    assert {(n, r["head"]) for n, r in rows} == {(n, h) for n in C.ROW_FRAMES for h in range(4)}  # every length at every head
    assert {r["head"] + n for n, r in rows} >= {4095, 4096, 4097, 4098, 8191, 8192, 8193, 8194}
    empty = {(r["head"], n) for n, r in rows if r["last_tile"] <= 0}
    assert {h for h, n in empty} == {0, 1, 2} and {n for h, n in empty} == {4094, 4095, 4096, 8191, 8192}  # planned, no element (head 3: never)
    assert {(r["head"], r["last_tile"]) for n, r in rows if 1 <= r["last_tile"] <= 3} >= {(1, 1), (2, 1), (3, 1), (2, 2), (3, 2), (3, 3)}  # nothing but a scalar tail
    assert any(r["head"] == 3 and n == 4093 and r["last_tile"] == C.TILE for n, r in rows)  # one tile, full to its last element
    # without the "+ 3" of fm_tiles ((row_len - 1) // 4096 + 1 tiles) these rows would lose their last elements
    assert any((n - 1) // C.TILE + 1 < (r["head"] + n + C.TILE - 1) // C.TILE for n, r in rows)


def test_the_sweep_puts_lo_and_hi_on_every_side_of_a_group_and_of_a_tile():
    gs = geometries(BY_GROUP["sweep"])
    for head in range(4):
        edge = C.TILE - head
        one = [r for c, o, g in gs if c.F == 1 and o == head for r in g["rows"]]
        assert all(r["head"] == head for r in one)
        assert {r["lo"] for r in one} >= {0, 1, 3, 4, 5, edge - 1, edge, edge + 1} and {r["hi"] for r in one} >= {edge - 1, edge, edge + 1}
        assert {r["hi"] - r["lo"] for r in one if r["lo"] in (0, 1, 3, 4, 5, edge - 1, edge, edge + 1)} >= set(C.SWEEP_LENGTHS)
        assert {(head + r["lo"]) % 4 for r in one} == {(head + r["hi"]) % 4 for r in one} == {0, 1, 2, 3}
        assert {(r["tile_lo"], r["tile_hi"]) for r in one} == {(0, 0), (0, 1), (1, 1)}
        three = [r for c, o, g in gs if c.F == 3 and o == head for r in g["rows"]]
        assert all(r["head"] == head and r["lo"] % 3 == 0 for r in three)
        assert any(edge - 2 <= r["lo"] < edge for r in three) or any(r["lo"] == edge for r in three)
        assert {(r["tile_lo"], r["tile_hi"]) for r in three} == {(0, 0), (0, 1), (1, 1)}
        assert {(r["hi"] - r["lo"]) // 3 for r in three} >= set(C.SWEEP_LENGTHS)
    near = {r["lo"] - (C.TILE - r["head"]) for c, o, g in gs if c.F == 3 for r in g["rows"]} & set(range(-2, 3))
    assert near == {-2, -1, 0, 1, 2}  # over the four heads, lo = 3 * dst_first lies at every distance from the boundary


def test_the_energy_cases_lie_on_every_side_of_a_block():
    gs = geometries(BY_GROUP["energy"])
    sizes = {(c.F, c.cuts[0].tracks[1].frames * c.F, bool(c.cuts[0].tracks[1].f16)) for c, o, g in gs}
    for n in (16383, 16384, 16385, 32768, 32769, 49153):
        assert (1, n, False) in sizes and (1, n, True) in sizes
    assert {n for F, n, h in sizes if F == 64} == {256 * 64, 257 * 64, 512 * 64}
    assert {g["rows"][0]["energy"][1] for c, o, g in gs} == {1, 2, 3, 4}
    assert any(c.cuts[0].tracks[1].f16 and g["rows"][0]["energy"][1] > 1 for c, o, g in gs)  # a binary16 track across a block
    for c, o, g in gs:  # the scaled track covers the whole cut at -20 dB, and the reference is stored: both have items
        ref, t = c.cuts[0].tracks
        assert t.snr == -20.0 and t.first == 0 and t.frames == c.cuts[0].num_frames == c.row_frames and c.cuts[0].ref_track == 0 and ref.offset >= 0
        assert g["rows"][0]["energy"] == [-(-t.frames * c.F // C.ENERGY_BLOCK)] * 2
    # one stored row too few, and the repeated element is the ONLY element of the second item
    assert {bool(c.cuts[0].tracks[1].f16) for c, o, g in gs if c.cuts[0].tracks[1].rows == 16384 and c.cuts[0].tracks[1].frames == 16385 and c.F == 1} == {False, True}


def test_the_trip_case_gives_every_workgroup_a_second_energy_item_and_its_cuts_alone_do_not():
    (case,) = BY_GROUP["trip"]
    g = C.geometry(case.cuts, case.F, case.row_frames, 0)
    assert g["energy_items"] == 2048 > MAX_WORKGROUPS == 1792 and len(case.cuts) == 8 and case.F == 8
    assert -(-g["energy_items"] // -(-g["energy_items"] // MAX_WORKGROUPS)) == 1024  # the grid: two items per workgroup
    for c in case.cuts:
        alone = C.geometry([c], case.F, case.row_frames, 0)
        assert alone["energy_items"] == 256 <= MAX_WORKGROUPS and len(c.tracks) == 256 and c.ref_track == 0
        assert c.tracks[0].frames == 20 and all(t.frames == 3 and t.first == i % 18 and t.snr == 10.0 + i % 7 for i, t in enumerate(c.tracks) if i)
    assert all(max(g["energy_items"] for c, o, g in geometries(BY_GROUP[k])) <= MAX_WORKGROUPS for k in ("rep", "rowlen", "sweep", "energy", "tables"))


def test_the_table_cases_hold_what_they_were_built_for():
    gs = {c.name: (c, C.geometry(c.cuts, c.F, c.row_frames, 0)) for c in BY_GROUP["tables"]}
    c, g = gs["tables_constant_reference"]
    assert c.cuts[0].tracks[c.cuts[0].ref_track].offset == -1 and g["rows"][0]["energy"] == [0, 1, 1]
    c, g = gs["tables_reference_of_3_partials_in_256_tracks"]
    assert len(c.cuts[0].tracks) == 256 and g["rows"][0]["energy"] == [3] + [1] * 255 and all(t.offset >= 0 for t in c.cuts[0].tracks)
    c, g = gs["tables_tracks_without_partials_around_tracks_with"]
    assert [e for r in g["rows"] for e in r["energy"]] == [0, 1, 0, 0, 1, 0]
    c, g = gs["tables_fold_of_no_frames_between_folds"]
    assert [cut.form for cut in c.cuts] == [FOLD] * 4 and [cut.num_frames for cut in c.cuts] == [25, 0, 0, 25]


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_the_float32_model_stays_within_the_bar_of_the_truth(case):
    truth = R.batch(case.host, case.cuts, case.F, case.row_frames)
    model = R.batch(case.host, case.cuts, case.F, case.row_frames, model=True)
    for b, c in enumerate(case.cuts):
        rows = slice(c.dst_first, c.dst_first + c.num_frames)
        outside = np.ones(case.row_frames, dtype=bool)
        outside[rows] = False
        assert (model[b][outside] == np.float32(R.LOG_EPSILON)).all()
        if c.form == COPY:
            assert np.array_equal(model[b].view(np.uint32), truth[b].astype(np.float32).view(np.uint32))
        elif c.num_frames:
            err = np.abs(model[b][rows].astype(np.float64) - truth[b][rows])
            bound = R.bar(truth[b][rows]) + R.carried(c)[:, None]
            assert (err <= bound).all(), (case.name, b, float((err - bound).max()))
