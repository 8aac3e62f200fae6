"""Feature-mix cases at the tile, group and block edges of csrc/kernel_featmix.hpp, each with its geometry STATED: the launch arithmetic
restated in Python (``geometry``), never read back from the library.  Test infrastructure, no device: tests/test_featmix_edges_reference.py
holds every claim to ``build_featmix_plan`` / ``fm_tiles`` and asserts that the set as a whole enters every path it was built for;
tests/test_gpu_featmix_edges.py runs the same cases on the device.

A case is a host arena, a table of ``FeatCut``s, F, ``row_frames`` and the ``out_offset``s (0 ... 3 elements behind a 16-byte boundary) at
which ``out`` is handed over: row c of ``out`` then starts ``head = (out_offset + c * row_len) % 4`` elements behind a 16-byte boundary,
and the fold launch counts its tiles of 4096 elements from that boundary.  ``expect`` holds, per ``out_offset``, the figures the case was
built for as literals.

The restated arithmetic:
    row_len = row_frames * F;  tiles per row = (row_len + 2) // 4096 + 1;  element e of a row lies in tile (head + e) // 4096
    lo = dst_first * F;  hi = lo + num_frames * F;  rep = lo + mix_frames * F of a fold one frame longer than its mix, lo + rows * F
    of a copy whose track has one stored row too few
    energy items of a track = ceil(frames * F / 16384) if it is stored and either scaled (fold, an SNR, a reference, not the first track
    being the reference itself) or the reference of a cut with a scaled track
``rep_behind``: the elements of the repeated frame that lie in a tile whose first element is at or behind ``rep`` -- the elements a
tile can only form by reading "up to F elements in front of itself"."""
from typing import Dict, List, NamedTuple, Sequence, Tuple

import numpy as np

from lhotse_amd.augmentation import FEATMIX_COPY as COPY, FEATMIX_FOLD as FOLD, FeatCut, FeatTrack

TILE = 4096           # kFmTile (held to ft_tile() by the CPU test)
ENERGY_BLOCK = 16384  # kFmEnergyBlock (ft_energy_block())
LOG_EPS = float(np.log(1e-10))


class Arena:
    """Tracks packed by hand into a byte buffer: float32 at 4-byte boundaries that are no 16-byte boundaries, binary16 at odd 2-byte ones."""

    def __init__(self, seed=0):
        self.rs = np.random.RandomState(seed)
        self.buf = bytearray(self.rs.bytes(6))
        self.k = 0

    def add(self, m: np.ndarray, f16=False) -> int:
        self.k += 1
        if f16:
            while len(self.buf) % 4 != 2:  # an odd multiple of 2
                self.buf += b"\x7b"
        else:
            while len(self.buf) % 16 != 4 * (1 + self.k % 3):
                self.buf += b"\x7b"
        off = len(self.buf)
        self.buf += np.ascontiguousarray(m, dtype=np.float16 if f16 else np.float32).tobytes()
        return off

    def feats(self, n, F, f16=False, lo=-15.0, hi=5.0):
        m = self.rs.uniform(lo, hi, (n, F)).astype(np.float32)
        return m.astype(np.float16).astype(np.float32) if f16 else m

    def track(self, n, F, f16=False, rows=None, **kw) -> FeatTrack:
        m = self.feats(n if rows is None else rows, F, f16)
        return FeatTrack(self.add(m, f16), n, rows, f16, **kw)

    def host(self) -> np.ndarray:
        return np.frombuffer(bytes(self.buf) + b"\x00" * (-len(self.buf) % 16), dtype=np.uint8).copy()


class Case(NamedTuple):
    name: str
    group: str  # rep | rowlen | sweep | energy | trip | tables
    host: np.ndarray
    cuts: List[FeatCut]
    F: int
    row_frames: int
    offsets: Tuple[int, ...]       # the out_offsets the case is run at
    expect: Dict[int, dict] = {}   # out_offset -> literal claims: keys of ``geometry`` (per-row lists) or of one of its rows as "key@row"


def _mix_frames(c: FeatCut) -> int:
    kept = [t for i, t in enumerate(c.tracks) if i == 0 or t.frames > 0]
    return max(int(t.first) + int(t.frames) for t in kept)


def energy_items(c: FeatCut, F: int) -> List[int]:
    """Energy work items of every track of one cut."""
    ref = int(c.ref_track)
    scaled = [c.form == FOLD and t.snr is not None and not np.isnan(t.snr) and ref >= 0 and not (i == 0 and ref == 0) for i, t in enumerate(c.tracks)]
    out = []
    for i, t in enumerate(c.tracks):
        needs = t.offset >= 0 and (scaled[i] or (i == ref and any(scaled)))
        out.append(-(-int(t.frames) * F // ENERGY_BLOCK) if needs else 0)
    return out


def geometry(cuts: Sequence[FeatCut], F: int, row_frames: int, out_offset: int) -> dict:
    """The claims of a case at one ``out_offset``: per row ``head``, ``lo``, ``hi``, ``rep`` (None: no repeated frame), the tiles that
    hold ``lo``, ``hi - 1`` and ``rep`` (None where there is no such element), ``rep_behind``, ``last_tile`` (the elements of the row in
    its last planned tile: <= 0 = planned but empty, 1 ... 3 = nothing but a scalar tail) and ``energy`` (items per track); for the
    batch ``tiles``, ``fold_items`` and ``energy_items``."""
    row_len = row_frames * F
    tiles = 0 if row_len == 0 else (row_len + 2) // TILE + 1
    rows = []
    for ci, c in enumerate(cuts):
        head = (out_offset + ci * row_len) % 4
        lo = int(c.dst_first) * F
        hi = lo + int(c.num_frames) * F
        rep = None
        if c.form == FOLD:
            if c.num_frames == _mix_frames(c) + 1:
                rep = lo + _mix_frames(c) * F
        else:
            t = c.tracks[0]
            if t.offset >= 0 and t.rows is not None and t.frames > 0 and t.rows == t.frames - 1:
                rep = lo + int(t.rows) * F

        def tile(e, head=head):
            return (head + e) // TILE

        behind = 0 if rep is None else sum(1 for e in range(rep, rep + F) if tile(e) * TILE - head >= rep)
        rows.append(dict(head=head, lo=lo, hi=hi, rep=rep, tile_lo=tile(lo) if hi > lo else None, tile_hi=tile(hi - 1) if hi > lo else None,
                         tile_rep=None if rep is None else tile(rep), rep_behind=behind, last_tile=head + row_len - (tiles - 1) * TILE,
                         energy=energy_items(c, F)))
    return dict(row_len=row_len, tiles=tiles, rows=rows, fold_items=len(cuts) * tiles, energy_items=sum(sum(r["energy"]) for r in rows))


def claim(g: dict, key: str):
    """``key`` of the batch, ``key@row`` of one row, or ``key@*``: the list over the rows."""
    if "@" not in key:
        return g[key]
    k, r = key.split("@")
    return [row[k] for row in g["rows"]] if r == "*" else g["rows"][int(r)][k]


def _tail(a: Arena, F: int) -> None:
    a.add(np.zeros((2, F), dtype=np.float32))  # nothing reads it: room behind the last track


ALL = (0, 1, 2, 3)


# ---- the repeated last frame (and the dropped one) at a tile boundary ---------------------------------------------------------------------
def _rep_cases() -> List[Case]:
    out = []

    def pair(F, total, expect, seed, short=None):
        """A fold of two tracks and a copy whose LAST frame repeats the one in front of it, frames [1, 1 + total) of a row of 1 + total:
        ``rep`` = total * F.  The long track ends at ``rep``; the short one (an SNR, binary16) ends more than F elements in front of the
        tile boundary, so the tile behind the boundary must leave it out and take the long one in."""
        n = total - 1  # frames of the mix / stored rows of the copy
        short = short or (min(10, n - 1), max(1, n // 2))
        a = Arena(seed)
        fold = FeatCut([a.track(n, F), a.track(short[1], F, f16=True, first=short[0], snr=5.0)], n + 1, FOLD, dst_first=1, ref_track=0)
        _tail(a, F)
        out.append(Case(f"rep_fold_F{F}_{total}", "rep", a.host(), [fold], F, total + 1, ALL, expect))
        a = Arena(seed + 1)
        copy = FeatCut([a.track(n + 1, F, rows=n)], n + 1, COPY, dst_first=1)
        _tail(a, F)
        out.append(Case(f"rep_copy_F{F}_{total}", "rep", a.host(), [copy], F, total + 1, ALL, expect))

    # F = 23, rep = 178 * 23 = 4094: the second tile starts 2, 1, 0 elements behind rep and 1 in front of it
    pair(23, 178, {0: {"rep@0": 4094, "tiles": 2, "rep_behind@0": 21, "tile_rep@0": 0}, 1: {"rep_behind@0": 22, "tile_rep@0": 0},
                       2: {"rep_behind@0": 23, "tile_rep@0": 1}, 3: {"rep_behind@0": 0, "tile_rep@0": 1}}, 100)
    # rep = 177 * 23 = 4071, a row of 4094: at head 3 the second tile holds ONE element, the last bin of the repeated frame; at the other
    # heads the second tile is planned but empty
    pair(23, 177, {0: {"rep@0": 4071, "tiles": 2, "last_tile@0": -2, "rep_behind@0": 0}, 1: {"last_tile@0": -1}, 2: {"last_tile@0": 0},
                       3: {"last_tile@0": 1, "rep_behind@0": 1}}, 102)
    # F = 1: the frame is one element; at head 2 it is the first element of the second tile
    pair(1, 4094, {0: {"rep@0": 4094, "rep_behind@0": 0}, 2: {"rep_behind@0": 1, "tile_rep@0": 1}, 3: {"rep_behind@0": 0, "tile_rep@0": 1}}, 104, short=(100, 3000))
    # F = 257: 15 * 257 = 3855, the repeated frame [3855, 4112) lies across the boundary at every head
    pair(257, 15, {0: {"rep@0": 3855, "rep_behind@0": 16}, 3: {"rep_behind@0": 19}}, 106, short=(1, 5))
    # F = 257, a row of 255 frames: the repeated frame [65278, 65535) starts one frame in front of the 16th boundary and ends on it at head 1
    # (16 * 4096 = 255 * 257 + 1): tile 16 is planned but empty at heads 0 and 1 and holds 1 and 2 elements of the repeated frame at heads 2, 3
    pair(257, 254, {0: {"rep@0": 65278, "tiles": 17, "last_tile@0": -1, "rep_behind@0": 0}, 1: {"last_tile@0": 0, "rep_behind@0": 0},
                        2: {"last_tile@0": 1, "rep_behind@0": 1}, 3: {"last_tile@0": 2, "rep_behind@0": 2}}, 108, short=(3, 100))
    # one frame DROPPED (num_frames == mix_frames - 1): hi = 178 * 23 = 4094 lies in front of the boundary at heads 0 and 1, on it at head 2
    # and behind it at head 3; the 23 elements behind hi are log(1e-10), not the dropped frame
    a = Arena(110)
    fold = FeatCut([a.track(178, 23), a.track(60, 23, f16=True, first=118, snr=5.0)], 177, FOLD, dst_first=1, ref_track=0)
    _tail(a, 23)
    out.append(Case("drop_fold_F23_178", "rep", a.host(), [fold], 23, 179, ALL,
                    {0: {"hi@0": 4094, "tile_hi@0": 0, "rep@0": None}, 1: {"tile_hi@0": 0}, 2: {"tile_hi@0": 0}, 3: {"tile_hi@0": 1}}))
    a = Arena(111)
    fold = FeatCut([a.track(4098, 1), a.track(60, 1, first=4038, snr=5.0)], 4097, FOLD, ref_track=0)  # hi = 4097: tile 1 at every head
    _tail(a, 1)
    out.append(Case("drop_fold_F1_4098", "rep", a.host(), [fold], 1, 4099, ALL, {0: {"hi@0": 4097, "tile_hi@0": 1}, 3: {"tile_hi@0": 1}}))
    return out


# ---- the row's length and alignment at the tile edge -----------------------------------------------------------------------------------
ROW_FRAMES = (4093, 4094, 4095, 4096, 4097, 8191, 8192, 8193)


def _rowlen_cases() -> List[Case]:
    out = []
    for n in ROW_FRAMES:  # F = 1, B = 3: a fold over the whole row, a copy with padding behind it, a cut of no frames
        a = Arena(200 + n)
        cuts = [FeatCut([a.track(n, 1), a.track(n // 2, 1, f16=True, first=n - n // 2, snr=3.0)], n, FOLD, ref_track=0),
                FeatCut([a.track(n - 5, 1, f16=bool(n % 2))], n - 2, COPY, pad_value=-7.5),
                FeatCut([FeatTrack(-1, 0)], 0, COPY)]
        _tail(a, 1)
        tiles = {4093: 1, 4094: 2, 4095: 2, 4096: 2, 4097: 2, 8191: 3, 8192: 3, 8193: 3}[n]
        out.append(Case(f"rowlen_{n}", "rowlen", a.host(), cuts, 1, n, ALL,
                        {0: {"tiles": tiles, "head@*": [0, n % 4, 2 * n % 4]}, 1: {"head@*": [1, (1 + n) % 4, (1 + 2 * n) % 4]}}))
    return out


# ---- lo and hi of a fold against a 16-byte group and a tile ----------------------------------------------------------------------------
SWEEP_LENGTHS = (1, 2, 3, 4, 5, 8)  # frames


def _sweep_cases() -> List[Case]:
    """One batch per F and head; row_len is a multiple of 4, so every row of a batch has the batch's head, and the boundary between tile
    0 and tile 1 is element 4096 - head of every row.  F = 1: lo in {0 ... 5, 4094 - head ... 4098 - head} (every residue of a 16-byte group on either side) x hi - lo in
    {1, 2, 3, 4, 5, 8}, and hi at the same three positions with lo = 0 and lo = hi - 8, and 8 frames across each of them.  F = 3: lo and hi are multiples of 3, so the frames
    at the boundary are those with 3 * dst_first in [4094 - head, 4098 - head] (the nearest ones on either side)."""
    out = []
    for F, row_frames in ((1, 4112), (3, 1376)):
        assert row_frames * F % 4 == 0
        for head in ALL:
            edge = TILE - head
            if F == 1:
                firsts = [0, 1, 2, 3, 4, 5, edge - 2, edge - 1, edge, edge + 1, edge + 2]
                ends = [edge - 1, edge, edge + 1]
            else:
                firsts = [0, 1, 2] + [d for d in range(edge // 3 - 2, edge // 3 + 3) if edge - 2 <= 3 * d <= edge + 2]
                ends = [d for d in range(edge // 3 - 2, edge // 3 + 3) if edge - 2 <= 3 * d <= edge + 2]
            spans = [(d, n) for d in firsts for n in SWEEP_LENGTHS] + [(0, e) for e in ends] + [(e - 8, 8) for e in ends] + [(e - 4, 8) for e in ends]
            a = Arena(300 + 10 * F + head)
            cuts = []
            for k, (d, n) in enumerate(spans):
                m = max(1, n // 2)
                cuts.append(FeatCut([a.track(n, F, f16=bool(k % 3 == 1)), a.track(m, F, f16=bool(k % 2), first=n - m, snr=3.0)], n, FOLD, dst_first=d, ref_track=0))
            _tail(a, F)
            out.append(Case(f"sweep_F{F}_head{head}", "sweep", a.host(), cuts, F, row_frames, (head,), {head: {"head@*": [head] * len(cuts), "tiles": 2}}))
    return out


# ---- energy blocks ------------------------------------------------------------------------------------------------------------------
ENERGY_SIZES = {1: (16383, 16384, 16385, 32768, 32769, 49153), 64: (256, 257, 512)}  # F -> frames


def _energy_cases() -> List[Case]:
    """A reference and a track scaled to -20 dB SNR (100 x the reference's energy) that covers the whole cut: log(gain) reaches every
    output value at full weight.  Both tracks are stored, so both have energy items."""
    out = []
    for F, sizes in ENERGY_SIZES.items():
        for n in sizes:
            for f16 in (False, True):
                a = Arena(400 + n % 1000 + F + int(f16))
                cuts = [FeatCut([a.track(n, F, f16=f16), a.track(n, F, f16=f16, snr=-20.0)], n, FOLD, ref_track=0)]
                _tail(a, F)
                items = -(-n * F // ENERGY_BLOCK)
                out.append(Case(f"energy_F{F}_{n}_{'f16' if f16 else 'f32'}", "energy", a.host(), cuts, F, n, (0, 3),
                                {0: {"energy@0": [items, items], "energy_items": 2 * items}}))
    # 16385 frames of one bin standing on 16384 stored rows: the repeated element is the only element of the track's second item; it is the
    # largest value of the track, so an energy without it moves the gain by more than any bound here
    for f16 in (False, True):
        a = Arena(450 + int(f16))
        m = a.feats(16384, 1, f16)
        m[-1] = 5.0
        cuts = [FeatCut([a.track(16385, 1), FeatTrack(a.add(m, f16), 16385, 16384, f16, 0, -20.0)], 16385, FOLD, ref_track=0)]
        _tail(a, 1)
        out.append(Case(f"energy_repeated_row_{'f16' if f16 else 'f32'}", "energy", a.host(), cuts, 1, 16385, (0, 3), {0: {"energy@0": [2, 2], "energy_items": 4}}))
    return out


# ---- more energy items than workgroups ------------------------------------------------------------------------------------------------
def _trip_case() -> Case:
    """8 folds of 256 tracks, F = 8: track 0 (the reference) has 20 stored frames, track t 3 stored frames from frame t % 18 with an SNR
    of 10 + t % 7 dB.  Every track is stored and needs an energy: 8 x 256 = 2048 energy items, of one block each."""
    a, F = Arena(500), 8
    cuts = [FeatCut([a.track(20, F)] + [a.track(3, F, f16=bool(t % 2), first=t % 18, snr=10.0 + t % 7) for t in range(1, 256)], 20, FOLD, ref_track=0)
            for _ in range(8)]
    _tail(a, F)
    return Case("trip_2048", "trip", a.host(), cuts, F, 20, ALL, {0: {"energy_items": 2048, "fold_items": 8, "energy@0": [1] * 256}})


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def _table_cases() -> List[Case]:
    out = []
    F = 23
    a = Arena(600)  # the reference is a constant track: its energy is frames * F * exp(value), no partial
    cuts = [FeatCut([FeatTrack(-1, 30, value=-2.0), a.track(30, F, snr=5.0), a.track(12, F, f16=True, first=9, snr=-3.0)], 30, FOLD, ref_track=0)]
    _tail(a, F)
    out.append(Case("tables_constant_reference", "tables", a.host(), cuts, F, 30, ALL, {0: {"energy@0": [0, 1, 1], "energy_items": 2}}))
    F = 64
    a = Arena(601)  # a reference of 600 x 64 = 38400 elements (3 partials) in front of 255 stored tracks of one partial each
    cuts = [FeatCut([a.track(600, F)] + [a.track(2, F, f16=bool(t % 2), first=(7 * t) % 598, snr=5.0 + t % 11) for t in range(1, 256)], 600, FOLD, ref_track=0)]
    _tail(a, F)
    out.append(Case("tables_reference_of_3_partials_in_256_tracks", "tables", a.host(), cuts, F, 600, (0, 3),
                    {0: {"energy@0": [3] + [1] * 255, "energy_items": 258, "tiles": 10}}))
    F = 23
    a = Arena(602)  # track order: no partial, partial, no partial | no partial, partial, no partial
    cuts = [FeatCut([FeatTrack(-1, 20, value=-4.0), a.track(20, F, snr=6.0), a.track(8, F, first=5)], 20, FOLD, ref_track=0),
            FeatCut([a.track(20, F), a.track(14, F, f16=True, first=6, snr=2.0), FeatTrack(-1, 20, value=-6.0)], 20, FOLD, ref_track=2)]
    _tail(a, F)
    out.append(Case("tables_tracks_without_partials_around_tracks_with", "tables", a.host(), cuts, F, 20, ALL,
                    {0: {"energy@0": [0, 1, 0], "energy@1": [0, 1, 0], "energy_items": 2}}))
    a = Arena(603)  # folds of 0 frames (no track with frames; one stored frame dropped) between folds with frames
    cuts = [FeatCut([a.track(25, F), a.track(10, F, first=15, snr=4.0)], 25, FOLD, ref_track=0),
            FeatCut([FeatTrack(-1, 0)], 0, FOLD),
            FeatCut([a.track(1, F)], 0, FOLD),
            FeatCut([a.track(25, F, f16=True), a.track(10, F, first=3, snr=8.0)], 25, FOLD, ref_track=0, dst_first=1)]
    _tail(a, F)
    out.append(Case("tables_fold_of_no_frames_between_folds", "tables", a.host(), cuts, F, 26, ALL,
                    {0: {"lo@1": 0, "hi@1": 0, "hi@2": 0, "energy_items": 4}}))
    return out


def all_cases() -> List[Case]:
    return _rep_cases() + _rowlen_cases() + _sweep_cases() + _energy_cases() + [_trip_case()] + _table_cases()


CASES = all_cases()
