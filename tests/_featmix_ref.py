"""The numpy statement of the feature-mix launches (include/hipfeat.h, "stored features mixed and collated on the device"): what
``collate_features`` (lhotse/dataset/collation.py:115-145) over ``MixedCut.load_features`` (lhotse/cut/mixed.py:1199-1309) computes for
a table of ``FeatCut``s over a host copy of the arena -- as a float64 TRUTH and as a float32 MODEL of the launch (float32 ``e``, gains
rounded to float32, one ``log``).  Shared by the CPU and the GPU tests; nothing here touches a device."""
import numpy as np

from lhotse_amd.augmentation import FEATMIX_COPY, FeatCut, FeatTrack

EPSILON = 1e-10
LOG_EPSILON = float(np.log(EPSILON))


def track_matrix(arena: np.ndarray, t: FeatTrack, F: int) -> np.ndarray:
    """The (frames, F) float32 matrix a track stands for: its stored rows (binary16 widened exactly), one row too many dropped, one too
    few repeated (lhotse/cut/mono.py:61-64); a constant track: float32(value) everywhere."""
    n = int(t.frames)
    if t.offset == -1:
        return np.full((n, F), np.float32(t.value), dtype=np.float32)
    rows = n if t.rows is None else int(t.rows)
    dt = np.float16 if t.f16 else np.float32
    take = min(rows, n)
    m = np.frombuffer(arena.tobytes()[int(t.offset): int(t.offset) + take * F * dt().itemsize], dtype=dt).reshape(take, F).astype(np.float32)
    if take < n:
        m = np.concatenate([m, m[-1:]], axis=0)
    return m


def _energy(m: np.ndarray) -> float:
    return float(np.sum(np.exp(m.astype(np.float64))))


def _gains(mats, c: FeatCut):
    g = [1.0] * len(mats)
    if c.ref_track < 0:
        return g
    e_ref = _energy(mats[c.ref_track])
    for i, (t, m) in enumerate(zip(c.tracks, mats)):
        if t.snr is None or np.isnan(t.snr) or (i == 0 and c.ref_track == 0):
            continue
        e_t = _energy(m)
        if e_ref > 0.0 and e_t > 0.0:
            g[i] = e_ref * 10.0 ** (-float(t.snr) / 10.0) / e_t
    return g


def cut_rows(arena: np.ndarray, c: FeatCut, F: int, model: bool = False) -> np.ndarray:
    """The (num_frames, F) matrix of one cut: float64 truth, or (``model``) the float32 arithmetic of the launch.  Copy form: float32 bits."""
    c = c if isinstance(c, FeatCut) else FeatCut(*c)
    tracks = [t if isinstance(t, FeatTrack) else FeatTrack(*t) for t in c.tracks]
    c = c._replace(tracks=tracks)
    mats = [track_matrix(arena, t, F) for t in tracks]
    T = int(c.num_frames)
    if c.form == FEATMIX_COPY:
        out = np.full((T, F), np.float32(c.pad_value), dtype=np.float32)
        out[: len(mats[0])] = mats[0]
        return out
    kept = [i for i, t in enumerate(tracks) if i == 0 or t.frames > 0]
    N = max(int(tracks[i].first) + int(tracks[i].frames) for i in kept)
    gains = _gains(mats, c)
    ft = np.float32 if model else np.float64
    e = np.zeros((N, F), dtype=ft)
    for i in kept:
        o, m = int(tracks[i].first), mats[i]
        add = np.zeros((N, F), dtype=ft)
        with np.errstate(over="ignore"):
            add[o: o + len(m)] = ft(np.float32(gains[i]) if model else gains[i]) * np.exp(m.astype(ft))
        e = e + add
        if i > 0:
            e = np.maximum(ft(EPSILON), e)
    with np.errstate(divide="ignore"):
        out = np.log(e)
    if N == T + 1:
        out = out[:T]
    elif N == T - 1:
        out = np.concatenate([out, out[-1:]], axis=0)
    assert len(out) == T, (N, T)
    return out


def batch(arena: np.ndarray, cuts_table, F: int, row_frames=None, model: bool = False) -> np.ndarray:
    """The (B, row_frames, F) batch: float64 truth (copy-form rows hold float32 values), or the float32 model."""
    cuts = [c if isinstance(c, FeatCut) else FeatCut(*c) for c in cuts_table]
    if row_frames is None:
        row_frames = max(int(c.dst_first) + int(c.num_frames) for c in cuts)
    out = np.full((len(cuts), row_frames, F), np.float32(LOG_EPSILON), dtype=np.float32 if model else np.float64)
    for b, c in enumerate(cuts):
        out[b, c.dst_first: c.dst_first + c.num_frames] = cut_rows(arena, c, F, model)
    return out


def bar(truth: np.ndarray, reference_max_abs: float = 0.0) -> np.ndarray:
    """The per-element accuracy bar of fold-form output: max(2 x the reference's own max-abs distance from truth on that cut,
    2 x spacing(float32(|truth|))) -- a 1-ulp logf plus one rounding of the result."""
    return np.maximum(2.0 * float(reference_max_abs), 2.0 * np.spacing(np.abs(truth).astype(np.float32)).astype(np.float64))


def carried(c: FeatCut) -> np.ndarray:
    """Per frame of a fold-form cut, (num_frames,): the bound on ``|log(e) - log(e_truth)|`` that the float32 arithmetic in front of the
    launch's log leaves, for the tests that have no recorded reference error to take their bar from.  With k = the tracks that cover
    the frame: every term ``g_t * exp(x_t)`` carries one ``expf`` (<= 1 ulp: 2^-23 relative), the gain's rounding to float32 (2^-24) and
    the product's (2^-24); all terms are positive, so their sum carries no more than the worst of them, and each add that is not an add
    of 0 rounds once more (2^-24): at most k of them, the first one too when the float32 floor (1e-10f, itself within 2^-24 of 1e-10)
    came before it.  The floor is 1-Lipschitz, so it adds nothing: r = (1 + 2^-23) (1 + 2^-24)^(k + 2) - 1 relative on ``e``, and
    ``|d log e| <= -log(1 - r)``.  The float64 energies contribute nothing that a float32 gain sees."""
    tracks = [t if isinstance(t, FeatTrack) else FeatTrack(*t) for t in c.tracks]
    kept = [t for i, t in enumerate(tracks) if i == 0 or t.frames > 0]
    N, T = max(int(t.first) + int(t.frames) for t in kept), int(c.num_frames)
    k = np.zeros(max(N, T), dtype=np.float64)
    for t in kept:
        k[int(t.first): int(t.first) + int(t.frames)] += 1.0
    if N == T - 1:
        k[T - 1] = k[T - 2]
    r = (1.0 + 2.0 ** -23) * (1.0 + 2.0 ** -24) ** (k[:T] + 2.0) - 1.0
    return -np.log1p(-r)


def load_golden():
    """tests/golden/featmix.json + .npz (tools/make_golden_featmix.py) -> {group: dict(arena, table, F, row_frames, ref, lens,
    reference_max_abs per cut -- None for a copy-form cut)}: the byte arena as ``HipPrecomputedFeatures`` packed it (binary16 rows),
    the ``FeatCut`` table of its classifier and the REFERENCE's batch."""
    import json
    import os

    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "featmix.json")) as f:
        meta = json.load(f)
    data = np.load(os.path.join(here, "featmix.npz"))
    out = {}
    for name, g in meta["groups"].items():
        table = [FeatCut([FeatTrack(o, n, r, h, first, snr, v) for o, n, r, h, first, snr, v in c["tracks"]], c["num_frames"], c["form"], c["pad_value"],
                         c["dst_first"], c["ref_track"]) for c in g["cuts"]]
        out[name] = dict(arena=data[f"{name}_arena"], table=table, F=meta["num_features"], row_frames=g["row_frames"], ref=data[f"{name}_ref"],
                         lens=data[f"{name}_lens"], reference_max_abs=[c.get("reference_max_abs") for c in g["cuts"]])
    return out


def widened(arena: np.ndarray, table, F: int):
    """The same batch with every binary16 track stored as float32 (the widened values) -> (arena, table): a track at byte ``o`` moves to
    byte ``2 * o``."""
    wide = np.zeros(2 * len(arena) + 16, dtype=np.uint8)
    new = []
    for c in table:
        tracks = []
        for t in c.tracks:
            if t.offset >= 0 and t.f16:
                rows = t.frames if t.rows is None else t.rows
                n = min(rows, t.frames) * F
                vals = np.frombuffer(arena.tobytes()[t.offset: t.offset + 2 * n], dtype=np.float16).astype(np.float32)
                wide[2 * t.offset: 2 * t.offset + 4 * n] = vals.view(np.uint8)
                t = t._replace(offset=2 * t.offset, f16=False)
            tracks.append(t)
        new.append(c._replace(tracks=tracks))
    return wide, new


def check_against_golden(g: dict, got: np.ndarray, label: str = "") -> None:
    """``got`` against one golden group: copy-form rows bit-equal to the reference, fold-form rows within the bar of the float64 truth
    (``reference_max_abs`` from the fixture); the measured distance is printed next to the reference's."""
    truth = batch(g["arena"], g["table"], g["F"], g["row_frames"])
    assert got.shape == g["ref"].shape, (label, got.shape)
    for b, (c, ref_err) in enumerate(zip(g["table"], g["reference_max_abs"])):
        if ref_err is None:
            assert np.array_equal(got[b].view(np.uint32), g["ref"][b].view(np.uint32)), (label, b)
            continue
        err = np.abs(got[b].astype(np.float64) - truth[b])
        print(f"{label} cut {b} ({len(c.tracks)} tracks): reference_max_abs = {ref_err:.3e}, measured max abs = {err.max():.3e}")
        assert (err <= bar(truth[b], ref_err)).all(), (label, b, float(err.max()), ref_err)
