"""GPU: cuts scaled and clipped on the device (hipfeat_level_*, lhotse_amd.augmentation.level_in_arena, HipVolume, HipClipping) against the
numpy statement of the rule (tests/_level_ref.py).

Bars.  SCALE and hard CLIP: ``array_equal`` to ``model32`` (which tests/test_level_reference.py shows to be ``array_equal`` to lhotse's
Volume / Clipping).  Soft CLIP, judged against the float64 truth of the same float32 input: max abs error <= 2 x the reference's own +
2^-24 x peak, rel-L2 <= 2 x the reference's own; the reference's figures are the recorded ones of tests/golden/level.json ("soft_cases",
written by tools/make_golden_level.py from lhotse's Clipping), never the device's."""
import json
import os

import numpy as np
import pytest
import torch

import _level_ref as L

from lhotse_amd import _lib
from lhotse_amd.augmentation import HipClipping, HipVolume, get_or_create_level, level_in_arena

pytestmark = pytest.mark.gpu
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4099, 70001)
GUARD = 5  # floats between neighbours in the arena: they must come back untouched
# (source offset mod 4, destination: None = in place, else its offset mod 4)
PLACEMENTS = ((0, None), (1, None), (3, None), (0, 0), (2, 2), (0, 1), (3, 2))
EXACT_PROGRAMS = [
    [("volume", 0.37)],
    [("clip", True, 0.0, True)],
    [("clip", True, 0.05, False)],
    [("clip", True, -6.0, True)],
    [("clip", True, 20.0, False)],
    [("volume", 1.9), ("clip", True, 20.0, True)],  # SCALE -> CLIP
    [("clip", True, -6.0, True), ("volume", 0.6)],  # CLIP -> SCALE
    [("volume", -1.3), ("volume", 0.9), ("clip", True, 20.0, True), ("volume", 1.1)],  # 4 ops, a negative factor
]


def _place(pos, mod):
    """the first offset >= pos + GUARD with offset % 4 == mod"""
    pos += GUARD
    return pos + ((mod - pos) % 4)


def _run(items, fill=float("nan"), level=None):
    """items: [(x, program, source offset mod 4, None | destination offset mod 4)] -> the outputs (numpy), through ONE level_in_arena call.
    Everything the items do not own -- the guards, and the sources of out-of-place items -- must come back unchanged."""
    so, do, pos = [], [], 0
    for x, _, smod, dmod in items:
        s = _place(pos, smod)
        pos = s + len(x)
        so.append(s)
        if dmod is None:
            do.append(s)
        else:
            d = _place(pos, dmod)
            pos = d + len(x)
            do.append(d)
    host = np.full(pos + GUARD, fill, dtype=np.float32)
    for (x, _, _, _), s in zip(items, so):
        host[s : s + len(x)] = x
    arena = torch.from_numpy(host).to("cuda:0")
    lens = [len(x) for x, _, _, _ in items]
    inplace = all(d is None for _, _, _, d in items)
    got = level_in_arena(arena, so, lens, [p for _, p, _, _ in items], None if inplace else do, level=level)
    assert got.tolist() == do
    out = arena.cpu().numpy()
    written = np.zeros(len(out), dtype=bool)
    for d, n in zip(do, lens):
        assert not written[d : d + n].any()
        written[d : d + n] = True
    assert np.array_equal(out[~written], host[~written], equal_nan=True)
    return [out[d : d + n].copy() for d, n in zip(do, lens)]


def _exact_grid():
    items, k = [], 0
    for n in LENGTHS:
        for pi, prog in enumerate(EXACT_PROGRAMS):
            for smod, dmod in (PLACEMENTS if n != 70001 else ((1, None), (0, 1), (3, 2))):
                amp = 1.5 if any(op[0] == "clip" and not op[3] for op in prog) else 0.5  # normalize=False: samples above 1 are what clips
                items.append((L.signal(100 + k, n, amp), prog, smod, dmod))
                k += 1
    return items


def test_scale_and_hard_clip_equal_the_model_bit_for_bit():
    items = _exact_grid()
    outs = _run(items)
    for (x, prog, smod, dmod), y in zip(items, outs):
        want = L.model32(x, prog)
        assert np.all(np.abs(want[want != 0]) >= np.finfo(np.float32).tiny)  # the inputs keep every result a normal number
        assert np.array_equal(y, want), (len(x), prog, smod, dmod, float(np.max(np.abs(y - want))))
    # ... and something was clipped: normalize=False on samples above 1 hits the rails
    clipped = [y for (x, prog, _, _), y in zip(items, outs) if prog == [("clip", True, 0.05, False)] and len(x) >= 63]
    assert clipped and all(np.max(y) == 1.0 and np.min(y) == -1.0 for y in clipped)


def _with_peak(n, at, value, seed):
    x = L.signal(seed, n, 0.25)
    x[at] = value
    return x


def test_peak_placement_and_special_items():
    n = 4099  # 4096 + 3: with source offset 1 the last group of the second tile is cut: the scalar tail; with offset 3 the first group is
    hard, soft_free = [("clip", True, 20.0, True)], [("volume", 2.0), ("clip", True, -6.0, True)]
    below, above = np.nextafter(L.SILENCE_PEAK, np.float32(0)), np.nextafter(L.SILENCE_PEAK, np.float32(1))
    items = []
    for smod in (0, 1, 3):
        items += [(_with_peak(n, 0, 0.9, 1), hard, smod, None),  # the peak at the first sample (the scalar head when smod != 0)
                  (_with_peak(n, n - 1, 0.9, 2), hard, smod, None),  # at the last sample
                  (_with_peak(n, n - 2, 0.9, 3), hard, smod, 2),  # in the scalar tail
                  (_with_peak(n, 4096 - smod, -0.9, 4), hard, smod, None),  # a negative peak, at the first sample of the second tile
                  (_with_peak(n, 777, -0.8, 5), soft_free, smod, 0),
                  (np.zeros(n, np.float32), hard, smod, None),  # all zero: passes through (p == 0)
                  (np.zeros(1, np.float32), soft_free, smod, None)]
        for p in (below, L.SILENCE_PEAK, above):  # around the silence threshold: passes through below it, is normalised from it on
            x = (L.signal(6, n, 1.0) * p).astype(np.float32)
            x[n // 2] = -p
            items.append((x, [("clip", True, 20.0, True)], smod, None))
            items.append((x / np.float32(4.0), [("volume", 4.0), ("clip", True, 20.0, True)], smod, 1))  # the threshold meets the PROPAGATED peak
        items.append((L.signal(7, n, 3.0), [("clip", True, 0.0, False)], smod, None))  # samples above 1, normalize=False
    outs = _run(items)
    for (x, prog, smod, dmod), y in zip(items, outs):
        assert np.array_equal(y, L.model32(x, prog)), (prog, smod, dmod, float(np.max(np.abs(x))))
    # the silence decision itself, not only agreement with the model: below the threshold the item is only scaled
    for (x, prog, _, _), y in zip(items, outs):
        peak = L.propagated_peak(x, [op[1] for op in prog if op[0] == "volume"])
        if 0 < peak < L.SILENCE_PEAK:
            assert np.array_equal(y, x * np.float32(4.0) if prog[0][0] == "volume" else x)
        if peak == above and prog[0][0] == "clip":
            assert not np.array_equal(y, x)  # 20 dB of gain on a normalised item clips its peak
    y = outs[[i for i, it in enumerate(items) if it[1] == [("clip", True, 0.0, False)]][0]]
    assert np.max(y) == 1.0 and np.min(y) == -1.0


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "level.json")) as _f:
    SOFT_FIGURES = json.load(_f)["soft_cases"]


def test_soft_clip_meets_the_reference_bar():
    assert [c[0] for c in L.SOFT_CASES] == [c["name"] for c in SOFT_FIGURES]  # the recorded figures belong to these cases
    items = [(L.signal(seed, n, amp), prog, (1, 0, 3)[k % 3], (None, 2)[k % 2]) for k, (_, seed, n, amp, prog) in enumerate(L.SOFT_CASES)]
    outs = _run(items)
    for (x, prog, _, _), y, fig in zip(items, outs, SOFT_FIGURES):
        truth = L.exact(x, prog)
        got_max, got_rel = L.distances(y, truth)
        bar_max, bar_rel = L.soft_bars(fig["ref_max_abs"], fig["ref_rel_l2"], truth)
        print(f"{fig['name']}: max abs {got_max:.3e} (bar {bar_max:.3e}), rel-L2 {got_rel:.3e} (bar {bar_rel:.3e})")
        assert got_max <= bar_max and got_rel <= bar_rel, (fig["name"], got_max, bar_max, got_rel, bar_rel)


def _mixed_batch(count):
    rng = np.random.RandomState(count)
    lengths = list(LENGTHS[:-1]) + [4096, 8191, 12289]
    progs = EXACT_PROGRAMS + [[("clip", False, 20.0, True)], [("volume", 0.5), ("clip", False, 0.0, True)]]
    return [(L.signal(5000 + i, lengths[rng.randint(len(lengths))], 0.7), progs[rng.randint(len(progs))], int(rng.randint(4)),
             (None, 0, 1, 2, 3)[rng.randint(5)]) for i in range(count)]


@pytest.mark.parametrize("count", [300, 390])  # 64-byte descriptors: 300 are searched in LDS, 390 (> 24576 / 64 = 384) where they are staged
def test_a_batch_equals_its_items_run_alone_and_repeats_bit_for_bit(count):
    items = _mixed_batch(count)
    level = get_or_create_level("cuda:0")
    first = _run(items, level=level)
    second = _run(items, fill=0.25, level=level)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    for it, a in list(zip(items, first))[:: (1 if count == 300 else 13)]:
        assert np.array_equal(_run([it], level=level)[0], a)  # 1 item: the table travels in the kernel arguments


def test_two_runs_of_a_long_soft_item_are_bit_identical():
    x = L.signal(9, 70001 * 3, 0.9)
    prog = [("volume", 1.2), ("clip", False, 20.0, True)]
    a, b = _run([(x, prog, 1, None)])[0], _run([(x, prog, 1, 3)], fill=-1.0)[0]
    assert np.array_equal(a, b)
    assert np.array_equal(a, _run([(x, prog, 1, None)])[0])


def test_zero_items_launch_nothing_and_bad_tables_raise():
    arena = torch.zeros(64, dtype=torch.float32, device="cuda:0")
    assert len(level_in_arena(arena, [], [], [])) == 0
    level = get_or_create_level("cuda:0")
    ticket, info = level.plan([], [], [])
    assert info[1:].tolist() == [0, 0, 0]
    level.run(ticket, arena)
    for args, status in ((([0], [0], [[("volume", 2.0)]]), _lib.ERR_INVALID), (([0], [8], [[]]), _lib.ERR_INVALID),
                         (([0], [8], [[("volume", 2.0)] * 5]), _lib.ERR_INVALID), (([0], [8], [[("volume", 2.0)]], [4]), _lib.ERR_INVALID),
                         (([0], [8], [[("clip", True, 0.0, True)] * 2]), _lib.ERR_UNSUPPORTED)):
        with pytest.raises(_lib.HipFeatError) as e:
            level.plan(*args)
        assert e.value.status == status
    with pytest.raises(ValueError, match="arena too small"):
        level_in_arena(arena, [60], [8], [[("volume", 2.0)]])
    assert torch.count_nonzero(arena).item() == 0


def test_transforms_numpy_and_tensor_and_the_peak_over_all_channels():
    x = np.stack([L.signal(11, 1001, 0.2), L.signal(12, 1001, 0.8)])  # the peak sits in channel 1: channel 0 is normalised by it too
    vol, clip = HipVolume(factor=0.75), HipClipping(hard=True, gain_db=12.0, normalize=True)
    y = vol(x, 16000)
    assert isinstance(y, np.ndarray) and y.shape == x.shape and np.array_equal(y, x * np.float32(0.75))
    y = clip(x, 16000)
    want = L.model32(x.reshape(-1), [("clip", True, 12.0, True)]).reshape(x.shape)
    assert isinstance(y, np.ndarray) and np.array_equal(y, want)
    assert not np.array_equal(y[0], L.model32(x[0], [("clip", True, 12.0, True)]))  # per-channel peaks would give this
    for dev in ("cpu", "cuda:0"):
        t = torch.from_numpy(x).to(dev)
        keep = t.clone()
        out = clip(t, 16000)
        assert isinstance(out, torch.Tensor) and out.device == t.device and out.shape == t.shape
        assert np.array_equal(out.cpu().numpy(), want) and torch.equal(t, keep)  # the input is not modified
    soft = HipClipping()(x, 16000)
    assert (soft.dtype, soft.shape) == (np.float32, x.shape) and L.distances(soft.reshape(-1), L.exact(x.reshape(-1), [("clip", False, 0.0, True)]))[0] < 1e-6
    assert HipClipping().to_dict() == {"name": "HipClipping", "kwargs": {"hard": False, "gain_db": 0.0, "normalize": True, "device": "cuda"}}
    assert (vol.reverse_timestamps(1.0, 2.0, 16000), clip.reverse_timestamps(1.0, None, 16000)) == ((1.0, 2.0), (1.0, None))
