"""GPU: cuts reverberated with a recorded impulse response on the device (hipfeat_reverb_*, lhotse_amd.augmentation.reverb_in_arena,
HipReverbWithImpulseResponse, FusedMiniBatch.features_of_tracks with 7-element tracks).

Bars (tests/_reverb_ref.py::bars).  Both the device (direct form, float32 partial sums of 256 taps) and the CPU path (float32 FFTs) are
judged against the exact float64 convolution of the same float32 inputs: the device's rel-L2 may be at most 2 x the FFT form's own + 2^-24,
its max abs error at most 2 x the FFT form's own + 2^-24 x peak.  One serial float32 chain over all taps is 3-16 x worse than the FFT form
and fails these.  Normalised audio: the same against the float64 result scaled by the float64 gain."""
import numpy as np
import pytest
import torch

import _reverb_ref as R

import lhotse_amd as LA
from lhotse_amd import _lib
from lhotse_amd.augmentation import HipReverb, HipReverbWithImpulseResponse, get_or_create_reverb, reverb_in_arena, reverb_tail_floats, scaled_rir
from lhotse_amd.input_strategies import FusedMiniBatch

pytestmark = pytest.mark.gpu
NS = (1, 255, 4097, 20000)
LS = (1, 255, 256, 257, 800, 3000)


def _signal(rng, n):
    """Gated noise: bursts of different levels with silence between them."""
    x = rng.standard_normal(n).astype(np.float32) * np.float32(0.1)
    gate = np.repeat(rng.choice([0.0, 0.3, 1.0], size=n // 500 + 1), 500)[:n].astype(np.float32)
    return x * gate if n > 1 else x


def _rir(rng, taps, peak_at):
    """Decaying noise with a dominant peak, as int16 samples in float32 (what load_audio returns for a 16-bit file)."""
    h = rng.standard_normal(taps) * np.exp(-6.0 * np.arange(taps) / max(taps, 2)) * 0.2
    h[peak_at] = 1.0
    return (np.round(h * 20000.0) / 32768.0).astype(np.float32)


def _shifts(taps):
    return sorted({0, taps // 2, taps - 1})


def _grid():
    rng = np.random.default_rng(20240607)
    items = []
    for n in NS:
        for taps in LS:
            x = _signal(rng, n)
            for peak in _shifts(taps):
                hs, shift = scaled_rir(_rir(rng, taps, peak))
                assert shift == peak
                items += [(x, hs, shift, False), (x, hs, shift, True)]
    return items


def _run(items, reverb=None, fill=float("nan"), info=None):
    """items: [(x, hs, shift, normalize)] -> the outputs (numpy) through reverb_in_arena alone; sources / RIRs must come back unchanged.
    ``info``: a list that receives the plan's info block (the two calls reverb_in_arena consists of are then made here)."""
    chunks, so, ro, pos = [], [], [], 0
    for x, hs, _, _ in items:
        so.append(pos), chunks.append(x)
        pos += len(x)
        ro.append(pos), chunks.append(hs)
        pos += len(hs)
    front = np.concatenate(chunks)
    lens = [len(x) for x, _, _, _ in items]
    arena = torch.full((((pos + 3) & ~3) + reverb_tail_floats(lens),), fill, dtype=torch.float32, device="cuda:0")
    arena[:pos] = torch.from_numpy(front)
    tables = (so, lens, ro, [len(h) for _, h, _, _ in items], [s for _, _, s, _ in items], [int(f) for _, _, _, f in items], pos)
    if info is None:
        offs = reverb_in_arena(arena, *tables, reverb=reverb)
    else:
        rv = reverb if reverb is not None else get_or_create_reverb(arena.device)
        ticket, offs, block = rv.plan(*tables)
        assert int(block[1]) <= arena.numel()
        info.append(block.copy())
        rv.run(ticket, arena)
    host = arena.cpu().numpy()
    assert np.array_equal(host[:pos], front)  # sources and impulse responses are untouched
    used = np.zeros(len(host), dtype=bool)
    used[:pos] = True
    for o, n in zip(offs.tolist(), lens):
        assert o % 4 == 0 and o >= pos and not used[o : o + n].any()
        used[o : o + n] = True
    if np.isnan(fill):
        assert np.isnan(host[~used]).all()  # nothing else was written
    return [host[o : o + n].copy() for o, n in zip(offs.tolist(), lens)]


@pytest.fixture(scope="module")
def grid():
    items = _grid()
    return items, _run(items)


def test_grid_meets_both_audio_bars_against_float64(grid):
    items, got = grid
    assert len(items) > 69  # (more than the kernel arguments carry: the staged tables are exercised too)
    worst = 0.0
    for (x, hs, shift, norm), y in zip(items, got):
        truth = R.exact(x, hs, shift, norm)
        ref_rel, ref_max = R.distances(R.fft32(x, hs, shift, norm), truth)
        rel, mx = R.distances(y, truth)
        bar_rel, bar_max = R.bars(ref_rel, ref_max, truth)
        print(f"N {len(x)} L {len(hs)} shift {shift} norm {int(norm)}: device {rel:.3g} / {mx:.3g}  fft32 {ref_rel:.3g} / {ref_max:.3g}")
        assert np.isfinite(y).all()
        assert rel <= bar_rel and mx <= bar_max, (len(x), len(hs), shift, norm, rel, bar_rel, mx, bar_max)
        worst = max(worst, rel / bar_rel)
    print("worst rel-L2 / bar", worst)


def test_small_batch_in_the_kernel_arguments_equals_the_staged_route(grid):
    items, got = grid
    pick = [3, 40, len(items) - 1]
    for k, y in zip(pick, _run([items[k] for k in pick])):
        assert np.array_equal(y, got[k])


def test_zero_input_gives_zeros_and_a_unit_tap_returns_the_input():
    rng = np.random.default_rng(5)
    hs, shift = scaled_rir(_rir(rng, 300, 10))
    x = _signal(rng, 3000)
    one = np.ones(1, dtype=np.float32)
    z, u, s = _run([(np.zeros(3000, np.float32), hs, shift, True), (x, one, 0, True), (x, one * np.float32(0.5), 0, False)])
    assert np.array_equal(z, np.zeros(3000, np.float32))
    assert np.array_equal(s, x * np.float32(0.5))
    # y = x exactly, so the gain is (float)sqrt(Sx / Sx) = 1 to 1 ulp
    assert np.all(np.abs(u - x) <= np.abs(x) * np.float32(2.0 ** -23))


def test_runs_repeat_and_items_do_not_depend_on_their_neighbours(grid):
    items, got = grid
    item = next(it for it in items if len(it[0]) == 20000 and len(it[1]) == 800 and it[2] == 400 and it[3])
    alone = _run([item])[0]
    again = _run([item])[0]
    assert np.array_equal(alone, again)
    among = _run([items[1], items[30], items[50], item, items[60], items[8], items[70], items[127]])[3]
    assert np.array_equal(alone, among)


# ---- more work items than workgroups, and the three ways the table travels -------------------------------------------------------
# Sizes the shapes below sit on (tests/test_mix_abi.py::test_launch_constants_the_gpu_shapes_sit_on fails when one of them moves):
INLINE_BYTES = 3328      # kMbInlineBytes, lhotse_amd/csrc/kernel_minibatch.hpp:31: a table up to this size travels in the kernel arguments
LDS_TABLE_BYTES = 24576  # kMbLdsTableBytes, kernel_minibatch.hpp:32: a staged table up to this size is copied to LDS, a larger one searched in HBM
MAX_WORKGROUPS = 1792    # items_grid (hipfeat_reverb_run), lhotse_amd/csrc/hipfeat.hip:1910: grid = ceil(work / ceil(work / 1792))
RV_ITEM_BYTES = 48       # sizeof(RvItem), lhotse_amd/csrc/reverb_tables.hpp:30
RV_BLOCK = 2048          # kRvBlock, reverb_tables.hpp:15: outputs per work item


def _route(num_items):
    bytes_ = num_items * RV_ITEM_BYTES
    return "kernel arguments" if bytes_ <= INLINE_BYTES else "LDS copy" if bytes_ <= LDS_TABLE_BYTES else "HBM"


def _work(items, info):
    """info: what the plan that ran reported -> (its work items, the workgroups of the two launches, the pairs of normalise flags a
    workgroup meets on consecutive trips of its loop)"""
    lens = [len(x) for x, _, _, _ in items]
    work = int(info[2])
    assert work == sum(-(-n // RV_BLOCK) for n in lens) and int(info[3]) == 2 * work
    per_wg = max(1, -(-work // MAX_WORKGROUPS))
    grid = -(-work // per_wg)
    owner = np.repeat(np.arange(len(items)), [-(-n // RV_BLOCK) for n in lens])
    flags = np.array([int(f) for _, _, _, f in items])[owner]
    pairs = {(int(flags[w]), int(flags[w + grid])) for w in range(work - grid)}
    return work, grid, pairs


def _integer_batch(seed, n_of, count):
    """`count` integer-valued items: L cycles through 1, 255, 256, 257, 300 and the shifts through 0, L / 2, L - 1; normalisation is on
    for an irregular half of them."""
    rng = np.random.default_rng(seed)
    combos = [(taps, s) for taps in (1, 255, 256, 257, 300) for s in _shifts(taps)]
    norm = rng.integers(0, 2, size=count)
    return [R.integer_item(rng, n_of(k), *combos[k % len(combos)], bool(norm[k])) for k in range(count)]


def _assert_exact(items, got):
    for k, ((x, hs, shift, norm), y) in enumerate(zip(items, got)):
        assert np.array_equal(y, R.integer_expected(x, hs, shift, norm)), (k, len(x), len(hs), shift, norm)


@pytest.mark.parametrize("count,n,route", [(40, 100000, "kernel arguments"), (80, 50000, "LDS copy")])
def test_workgroups_that_take_a_second_work_item(count, n, route):
    """More than 1792 work items: every workgroup makes a second trip through both kernels' loops -- xs / hs / red / gain are re-used, the
    partials are indexed by a work item that is not blockIdx.x, and in the gain kernel a skipped item precedes a scaled one and the other
    way round.  Integer-valued items: the expected output is exact (tests/_reverb_ref.py), so the comparison is array_equal."""
    items = _integer_batch(count, lambda k: n, count)
    info = []
    got = _run(items, info=info)  # (_run: sources untouched, nothing written outside the outputs)
    work, grid, pairs = _work(items, info[0])
    print(f"{count} x {n}: {work} work items over {grid} workgroups, table {count * RV_ITEM_BYTES} B ({_route(count)}), flag pairs {sorted(pairs)}")
    assert work > MAX_WORKGROUPS and grid < work and _route(count) == route
    assert {(0, 1), (1, 0), (1, 1), (0, 0)} <= pairs
    _assert_exact(items, got)


@pytest.mark.parametrize("count", [69, 70, 512, 513, 2000])
def test_table_routes_at_their_boundaries(count):
    """69 | 70 items: the last table that fits the kernel arguments and the first that is staged; 512 | 513: the last that is searched in
    LDS and the first that is searched in HBM; 2000: HBM, and more work items (one per item) than workgroups."""
    rng = np.random.default_rng(count)
    items = [R.integer_item(rng, int(n), int(taps), int(rng.integers(0, taps)), bool(f))
             for n, taps, f in zip(rng.integers(1, 301, size=count), rng.integers(1, 41, size=count), rng.integers(0, 2, size=count))]
    info = []
    got = _run(items, info=info)
    work, grid, pairs = _work(items, info[0])
    print(f"{count} items: {work} work items over {grid} workgroups, table {count * RV_ITEM_BYTES} B ({_route(count)})")
    want = {69: "kernel arguments", 70: "LDS copy", 512: "LDS copy", 513: "HBM", 2000: "HBM"}[count]
    assert _route(count) == want and work == count and (grid < work) == (count == 2000)
    _assert_exact(items, got)
    for k in (0, count // 4, count // 2, count - 2, count - 1):
        assert np.array_equal(_run([items[k]])[0], got[k]), k


def test_plan_refuses_bad_tables_and_a_ticket_runs_once():
    rv = HipReverb("cuda:0")
    good = dict(src_offsets=[0], src_lens=[100], rir_offsets=[100], rir_lens=[20], shifts=[3], normalize=[1], tail_start=120)

    def refused(**kw):
        with pytest.raises(_lib.HipFeatError) as e:
            rv.plan(**{**good, **kw})
        assert e.value.status == _lib.ERR_INVALID

    refused(src_offsets=[-1])
    refused(rir_offsets=[-4])
    refused(src_lens=[0])
    refused(rir_lens=[0])
    refused(shifts=[-1])
    refused(shifts=[20])
    refused(tail_start=119)           # the impulse response reaches past tail_start
    refused(src_offsets=[21], rir_offsets=[0])  # the source does
    refused(tail_start=-4)
    tickets = [rv.plan(**good)[0] for _ in range(16)]
    assert tickets == list(range(16))  # none of the refused tables planned anything
    refused()  # a 17th plan
    arena = torch.zeros(120 + reverb_tail_floats([100]), dtype=torch.float32, device="cuda:0")
    with pytest.raises(_lib.HipFeatError):
        rv.run(0, arena[:150].contiguous())  # too small: nothing launched, the ticket stays
    rv.run(0, arena)
    with pytest.raises(_lib.HipFeatError) as e:
        rv.run(0, arena)
    assert e.value.status == _lib.ERR_INVALID
    with pytest.raises(_lib.HipFeatError):
        rv.run(999, arena)
    for t in tickets[1:]:
        rv.run(t, arena)
    torch.cuda.synchronize()
    assert rv.plan(**good)[0] == 16
    rv.close()


def test_transform_on_two_channels_equals_the_per_channel_items():
    rng = np.random.default_rng(9)
    x = np.stack([_signal(rng, 5000), _signal(rng, 5000)])
    rir2 = np.stack([_rir(rng, 700, 40), _rir(rng, 700, 0)])
    for rir, pairs in ((rir2[:1], [(0, 0), (1, 0)]), (rir2, [(0, 0), (1, 1)])):
        tf = HipReverbWithImpulseResponse(rir=rir, rir_channels=list(range(len(rir))), device="cuda:0")
        y = tf(x, 16000)
        assert isinstance(y, np.ndarray) and y.shape == x.shape and y.dtype == np.float32
        want = _run([(x[a],) + scaled_rir(rir[b]) + (True,) for a, b in pairs])
        for d in range(2):
            assert np.array_equal(y[d], want[d])
        yt = tf(torch.from_numpy(x).cuda(), 16000)
        assert yt.is_cuda and np.array_equal(yt.cpu().numpy(), y)
    mono = HipReverbWithImpulseResponse(rir=rir2, rir_channels=[0, 1], normalize_output=False, device="cuda:0")(x[:1], 16000)
    want = _run([(x[0],) + scaled_rir(rir2[b]) + (False,) for b in range(2)])
    assert mono.shape == (2, 5000) and np.array_equal(mono[0], want[0]) and np.array_equal(mono[1], want[1])
    with pytest.raises(ValueError):
        HipReverbWithImpulseResponse(rir=np.zeros((3, 10), np.float32), rir_channels=[0, 1, 2], device="cuda:0")(x, 16000)
    with pytest.raises(_lib.HipFeatError) as e:
        HipReverbWithImpulseResponse(rir=None)
    assert e.value.status == _lib.ERR_UNSUPPORTED


# ---- the on-the-fly route over the reference's goldens (tests/golden/reverb.*, tools/make_golden_reverb.py) --------------------
from _golden import err_stats  # noqa: E402
from _reverb_golden import GROUPS, corpus_files, exact_audio, load_reverb_goldens, rir_samples, tracks_of  # noqa: E402

from lhotse_amd.compat import LOG_EPSILON  # noqa: E402

REL_TOL, ABS_TOL = 1e-4, 2e-3  # the suite's bar for driver goldens (tests/test_gpu_reference_drivers.py)
RESAMPLER_TOL = 1e-5           # (tests/test_gpu_resample.py)
SR = 16000


@pytest.fixture(scope="module")
def goldens():
    return load_reverb_goldens()


@pytest.fixture(scope="module")
def paths(tmp_path_factory, goldens):
    return corpus_files(tmp_path_factory.mktemp("wav"), goldens[1])


@pytest.fixture(scope="module")
def routed(goldens, paths):
    """Every golden group through features_of_tracks once, with the audio -> {group: (feats, lens, audio)}."""
    arrays, meta = goldens
    out = {}
    for group in GROUPS:
        entries = meta["groups"][group]
        # groups 1-4: the reference framed every cut on its own; the K2 batch is ONE zero-padded batch
        cfg = LA.HipFbankConfig(device="cuda:0", edge_rule="batch_zero_pad") if group == "k2" else LA.HipFbankConfig(device="cuda:0")
        fm = FusedMiniBatch(LA.HipFbank(cfg), return_audio=True)
        feats, lens, audio = fm.features_of_tracks([tracks_of(e, paths, arrays) for e in entries], [e["want"] for e in entries], SR)
        out[group] = (feats.cpu().numpy(), [int(x) for x in lens], [a.numpy() for a in audio], feats.is_cuda)
    return out


@pytest.mark.parametrize("group", GROUPS)
def test_features_of_tracks_equal_the_reference_features(goldens, routed, group):
    arrays, meta = goldens
    entries = meta["groups"][group]
    got, lens, audio, on_device = routed[group]
    want = [arrays[f"{group}/{i}/feats"] for i in range(len(entries))]
    assert on_device and got.shape == (len(entries), max(len(w) for w in want), 80)
    assert lens == [len(w) for w in want]
    for i, w in enumerate(want):
        s = err_stats(got[i, : len(w)], w)
        print(group, i, s)
        assert s["rel_l2"] <= REL_TOL and s["max_abs"] <= ABS_TOL, (group, i, s)
        assert np.all(got[i, len(w) :] == np.float32(LOG_EPSILON))  # the padding rows, bit for bit
        assert len(audio[i]) == entries[i]["want"]
    if group == "k2":
        assert {"mixed", "reverb", "speed", "plain"} <= set(meta["k2_kinds"])


@pytest.mark.parametrize("group", ["reverb", "options", "speed_reverb"])
def test_returned_audio_meets_the_audio_bars(goldens, routed, group):
    arrays, meta = goldens
    checked = 0
    for i, e in enumerate(meta["groups"][group]):
        if not e["audio"]:
            continue
        got, row = routed[group][2][i], e["tracks"][0]
        truth = exact_audio(arrays, group, i)
        rel, mx = R.distances(got, truth)
        bar_rel, bar_max = R.bars(e["reference_rel_l2"], e["reference_max_abs"], truth)
        if row["factor"] != 1.0:
            # behind the device's Speed: its samples are within RESAMPLER_TOL of the CPU Speed's, and the convolution is linear, so the
            # output moves by at most RESAMPLER_TOL x gain x sum|hs|; judged against load_audio()
            hs = R.scale_and_shift(rir_samples(arrays, row["reverb"]))[0]
            slack = RESAMPLER_TOL * e["gain"] * float(np.abs(hs.astype(np.float64)).sum())
            d = float(np.abs(got.astype(np.float64) - arrays[f"{group}/{i}/audio"]).max())
            print(group, i, "max abs from load_audio()", d, "bound", slack + bar_max + e["reference_max_abs"])
            assert d <= slack + bar_max + e["reference_max_abs"], (group, i, d, slack)
        else:
            print(group, i, f"device {rel:.3g} / {mx:.3g}  reference {e['reference_rel_l2']:.3g} / {e['reference_max_abs']:.3g}")
            assert rel <= bar_rel and mx <= bar_max, (group, i, rel, bar_rel, mx, bar_max)
        checked += 1
    assert checked >= 2
