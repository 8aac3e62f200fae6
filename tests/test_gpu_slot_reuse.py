"""GPU: a staging slot's SECOND use while its first may still be in flight, with a table that has outgrown the slot -- for each of the
five ticketed handles (mix, reverb, level, collate, sinc).

A private handle gets 17 plan -> run pairs on one stream with no host synchronisation between them.  Runs 0 ... 15 carry a table of one or
two entries (the kernel-argument route where the kind has one) and make every slot allocate its first 16384 bytes; run 16 lands on
slot 0 again with a table LARGER than that, so the slot has to wait for run 0's launches, free both buffers and allocate anew before it
stages.  Every run has its own small arena; after ONE final synchronise, runs 0, 15 and 16 are held to the reference and the tolerance
of the kind's own GPU test (imported from there: nothing is restated here).

The entry points without tickets take their slots round-robin from a ring and get the same treatment: hipfeat_extract
(a plan's ring of 4), hipfeat_resample (a resampler's ring of 4) and hipfeat_stats_update (an accumulator's ring of 16).  One private
handle gets ring-size small calls and then one whose table is LARGER than any first allocation such a ring has ever made (64 KiB once,
16384 bytes now), all on one stream with no host synchronisation in between; every call writes a NaN-filled buffer of its own.  After
ONE final synchronise the first call, the last small one and the big one are bit-equal to the same call made alone, with a synchronise
behind it, on a second private handle (the accumulator: its state to that of a second one fed update by update).

The first use is PROVABLY in flight when the second comes: every run is issued on a side stream behind a stall (tests/_stalled_stream.py)
of 10 times the host time that the same small runs took on a rehearsal handle.  After tickets 0 ... 15 (the ring's small calls) are
issued the stall must still be there -- none of them has started -- and after run 16 it must be gone: the host can only have got past
``StagedSlot::wait`` by waiting for run 0, which sits behind the stall."""
import time

import numpy as np
import pytest
import torch

import _level_ref as L
import _reverb_ref as R
import _sinc_ref as SR
import test_gpu_mix
import test_gpu_reverb
import test_gpu_sinc
from _collate_ref import bits_of, collate_ref
from _hip import make_hip
from _stalled_stream import Stall, side_streams, stall_ms_for

from lhotse_amd import _lib
from lhotse_amd.augmentation import (HipCollator, HipLevel, HipMixer, HipResampleTensor, HipReverb, HipSincResampler, mixed_tail_floats, reverb_tail_floats,
                                     scaled_rir)
from lhotse_amd.stats import HipStatsAccumulator

pytestmark = pytest.mark.gpu
SLOTS = 16
FIRST_ALLOCATION = 16384  # bytes a slot holds after its first use with a small table: max(2 * bytes, 1 << 14)
RUNS = [1, 2] * (SLOTS // 2)  # entries of the tables of runs 0 ... 15
CHECKED = (0, SLOTS - 1, SLOTS)
SINC_ROW_BYTES, LEVEL_ITEM_BYTES, COLLATE_ROW_BYTES = 64, 64, 32  # sizeof(SincRow), sizeof(LvItem), sizeof(CoRow): the static_asserts of csrc/*_tables.hpp
RING = 4  # slots of a plan's and of a resampler's ring
FORMER_FIRST_ALLOCATION = 65536  # what the rings of hipfeat_extract and hipfeat_resample allocated at least before they shared StagedSlot::reserve
CUT_DESC_BYTES = 32  # sizeof(CutDesc): the static_assert of csrc/common.hpp
RES_CUT_BYTES = 32   # sizeof(ResCut), csrc/kernel_resample.hpp (tests/test_gpu_minibatch.py cites it for the mini-batch blob)
ST_CUT_BYTES = 16    # sizeof(StCut): the static_assert of csrc/stats_tables.hpp


def _lengths(rng, n):
    return [int(v) for v in rng.integers(8, 65, size=n)]


def _stall_behind(what, rehearse):
    """A stall on a side stream, 10 times the host time of ``rehearse()`` (the small runs on a handle of their own) -> (stream, stall)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rehearse()
    enqueue_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    side = side_streams()[0]
    stall = Stall(side, stall_ms_for(enqueue_ms))
    print(f"slot reuse, {what}: small runs enqueued in {enqueue_ms:.3f} ms, stall {stall.ms:.0f} ms")
    return side, stall


def _drive(handle, cases, rehearsal):
    """cases: 17 of (issue(handle) -> ticket, check(), bytes of the table), their device buffers already filled; rehearsal: the 16 small
    ones once more, for a second handle that only times their enqueue"""
    assert len(cases) == SLOTS + 1 and len(rehearsal) == SLOTS
    small, big = [c[2] for c in cases[:SLOTS]], cases[SLOTS][2]
    assert max(small) <= test_gpu_mix.INLINE_BYTES and 2 * max(small) <= FIRST_ALLOCATION < big
    twin = type(handle)("cuda:0")
    side, stall = _stall_behind(type(handle).__name__, lambda: [issue(twin) for issue, _, _ in rehearsal])
    with torch.cuda.stream(side):  # the uploads are done (_stall_behind); from here on nothing waits until run 16 needs the slot of run 0
        tickets = [issue(handle) for issue, _, _ in cases[:SLOTS]]
        assert stall.still_stalled(), "tickets 0 ... 15 were not all issued while the stream was stalled"
        tickets.append(cases[SLOTS][0](handle))
    assert not stall.still_stalled(), "run 16 took the slot of run 0 without waiting for it"
    assert tickets == list(range(SLOTS + 1)) and tickets[SLOTS] % SLOTS == 0  # run 16 reuses the slot of run 0
    torch.cuda.synchronize()
    twin.close()
    for k in CHECKED:
        cases[k][1]()
    handle.close()


def _mix_case(seed, entries):
    """entries <= 2: ONE cut of that many tracks (the second at an SNR against the first); else that many one-track cuts"""
    rng = np.random.default_rng(seed)
    rs = np.random.RandomState(seed)
    if entries <= 2:
        cuts = [test_gpu_mix._random_cut(rs, _lengths(rng, 1)[0], [(n, 3, 10.0) for n in _lengths(rng, entries - 1)])]
    else:
        cuts = [test_gpu_mix._random_cut(rs, n, []) for n in _lengths(rng, entries)]
    first, so, sl, do, snrs, refs, chunks, pos = [0], [], [], [], [], [], [], 0
    for tracks, ref in cuts:
        for x, o, snr in tracks:
            so.append(pos), sl.append(len(x)), do.append(int(o)), snrs.append(snr), chunks.append(x)
            pos += len(x)
        first.append(len(so)), refs.append(ref)
    host = np.full(((pos + 3) & ~3) + mixed_tail_floats(first, sl, do), np.nan, dtype=np.float32)
    host[:pos] = np.concatenate(chunks)
    arena, where = torch.from_numpy(host).cuda(), []

    def issue(mixer):
        ticket, offs, lens, info = mixer.plan(first, so, sl, do, snrs, refs, None, pos)
        assert int(info[1]) <= arena.numel()
        where.extend(zip(offs.tolist(), lens.tolist()))
        mixer.run(ticket, arena)
        return ticket

    def check():
        got = arena.cpu().numpy()
        test_gpu_mix._check_against_rule(cuts, [-1] * len(cuts), [got[o : o + n] for o, n in where])

    return issue, check, (len(cuts) + len(so)) * test_gpu_mix.DESCRIPTOR_BYTES


def test_mix():
    cases = [_mix_case(100 + k, n) for k, n in enumerate(RUNS)] + [_mix_case(116, 300)]
    assert cases[SLOTS][2] == 600 * test_gpu_mix.DESCRIPTOR_BYTES  # 300 cuts + 300 tracks
    _drive(HipMixer("cuda:0"), cases, [_mix_case(100 + k, n) for k, n in enumerate(RUNS)])


def _reverb_case(seed, entries):
    rng = np.random.default_rng(seed)
    items = []
    for k, n in enumerate(_lengths(rng, entries)):
        taps = int(rng.integers(1, 33))
        hs, shift = scaled_rir(test_gpu_reverb._rir(rng, taps, int(rng.integers(0, taps))))
        items.append((rng.standard_normal(n).astype(np.float32) * np.float32(0.1), hs, shift, k % 2 == 0))
    chunks, so, ro, pos = [], [], [], 0
    for x, hs, _, _ in items:
        so.append(pos), chunks.append(x)
        pos += len(x)
        ro.append(pos), chunks.append(hs)
        pos += len(hs)
    lens = [len(x) for x, _, _, _ in items]
    host = np.full(((pos + 3) & ~3) + reverb_tail_floats(lens), np.nan, dtype=np.float32)
    host[:pos] = np.concatenate(chunks)
    arena, where = torch.from_numpy(host).cuda(), []

    def issue(rv):
        ticket, offs, info = rv.plan(so, lens, ro, [len(h) for _, h, _, _ in items], [s for _, _, s, _ in items], [int(f) for _, _, _, f in items], pos)
        assert int(info[1]) <= arena.numel()
        where.extend(offs.tolist())
        rv.run(ticket, arena)
        return ticket

    def check():
        got = arena.cpu().numpy()
        for (x, hs, shift, norm), o in zip(items, where):
            y, truth = got[o : o + len(x)], R.exact(x, hs, shift, norm)
            bar_rel, bar_max = R.bars(*R.distances(R.fft32(x, hs, shift, norm), truth), truth)
            rel, mx = R.distances(y, truth)
            assert np.isfinite(y).all() and rel <= bar_rel and mx <= bar_max, (len(x), len(hs), shift, norm, rel, bar_rel, mx, bar_max)

    return issue, check, entries * test_gpu_reverb.RV_ITEM_BYTES


def test_reverb():
    cases = [_reverb_case(200 + k, n) for k, n in enumerate(RUNS)] + [_reverb_case(216, 342)]
    _drive(HipReverb("cuda:0"), cases, [_reverb_case(200 + k, n) for k, n in enumerate(RUNS)])


def _level_case(seed, entries):
    rng = np.random.default_rng(seed)
    programs = [[("volume", 0.37)], [("clip", True, -6.0, True)], [("volume", 1.9), ("clip", True, 20.0, True)]]
    items, so, pos = [], [], 0
    for k, n in enumerate(_lengths(rng, entries)):
        pos += 1 + k % 4  # sources at every residue modulo 4
        so.append(pos)
        items.append((L.signal(seed * 1000 + k, n), programs[k % 3]))
        pos += n
    host = np.full(pos + 5, np.nan, dtype=np.float32)
    for (x, _), s in zip(items, so):
        host[s : s + len(x)] = x
    arena = torch.from_numpy(host).cuda()

    def issue(level):
        ticket, info = level.plan(so, [len(x) for x, _ in items], [p for _, p in items])
        assert int(info[1]) <= arena.numel()
        level.run(ticket, arena)
        return ticket

    def check():
        got = arena.cpu().numpy()
        for (x, prog), s in zip(items, so):
            assert np.array_equal(got[s : s + len(x)], L.model32(x, prog)), (len(x), prog)

    return issue, check, entries * LEVEL_ITEM_BYTES


def test_level():
    cases = [_level_case(300 + k, n) for k, n in enumerate(RUNS)] + [_level_case(316, 257)]
    _drive(HipLevel("cuda:0"), cases, [_level_case(300 + k, n) for k, n in enumerate(RUNS)])


def _collate_case(seed, entries):
    rng = np.random.default_rng(seed)
    lens, row_len = _lengths(rng, entries), 67
    offs, pos = [], 0
    for k, n in enumerate(lens):
        pos += k % 4
        offs.append(pos)
        pos += n
    host = rng.standard_normal(pos + 5).astype(np.float32)
    dst = [k % 3 for k in range(entries)]
    arena, out = torch.from_numpy(host).cuda(), torch.full((entries, row_len), float("nan"), dtype=torch.float32, device="cuda:0")

    def issue(collator):
        ticket, info = collator.plan(offs, lens, dst, row_len, torch.float32)
        assert int(info[1]) <= arena.numel() and int(info[2]) == out.numel()
        collator.run(ticket, arena, out)
        return ticket

    def check():
        assert np.array_equal(bits_of(out.cpu()), bits_of(collate_ref(host, offs, lens, row_len, dst, torch.float32)))

    return issue, check, entries * COLLATE_ROW_BYTES


def test_collate():
    cases = [_collate_case(400 + k, n) for k, n in enumerate(RUNS)] + [_collate_case(416, 513)]
    _drive(HipCollator("cuda:0"), cases, [_collate_case(400 + k, n) for k, n in enumerate(RUNS)])


def _sinc_case(seed, entries):
    rng = np.random.default_rng(seed)
    rows = [(rng.random(n).astype(np.float32) - np.float32(0.5), test_gpu_sinc.WEIGHT_RATES[k % 2]) for k, n in enumerate(_lengths(rng, entries))]
    in_off, pos = [], 5
    for k, (x, _) in enumerate(rows):
        pos += (k % 4 - pos) % 4
        in_off.append(pos)
        pos += len(x) + 3
    out_len = [SR.resampled_length(len(x), *SR.geometry(*r)[:2]) for x, r in rows]
    out_off = []
    for k, n in enumerate(out_len):
        pos += ((k + 1) % 4 - pos) % 4
        out_off.append(pos)
        pos += n + 3
    host = np.full(pos + 64, test_gpu_sinc.FILL, dtype=np.float32)
    for o, (x, _) in zip(in_off, rows):
        host[o : o + len(x)] = x
    arena = torch.from_numpy(host).cuda()

    def issue(sinc):
        ticket, planned, info = sinc.plan(in_off, [len(x) for x, _ in rows], [r for _, r in rows], out_off, arena.numel())
        assert planned.tolist() == out_len and info[1] <= arena.numel()
        sinc.run(ticket, arena)
        return ticket

    def check():
        got = arena.cpu().numpy()
        for (x, r), o, n in zip(rows, out_off, out_len):
            assert np.abs(got[o : o + n] - SR.resample(x, *r, filt=test_gpu_sinc.filt(r))).max() <= test_gpu_sinc.ABS_TOL, (len(x), r)

    return issue, check, entries * SINC_ROW_BYTES


def test_sinc():
    cases = [_sinc_case(500 + k, n) for k, n in enumerate(RUNS)] + [_sinc_case(516, 257)]
    _drive(HipSincResampler("cuda:0"), cases, [_sinc_case(500 + k, n) for k, n in enumerate(RUNS)])


# ---- the rings of the entry points without tickets --------------------------------------------------------------------------------
def _drive_ring(make_handle, close, calls):
    """calls: RING + 1 of (issue(handle, out, stream), shape of out, bytes of the table), their inputs already on the device"""
    assert len(calls) == RING + 1
    small, big = max(c[2] for c in calls[:RING]), calls[RING][2]
    assert 4 * small <= FIRST_ALLOCATION and big > FORMER_FIRST_ALLOCATION  # the big table outgrows the slot whatever floor sized it
    checked = (0, RING - 1, RING)
    outs = [torch.full(shape, float("nan"), dtype=torch.float32, device="cuda") for _, shape, _ in calls]
    alone = {k: torch.full(calls[k][1], float("nan"), dtype=torch.float32, device="cuda") for k in checked}
    stream = torch.cuda.current_stream().cuda_stream
    handle, second = make_handle(), make_handle()
    rehearsal = [torch.empty_like(out) for out in outs[:RING]]
    side, stall = _stall_behind("ring", lambda: [issue(second, out, stream) for (issue, _, _), out in zip(calls, rehearsal)])
    for (issue, _, _), out in zip(calls[:RING], outs):  # (the uploads and fills are done: _stall_behind)
        issue(handle, out, side.cuda_stream)
    assert stall.still_stalled(), "the ring's small calls were not all issued while the stream was stalled"
    calls[RING][0](handle, outs[RING], side.cuda_stream)  # call RING lands on the slot of call 0
    assert not stall.still_stalled(), "call RING took the slot of call 0 without waiting for it"
    torch.cuda.synchronize()
    for k in checked:
        calls[k][0](second, alone[k], stream)
        torch.cuda.synchronize()
        got, want = outs[k].cpu().numpy(), alone[k].cpu().numpy()
        assert np.isfinite(want).all() and np.array_equal(got, want), (k, calls[k][1])
    close(handle), close(second)


def _extract_call(seed, cuts, longest):
    rng = np.random.default_rng(seed)
    lens = _lib.i64(rng.integers(400, longest + 1, size=cuts))
    offs = _lib.i64(np.cumsum(lens) - lens)
    wave = torch.from_numpy(rng.random(int(lens.sum()), dtype=np.float32) - np.float32(0.5)).cuda()

    def issue(ex, out, stream):
        plan = ex.plan
        plan.lib.check("hipfeat_extract", plan.handle, wave.data_ptr(), _lib.addr(offs), _lib.addr(lens), None, cuts, out.data_ptr(), None, 80, stream)

    return issue, (int(((lens + 80) // 160).sum()), 80), cuts * CUT_DESC_BYTES  # (the ragged batch's workgroup map comes on top)


def test_extract():
    calls = [_extract_call(600 + k, n, 2000) for k, n in enumerate(RUNS[:RING])] + [_extract_call(604, 2100, 800)]
    _drive_ring(lambda: make_hip("fbank", {}), lambda ex: ex.plan.close(), calls)  # (an extractor's plan is its own)


def _resample_call(seed, cuts, resampler_of_lengths):
    rng = np.random.default_rng(seed)
    lens = _lib.i64(_lengths(rng, cuts))
    out_lens = _lib.i64(resampler_of_lengths.output_lengths(lens))
    offs, out_offs = _lib.i64(np.cumsum(lens) - lens), _lib.i64(np.cumsum(out_lens) - out_lens)
    wave = torch.from_numpy(rng.random(int(lens.sum()), dtype=np.float32) - np.float32(0.5)).cuda()

    def issue(r, out, stream):
        r.lib.check("hipfeat_resample", r.handle, wave.data_ptr(), _lib.addr(offs), _lib.addr(lens), cuts, out.data_ptr(), _lib.addr(out_offs), stream)

    return issue, (int(out_lens.sum()),), cuts * RES_CUT_BYTES


def test_resample():
    make = lambda: HipResampleTensor(17600, 16000)  # noqa: E731
    lengths = make()
    assert lengths.kernel_name == "resample_fast<11,10,7>"  # a compile-time ratio
    calls = [_resample_call(700 + k, n, lengths) for k, n in enumerate(RUNS[:RING])] + [_resample_call(704, 2100, lengths)]
    _drive_ring(make, lambda r: r.close(), calls)
    lengths.close()


def test_stats():
    F = 8
    rng = np.random.default_rng(800)
    updates = []
    for cuts in RUNS + [1100]:
        frames = _lib.i64(rng.integers(1, 4, size=cuts))
        updates.append((torch.from_numpy(rng.standard_normal((int(frames.sum()), F)).astype(np.float32)).cuda(), frames))
    small, big = max(len(f) for _, f in updates[:SLOTS]) * ST_CUT_BYTES, len(updates[SLOTS][1]) * ST_CUT_BYTES
    assert 2 * small <= FIRST_ALLOCATION < big
    acc, one_by_one, twin = HipStatsAccumulator(F, "cuda:0"), HipStatsAccumulator(F, "cuda:0"), HipStatsAccumulator(F, "cuda:0")
    side, stall = _stall_behind("stats", lambda: [twin.update(feats, frames) for feats, frames in updates[:SLOTS]])
    with torch.cuda.stream(side):  # (the uploads are done: _stall_behind)
        for feats, frames in updates[:SLOTS]:
            acc.update(feats, frames)
        assert stall.still_stalled(), "updates 0 ... 15 were not all issued while the stream was stalled"
        acc.update(*updates[SLOTS])  # update 16 lands on the slot of update 0
    assert not stall.still_stalled(), "update 16 took the slot of update 0 without waiting for it"
    torch.cuda.synchronize()
    twin.close()
    for feats, frames in updates:
        one_by_one.update(feats, frames)
        torch.cuda.synchronize()
    got, want = acc.state(), one_by_one.state()
    assert got["total_frames"] == want["total_frames"] == sum(int(f.sum()) for _, f in updates)
    for key in ("total_sum", "total_unnorm_var"):
        assert np.isfinite(want[key]).all() and np.array_equal(got[key].view(np.uint64), want[key].view(np.uint64)), key
    got, want = acc.get(), one_by_one.get()
    for key in ("norm_means", "norm_stds"):
        assert np.array_equal(got[key].view(np.uint64), want[key].view(np.uint64)), key
    acc.close(), one_by_one.close()
