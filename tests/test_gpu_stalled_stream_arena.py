"""GPU: the six ticketed arena handles behind a stalled stream (the scenario: tests/_stalled_stream.py::run_scenario).

Every case takes a private handle and two calls P and Q (plan -> run through the Python wrapper, on torch's current stream) whose tables
differ; 8 rounds of (P, Q) on the default stream give each of the handle's 16 slots its first allocation and the bits to compare with.
Behind the stall the inputs arrive by a copy on the SAME stream into NaN-filled buffers, so a launch, a staging copy or a memset that is
not on the caller's stream reads NaN (or is overwritten); Q runs meanwhile from a second stream on the same handle.

Each kind runs with its tables staged through the slot's pinned and device buffers (``HIPFEAT_MB_NO_INLINE``, read at handle creation)
and with them in the kernel arguments.  References and bars are those of the kind's own GPU test; every kind claims run-to-run
bit-equality there, so the stalled results are held to the bits of the synchronised run."""
import numpy as np
import pytest
import torch

import _featmix_cases as FC
import _featmix_ref as FR
import _level_ref as L
import _sinc_ref as SR
import test_gpu_collate_channels
import test_gpu_featmix_edges
import test_gpu_mix
import test_gpu_reverb_fft
import test_gpu_sinc
from _collate_ref import bits_of, collate_ref
from _multichannel_ref import collate_sources_ref
from _stalled_stream import Call, run_scenario

from lhotse_amd import augmentation as A

pytestmark = pytest.mark.gpu
WARM_ROUNDS = 8  # x (P, Q) = the 16 slots of a ticketed handle
NAN = float("nan")
NAN16 = 0x7FFF  # a NaN in binary16 and in bfloat16: no collated row of finite samples holds it


@pytest.fixture(params=["staged", "arguments"])
def route(request, monkeypatch):
    if request.param == "staged":
        monkeypatch.setenv("HIPFEAT_MB_NO_INLINE", "1")  # read when the handle is created
    return request.param


def _arena(floats, front):
    host = torch.full((floats,), NAN, dtype=torch.float32)
    host[: len(front)] = torch.from_numpy(front)
    return host


# ---- mix ------------------------------------------------------------------------------------------------------------------------
def _mix_call(mixer, seed, shapes):
    """shapes: per cut (speech samples, [(noise samples, offset, snr)])"""
    rs = np.random.RandomState(seed)
    cuts = [test_gpu_mix._random_cut(rs, n, noises) for n, noises in shapes]
    first, so, sl, do, snrs, refs, chunks, pos = [0], [], [], [], [], [], [], 0
    for tracks, ref in cuts:
        for x, o, snr in tracks:
            so.append(pos), sl.append(len(x)), do.append(int(o)), snrs.append(snr), chunks.append(x)
            pos += len(x)
        first.append(len(so)), refs.append(ref)
    floats = ((pos + 3) & ~3) + A.mixed_tail_floats(first, sl, do)

    def run(bufs):
        ticket, offs, lens, info = mixer.plan(first, so, sl, do, snrs, refs, None, pos)
        assert int(info[1]) <= floats and int(info[2]) > 0  # (energy items: the first of the two launches runs)
        mixer.run(ticket, bufs["arena"])
        return [bufs["arena"][o : o + n] for o, n in zip(offs.tolist(), lens.tolist())]

    def check(got):
        test_gpu_mix._check_against_rule(cuts, [-1] * len(cuts), [g.numpy() for g in got])

    return Call({"arena": _arena(floats, np.concatenate(chunks))}, {}, run, check)


def test_mix(route):
    mixer = A.HipMixer("cuda:0")
    P = _mix_call(mixer, 11, [(5000, [(3000, 1201, 12.5)]), (4097, [])])
    Q = _mix_call(mixer, 12, [(2000, []), (9000, [(9000, 0, 10.0), (777, 4223, 20.0)]), (33, [(20, 3, 5.0)])])
    run_scenario(f"mix, {route}", P, Q, WARM_ROUNDS)
    mixer.close()


# ---- reverb ---------------------------------------------------------------------------------------------------------------------
MIN_FFT_TAPS = 64


def _reverb_call(rv, seed, shapes, method):
    """shapes: per item (samples, taps, shift, normalize)"""
    rng = np.random.default_rng(seed)
    items = [test_gpu_reverb_fft._item(rng, n, taps, shift, norm) for n, taps, shift, norm in shapes]
    chunks, so, ro, pos = [], [], [], 0
    for x, hs, _, _ in items:
        so.append(pos), chunks.append(x)
        pos += len(x)
        ro.append(pos), chunks.append(hs)
        pos += len(hs)
    lens, taps, shifts = [len(x) for x, _, _, _ in items], [len(h) for _, h, _, _ in items], [s for _, _, s, _ in items]
    floats = ((pos + 3) & ~3) + A.reverb_fft_tail_floats(lens, taps, shifts, ro)  # (the outputs and, an upper bound, every item's spectra)
    fft_items = sum(method == "fft" or (method == "auto" and t >= MIN_FFT_TAPS) for t in taps)

    def run(bufs):
        ticket, offs, info = rv.plan(so, lens, ro, taps, shifts, [int(f) for _, _, _, f in items], pos, method, MIN_FFT_TAPS)
        assert int(info[1]) <= floats
        if method != "direct":
            assert (int(info[5]) > 0) == (fft_items > 0)  # output blocks of the FFT route
        rv.run(ticket, bufs["arena"])
        return [bufs["arena"][o : o + n] for o, n in zip(offs.tolist(), lens)]

    def check(got):
        test_gpu_reverb_fft._assert_bars(items, [g.numpy() for g in got], f"stalled stream, {method}")

    return Call({"arena": _arena(floats, np.concatenate(chunks))}, {}, run, check), fft_items


@pytest.mark.parametrize("method", ["direct", "fft", "auto"])
def test_reverb(route, method):
    """P's impulse responses reach ``min_fft_taps`` (one does not), Q's stay under it: with "auto" one handle's tickets hold both routes."""
    rv = A.HipReverb("cuda:0")
    P, fft_p = _reverb_call(rv, 21, [(3000, 100, 40, True), (1025, 2049, 1024, False), (500, 20, 3, True)], method)
    Q, fft_q = _reverb_call(rv, 22, [(700, 30, 29, True), (2049, 63, 0, True), (64, 5, 1, False), (1, 1, 0, True)], method)
    if method == "auto":
        assert (fft_p, fft_q) == (2, 0)
    run_scenario(f"reverb {method}, {route}", P, Q, WARM_ROUNDS)
    rv.close()


# ---- level ----------------------------------------------------------------------------------------------------------------------
def _level_call(level, seed, lengths):
    programs = [[("volume", 0.37)], [("clip", True, -6.0, True)], [("volume", 1.9), ("clip", True, 20.0, True)]]
    items, so, pos = [], [], 0
    for k, n in enumerate(lengths):
        pos += 1 + k % 4  # sources at every residue modulo 4
        so.append(pos)
        items.append((L.signal(seed * 1000 + k, n), programs[(k + 1) % 3]))  # (the first item clips: the peak launch runs)
        pos += n
    host = np.full(pos + 5, np.nan, dtype=np.float32)
    for (x, _), s in zip(items, so):
        host[s : s + len(x)] = x

    def run(bufs):
        ticket, info = level.plan(so, [len(x) for x, _ in items], [p for _, p in items])
        assert int(info[1]) <= len(host)
        level.run(ticket, bufs["arena"])
        return [bufs["arena"][s : s + len(x)] for (x, _), s in zip(items, so)]

    def check(got):
        for (x, prog), g in zip(items, got):
            assert np.array_equal(g.numpy(), L.model32(x, prog)), (len(x), prog)

    return Call({"arena": torch.from_numpy(host)}, {}, run, check)


def test_level(route):
    level = A.HipLevel("cuda:0")
    run_scenario(f"level, {route}", _level_call(level, 31, [4097, 300, 9000]), _level_call(level, 32, [64, 5000, 1, 2048, 333]), WARM_ROUNDS)
    level.close()


# ---- collate --------------------------------------------------------------------------------------------------------------------
def _collate_call(collator, seed, lens, row_len, dtype, sources):
    """sources: None = ``plan``; else sources per row (0, 1 and 3 among them) = ``plan_sources``"""
    rng = np.random.default_rng(seed)
    counts = [1] * len(lens) if sources is None else sources
    first, src, pos = [0], [], 0
    for k, (n, c) in enumerate(zip(lens, counts)):
        for _ in range(c):
            pos += k % 4
            src.append(pos)
            pos += n
        first.append(len(src))
    host = rng.standard_normal(pos + 5).astype(np.float32)
    dst = [0 if k % 3 == 0 else row_len - n if k % 3 == 1 else (row_len - n) // 2 for k, n in enumerate(lens)]
    poison = NAN if dtype == torch.float32 else NAN16

    def run(bufs):
        if sources is None:
            ticket, info = collator.plan(src, lens, dst, row_len, dtype)
        else:
            ticket, info = collator.plan_sources(first, src, lens, dst, row_len, dtype)
        assert int(info[1]) <= len(host) and int(info[2]) == bufs["out"].numel()
        collator.run(ticket, bufs["arena"], bufs["out"])
        return [bufs["out"]]

    def check(got):
        if sources is None:
            assert np.array_equal(bits_of(got[0]), bits_of(collate_ref(host, src, lens, row_len, dst, dtype)))
        else:
            assert test_gpu_collate_channels.same_bits(got[0], collate_sources_ref(host, first, src, lens, row_len, dst, dtype))

    return Call({"arena": torch.from_numpy(host)}, {"out": ((len(lens), row_len), dtype, poison)}, run, check)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("form", ["plan", "plan_sources"])
def test_collate(route, form, dtype):
    collator = A.HipCollator("cuda:0")
    P = _collate_call(collator, 41, [4097, 16, 0, 1000], 4101, dtype, None if form == "plan" else [3, 1, 0, 2])
    Q = _collate_call(collator, 42, [67, 1, 33, 64, 5], 67, dtype, None if form == "plan" else [0, 3, 1, 1, 3])
    run_scenario(f"collate {form} {dtype}, {route}", P, Q, WARM_ROUNDS)
    collator.close()


# ---- sinc -----------------------------------------------------------------------------------------------------------------------
def _sinc_call(sinc, seed, lengths):
    rng = np.random.default_rng(seed)
    rows = [(rng.random(n).astype(np.float32) - np.float32(0.5), test_gpu_sinc.WEIGHT_RATES[k % 2]) for k, n in enumerate(lengths)]
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
    host = np.full(pos + 64, np.nan, dtype=np.float32)
    for o, (x, _) in zip(in_off, rows):
        host[o : o + len(x)] = x

    def run(bufs):
        ticket, planned, info = sinc.plan(in_off, [len(x) for x, _ in rows], [r for _, r in rows], out_off, len(host))
        assert planned.tolist() == out_len and info[1] <= len(host)
        sinc.run(ticket, bufs["arena"])
        return [bufs["arena"][o : o + n] for o, n in zip(out_off, out_len)]

    def check(got):
        for (x, r), g in zip(rows, got):
            assert np.abs(g.numpy() - SR.resample(x, *r, filt=test_gpu_sinc.filt(r))).max() <= test_gpu_sinc.ABS_TOL, (len(x), r)

    return Call({"arena": torch.from_numpy(host)}, {}, run, check)


def test_sinc(route):
    sinc = A.HipSincResampler("cuda:0")
    run_scenario(f"sinc, {route}", _sinc_call(sinc, 51, [64, 300, 8]), _sinc_call(sinc, 52, [33, 9, 257, 100]), WARM_ROUNDS)
    sinc.close()


# ---- featmix --------------------------------------------------------------------------------------------------------------------
def _featmix_call(mixer, case):
    F, T, host = case.F, case.row_frames, case.host
    lay = A.featmix_layout(len(host), case.cuts, F, T)
    assert lay["row_frames"] == T

    def run(bufs):
        ticket, info = mixer.plan(lay)
        assert int(info[2]) > 0 and int(info[3]) > 0  # energy items and fold items: both launches run
        mixer.run(ticket, bufs["arena"], bufs["out"])
        return [bufs["out"]]

    def check(got):
        test_gpu_featmix_edges.check(case, got[0].numpy().reshape(len(case.cuts), T, F), FR.batch(host, case.cuts, F, T))

    return Call({"arena": torch.from_numpy(host)}, {"out": ((len(case.cuts) * T * F,), torch.float32, NAN)}, run, check)


def test_featmix(route):
    """P and Q: two cases of tests/_featmix_cases.py (a fold of two tracks, one at an SNR, with a repeated and with a dropped last frame)."""
    by_name = {c.name: c for c in FC.CASES}
    mixer = A.HipFeatureMixer("cuda:0")
    run_scenario(f"featmix, {route}", _featmix_call(mixer, by_name["rep_fold_F23_178"]), _featmix_call(mixer, by_name["drop_fold_F1_4098"]), WARM_ROUNDS)
    mixer.close()
