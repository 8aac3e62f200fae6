"""GPU: every device entry point with buffers of more than 2^31 elements.

All of them take 64-bit element offsets or sizes (CutDesc::wave_off / out_row, ResCut::in_off / out_off, MixTrack::src_off,
MixCut::out_off, RvItem::src_off / rir_off / out_off, LvItem::src_off / dst_off; the sizes of hipfeat_global_mvn, hipfeat_float_to_half,
hipfeat_pcm16_to_float, hipfeat_specaug) and handle them with hand-written code: descriptors pulled dword by dword through
v_readfirstlane, offsets rebuilt as (hi << 32) | lo, unsigned byte offsets added to a pointer, SGPR base + 32-bit lane offset stores.
No other test makes the upper dword of any of these values non-zero.

Two buffers of 2^31 + 2^24 float32 (8.06 GiB each, module fixture) hold everything.  Items sit where tests/_large_buffers.py puts them:
astride and behind byte offset 2^31 (float 2^29), byte offset 2^32 (float 2^30) and element index 2^31.  The bar is DERIVED, not measured:
the same call on the "near twin" -- the same items at the same offsets modulo 4 in a buffer of a few hundred thousand floats -- executes the
same instructions on the same operands, so far == near bit for bit; the near result is held to the family's float64 reference at the bar
its own test module uses; and nothing outside the items' windows may change (a store whose address wrapped modulo 2^32 bytes lands at a
lower address INSIDE the buffer: no fault, but the count of written elements breaks).  Whole-buffer work (fill, count, compare) stays on
the device, in chunks of at most 2^28 elements where it would otherwise make a temporary of the buffer's size.

Each test prints the largest element index it saw read and written correctly ("[far] ..." lines; pytest -s).
"""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import _large_buffers as LB
import _level_ref as LV
import _reverb_ref as RV
from _golden import err_stats, ref32
from _hip import make_hip
from _mix_ref import mix_tracks

import lhotse_amd as LA
from lhotse_amd import _lib
from lhotse_amd import augmentation as A
from oracle import kaldi_ref as K
from oracle import librosa_ref
from oracle import resample_ref
from oracle import specaug_ref
from oracle import whisper_ref

pytestmark = pytest.mark.gpu

FILL = 0.25          # what `wave` holds wherever no item lies: a load whose address wrapped reads this (or another item)
CHUNK = 2 ** 28      # elements per whole-buffer device op that makes a temporary
NEED_FREE = 24 << 30
INT32_MAX = 2 ** 31 - 1
LOG_EPSILON = -23.025850929940457
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the two buffers ---------------------------------------------------------------------------------------------------------------
class Buffers:
    def __init__(self):
        self.wave = torch.empty(LB.BUFFER_ELEMS, dtype=torch.float32, device="cuda")
        self.out = torch.empty(LB.BUFFER_ELEMS, dtype=torch.float32, device="cuda")
        self.wave_is_filled = False

    def filled_wave(self) -> torch.Tensor:
        """`wave`, holding FILL everywhere (filled once; a test that dirties it restores its windows, or marks it)."""
        if not self.wave_is_filled:
            self.wave.fill_(FILL)
            self.wave_is_filled = True
        return self.wave

    def nan_out(self) -> torch.Tensor:
        self.out.fill_(float("nan"))
        return self.out


@pytest.fixture(scope="module")
def bufs():
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"the large-offset tests need 24 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    torch.cuda.reset_peak_memory_stats()
    b = Buffers()
    yield b
    peak = torch.cuda.max_memory_allocated()
    print(f"[far] peak device memory of the module: {peak / 2 ** 30:.2f} GiB")
    del b.wave, b.out
    torch.cuda.empty_cache()
    assert peak < 20 << 30, peak


def _count(t: torch.Tensor, pred) -> int:
    """Elements of the 1-D tensor `t` for which `pred(chunk)` holds: on the device, chunk by chunk."""
    total = torch.zeros((), dtype=torch.int64, device=t.device)
    for c in t.split(CHUNK):
        total += pred(c).sum()
    return int(total)


def _not_nan(t):
    return _count(t, lambda c: c == c)


def _differs(t, value=FILL):
    return _count(t, lambda c: c != value)


def _put(buf, offsets, arrays):
    for o, x in zip(offsets, arrays):
        buf[int(o) : int(o) + len(x)] = torch.from_numpy(np.ascontiguousarray(x)).to(buf.device)


def _clear(buf, offsets, lengths, value=FILL):
    for o, n in zip(offsets, lengths):
        buf[int(o) : int(o) + int(n)] = value


def _get(buf, offsets, lengths):
    return [buf[int(o) : int(o) + int(n)].clone() for o, n in zip(offsets, lengths)]


def _sig(seed, n, amp=1.0):
    return ((np.random.RandomState(seed).rand(int(n)).astype(np.float32) - np.float32(0.5)) * np.float32(amp)).astype(np.float32)


@contextlib.contextmanager
def _env(switches):
    old = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _report(what, read_to=None, wrote_to=None):
    parts = [f"[far] {what}:"]
    if read_to is not None:
        parts.append(f"read up to element {int(read_to)} (2^31 + {int(read_to) - 2 ** 31})")
    if wrote_to is not None:
        parts.append(f"wrote up to element {int(wrote_to)} (2^31 + {int(wrote_to) - 2 ** 31})")
    print(" ".join(parts))


# ---- feature kernels: every family, through the C ABI -------------------------------------------------------------------------------
# (id, family, kind, config, switches while the plan is created, kernel name: prefix, substring, bar)
PLANS = [
    ("fft512c-fbank80", "kaldi", "fbank", {}, {}, "fft512c_kernel", "", "parity"),
    ("fft512c-mfcc", "kaldi", "mfcc", {}, {}, "fft512c_kernel<13> mfcc", "", "parity"),
    ("fft512b-logmel", "kaldi", "fbank", {}, {"HIPFEAT_FFT512_VARIANT": "b"}, "fft512b_kernel", "", "parity"),
    ("fft512b-spectrogram", "kaldi", "spectrogram", {}, {}, "fft512b_kernel", " spectrogram ", "parity"),
    ("fft256c-8k", "kaldi", "fbank", {"sampling_rate": 8000}, {}, "fft256c_kernel", "", "fft256"),
    ("fft256-tile-8k", "kaldi", "fbank", {"sampling_rate": 8000}, {"HIPFEAT_FFT256_VARIANT": "b"}, "fft256_kernel", "", "fft256"),
    ("fft1024c-24k", "kaldi", "fbank", {"sampling_rate": 24000}, {}, "fft1024c_kernel", "", "rates"),
    ("fft2048c-48k", "kaldi", "fbank", {"sampling_rate": 48000}, {}, "fft2048c_kernel<19,0>", "", "rates"),
    ("fft2048c-44k", "kaldi", "fbank", {"sampling_rate": 44100}, {}, "fft2048c_kernel<18,1>", "", "rates"),
    ("wave-use-energy", "kaldi", "fbank", {"use_energy": True}, {}, "wave_kernel<4>", "", "floor"),
    ("generic", "kaldi", "fbank", {}, {"HIPFEAT_FORCE_GENERIC": "1"}, "generic", "", "floor"),
    ("whisper3-80", "whisper", None, {"num_filters": 80}, {}, "whisper3_kernel", "", "whisper"),
    ("whisper2-23", "whisper", None, {"num_filters": 23}, {}, "whisper_kernel2", "", "whisper"),
    ("librosa", "librosa", None, {}, {}, "fft1024c_kernel<32>", "", "librosa"),
]
PLAN_BY_ID = {p[0]: p for p in PLANS}
DURATIONS = (0.4, 0.55, 0.7, 0.85, 1.0, 1.2, 1.4)  # seconds: the ragged batch (lengths made odd)
_EXTRACTORS = {}


def _extractor(plan_id):
    if plan_id not in _EXTRACTORS:
        _, family, kind, cfg, switches, prefix, part, _ = PLAN_BY_ID[plan_id]
        with _env(switches):
            if family == "kaldi":
                ex = make_hip(kind, cfg)
            elif family == "whisper":
                ex = LA.HipWhisperFbank(LA.HipWhisperFbankConfig(**cfg))
            else:
                ex = LA.HipLibrosaFbank(LA.HipLibrosaFbankConfig(**cfg))
            name = ex.kernel_name  # (plans are created lazily: touch it while the switches are set)
        assert name.startswith(prefix) and part in name, (plan_id, name)
        _EXTRACTORS[plan_id] = ex
    return _EXTRACTORS[plan_id]


def _sampling_rate(plan_id, ex):
    family, cfg = PLAN_BY_ID[plan_id][1], PLAN_BY_ID[plan_id][3]
    return int(ex.config.sampling_rate) if family == "librosa" else int(cfg.get("sampling_rate", 16000))


def _judge(plan_id, ex, x, got):
    """The near result against the family's float64 reference, with the bar of the family's own test module."""
    _, family, kind, cfg, _, _, _, bar = PLAN_BY_ID[plan_id]
    ctx = (plan_id, len(x))
    if bar == "whisper":  # tests/test_gpu_whisper.py::test_mfma_dft_kernel_agrees_with_the_generic_direct_dft: 2e-4 against float64
        truth = whisper_ref.log_mel_spectrogram(x, whisper_ref.slaney_mel_filters(16000, 400, cfg["num_filters"]), dtype=np.float64)
        assert got.shape == truth.shape and np.abs(got - truth).max() <= 2e-4, (ctx, np.abs(got - truth).max())
        return
    if bar == "librosa":  # tests/test_gpu_librosa.py::_close, broadband input
        from test_gpu_librosa import _close

        _close(got, librosa_ref.logmelfilterbank(x), ctx)
        return
    fields = {k: v for k, v in cfg.items() if k in K.RefConfig.__dataclass_fields__}
    if kind == "mfcc":
        fields.setdefault("num_filters", 23)
    rc = K.RefConfig(kind=kind, **fields)
    want, truth = ref32(rc).extract(x), K.RefExtractor(rc, np.float64).extract(x)
    assert got.shape == want.shape == truth.shape, ctx
    if bar == "parity":  # tests/test_gpu_parity.py::assert_parity (1e-4 rel-L2, 2e-3 max abs; the MFCC clause of its docstring)
        from test_gpu_parity import assert_parity

        assert_parity(got, want, truth, ctx, suite="large_offsets", kernel=ex.kernel_name, kind=kind)
        if kind == "spectrogram":
            assert err_stats(got, want)["frac_within"] >= 0.9995
    elif bar == "fft256":  # tests/test_gpu_fft256.py::test_fft256_fast_path_matches_oracle_and_generic
        floor = np.linalg.norm(want - truth) / np.linalg.norm(truth)
        rel = np.linalg.norm(got - truth) / np.linalg.norm(truth)
        assert rel <= max(1e-4, 3 * floor), (ctx, rel, floor)
        assert np.abs(got - truth).max() <= max(2e-3, 3 * np.abs(want - truth).max()), ctx
    elif bar == "rates":  # tests/test_gpu_fft2048.py, tests/test_gpu_fixed_schedule.py
        s = err_stats(got, want)
        assert s["rel_l2"] <= 1e-4 and s["max_abs"] <= max(2e-3, 3 * err_stats(want, truth)["max_abs"]), (ctx, s)
    else:  # "floor", tests/test_gpu_random_configs.py: rel <= max(1e-4, 3 x floor)
        den = max(np.linalg.norm(truth), 1e-30)
        rel, floor = np.linalg.norm(got - truth) / den, np.linalg.norm(want - truth) / den
        assert rel <= max(1e-4, 3 * floor), (ctx, rel, floor)


def _extract(plan, wave, offsets, lengths, out, rows, stride, route):
    L, stream = plan.lib, torch.cuda.current_stream().cuda_stream
    offsets, lengths, rows = _lib.i64(offsets), _lib.i64(lengths), _lib.i64(rows)
    if route == "layout":
        h = np.zeros(1, dtype=np.uint64)
        L.check("hipfeat_layout_create", plan.handle, len(lengths), _lib.addr(offsets), _lib.addr(lengths), None, _lib.addr(rows), int(stride), stream, _lib.addr(h))
        try:
            L.check("hipfeat_extract_layout", plan.handle, int(h[0]), wave.data_ptr(), out.data_ptr(), stream)
            torch.cuda.synchronize()
        finally:
            L.check("hipfeat_layout_destroy", int(h[0]))
    else:
        L.check("hipfeat_extract", plan.handle, wave.data_ptr(), _lib.addr(offsets), _lib.addr(lengths), None, len(lengths), out.data_ptr(),
                _lib.addr(rows), int(stride), stream)
        torch.cuda.synchronize()


def _rows_of(out, rows, frames, stride, F):
    return [out[int(r) * stride : (int(r) + int(t)) * stride].view(int(t), stride) for r, t in zip(rows, frames)]


def _feature_case(bufs, plan_id, shape, route="transient", stride=None):
    ex = _extractor(plan_id)
    plan = ex.plan
    sr, F = _sampling_rate(plan_id, ex), plan.feature_dim
    stride = F if stride is None else stride
    if shape == "ragged":
        pw = LB.place([int(sr * d) | 1 for d in DURATIONS])
    else:  # four equal cuts: the uniform workgroups-per-cut path
        pw = LB.place_behind(int(sr * 0.9) | 1)
    LB.check(pw)
    lens = pw.lengths
    waves = [_sig(1000 + 17 * i + len(plan_id), n) for i, n in enumerate(lens)]
    frames = [int(t) for t in plan.frame_counts(np.array(lens, dtype=np.int64), None)]
    pr = LB.place(frames, stride) if shape == "ragged" else LB.place_behind(frames[0], stride)
    LB.check(pr)
    written = sum(frames) * F

    def run(wave, out, woffs, rows):
        _put(wave, woffs, waves)
        _extract(plan, wave, woffs, lens, out, rows, stride, route)
        blocks = _rows_of(out, rows, frames, stride, F)
        assert all(bool(torch.isfinite(b[:, :F]).all()) for b in blocks)  # every element inside the cuts' rows was written
        assert _not_nan(out) == written  # ... and nothing else (the columns [F, stride) of the rows included)
        return [b[:, :F].clone() for b in blocks]

    # the near twin, and the reference
    wave_n = torch.full((pw.near_size,), FILL, dtype=torch.float32, device="cuda")
    out_n = torch.full((pr.near_size * stride,), float("nan"), dtype=torch.float32, device="cuda")
    near = run(wave_n, out_n, pw.near, pr.near)
    for x, y in zip(waves, near):
        _judge(plan_id, ex, x, y.cpu().numpy())
    # the same call with every offset's upper bits set
    wave = bufs.filled_wave()
    out = bufs.nan_out()
    try:
        far = run(wave, out, pw.far, pr.far)
    finally:
        _clear(wave, pw.far, lens)
    for i, (a, b) in enumerate(zip(far, near)):
        assert torch.equal(a, b), (plan_id, shape, route, i, pw.roles[i], pw.marks[i], float((a - b).abs().max()))
    _report(f"hipfeat_extract{'_layout' if route == 'layout' else ''} {plan_id} {shape} stride {stride} ({ex.kernel_name.split(' ')[0]})",
            read_to=pw.far[-1] + lens[-1] - 1, wrote_to=(pr.far[-1] + frames[-1] - 1) * stride + F - 1)


@pytest.mark.parametrize("shape", ["ragged", "uniform"])
@pytest.mark.parametrize("plan_id", [p[0] for p in PLANS])
def test_feature_kernels_read_and_write_behind_every_mark(bufs, plan_id, shape):
    _feature_case(bufs, plan_id, shape)


@pytest.mark.parametrize("shape", ["ragged", "uniform"])
def test_layout_route_behind_every_mark(bufs, shape):
    _feature_case(bufs, "fft512c-fbank80", shape, route="layout")


@pytest.mark.parametrize("shape", ["ragged", "uniform"])
def test_odd_row_stride_behind_every_mark(bufs, shape):
    _feature_case(bufs, "fft512c-fbank80", shape, stride=83)


# ---- the collated route past 2^31 output floats ------------------------------------------------------------------------------------
def _collated_into(plan, wave, offsets, lengths, out, pad_value, pair):
    """What Plan.run_collated does on either of its routes -- the launch pair of hipfeat_minibatch_* (a bank without resamplers) or
    hipfeat_extract_collated -- but into `out` instead of a third allocation of 8 GiB.  -> (frame counts, rows per cut)"""
    lib, B = plan.lib, len(lengths)
    stream = torch.cuda.current_stream().cuda_stream
    if pair:
        bank = plan._pair_bank()
        res, info = np.empty((3, B), dtype=np.int64), np.zeros(4, dtype=np.int64)
        idx = np.full(B, -1, dtype=np.int32)
        lib.check("hipfeat_minibatch_plan", bank.handle, plan.handle, B, _lib.addr(offsets), _lib.addr(lengths), _lib.addr(idx), None, wave.numel(), 0, 0, None,
                  _lib.addr(res[0]), _lib.addr(res[1]), _lib.addr(res[2]), None, _lib.addr(info))
        tmax = int(info[2])
        assert B * tmax * plan.feature_dim <= out.numel()
        lib.check("hipfeat_minibatch_run", bank.handle, int(info[0]), wave.data_ptr(), wave.numel(), out.data_ptr(), tmax, float(pad_value), stream)
        frames = res[2].copy()
    else:
        frames = plan.frame_counts(lengths, None)
        tmax = int(frames.max())
        got = np.zeros(B, dtype=np.int64)
        assert B * tmax * plan.feature_dim <= out.numel()
        lib.check("hipfeat_extract_collated", plan.handle, wave.data_ptr(), _lib.addr(offsets), _lib.addr(lengths), None, B, out.data_ptr(), tmax, float(pad_value),
                  _lib.addr(got), stream)
        assert np.array_equal(got, frames)
    torch.cuda.synchronize()
    return frames, tmax


@pytest.fixture(scope="module")
def headline_signal():
    """One 10 s signal, its 7.3 s prefix, and what the reference gives for both (computed once, shared by the two routes)."""
    x = _sig(77, 160000)
    short = x[:116800]
    rc = K.RefConfig(kind="fbank")
    o32, o64 = ref32(rc), K.RefExtractor(rc, np.float64)
    return x, short, {"full": (o32.extract(x), o64.extract(x)), "short": (o32.extract(short), o64.extract(short))}


@pytest.mark.parametrize("route", ["launch-pair", "extract-collated"])
def test_collated_output_past_2_31_floats(bufs, headline_signal, route):
    """27 000 cuts that all point at the same 10 s of samples (reading is aliasing-safe), every 2700th only at its first 7.3 s:
    27 000 x 1000 x 80 = 2.16e9 output floats, the smallest batch that crosses 2^31 on this route."""
    from test_gpu_parity import assert_parity

    x, short, refs = headline_signal
    ex = _extractor("fft512c-fbank80")
    plan = ex.plan
    B, T, F = 27000, 1000, 80
    is_short = np.arange(B) % 2700 == 2699
    lengths = np.where(is_short, len(short), len(x)).astype(np.int64)
    offsets = np.zeros(B, dtype=np.int64)
    sig = torch.from_numpy(x).cuda()
    out = bufs.nan_out()
    frames, tmax = _collated_into(plan, sig, offsets, lengths, out, LOG_EPSILON, pair=route == "launch-pair")
    assert tmax == T and B * T * F > 2 ** 31 and frames.tolist() == np.where(is_short, 730, 1000).tolist()
    cuts = out[: B * T * F].view(B, T * F)
    first_short = int(np.flatnonzero(is_short)[0])
    same = torch.empty(B, dtype=torch.bool, device="cuda")
    for b0 in range(0, B, 3000):  # 3000 x 80 000 floats per compare: under 2^28
        same[b0 : b0 + 3000] = (cuts[b0 : b0 + 3000] == cuts[0][None, :]).all(dim=1)
    for b in np.flatnonzero(is_short):  # (padding rows included)
        assert not bool(same[b])
        same[b] = torch.equal(cuts[b], cuts[first_short])
    bad = torch.nonzero(~same).flatten().tolist()
    assert not bad, (route, len(bad), bad[:8])
    assert _not_nan(out) == B * T * F
    s0 = cuts[first_short].view(T, F)
    assert bool((s0[730:] == np.float32(LOG_EPSILON)).all())  # the padding rows hold the pad value, exactly
    assert_parity(cuts[0].view(T, F).cpu().numpy(), *refs["full"], (route, "full"), suite="large_offsets", kernel=ex.kernel_name)
    assert_parity(s0[:730].cpu().numpy(), *refs["short"], (route, "short"), suite="large_offsets", kernel=ex.kernel_name)
    _report(f"collated {route} ({'hipfeat_minibatch_run' if route == 'launch-pair' else 'hipfeat_extract_collated'})", wrote_to=B * T * F - 1)


# ---- arena kernels ------------------------------------------------------------------------------------------------------------------
def _outside_is_untouched(arena, offsets, lengths):
    """No element of `arena` outside the given windows differs from FILL (counted on the device)."""
    inside = sum(int((arena[int(o) : int(o) + int(n)] != FILL).sum()) for o, n in zip(offsets, lengths))
    assert _differs(arena) == inside


RESAMPLERS = [("generic", 17600, 16000, {"HIPFEAT_RESAMPLE_GENERIC": "1"}, "resample_generic"),
              ("fast", 17600, 16000, {}, "resample_fast<11,10,7>"),
              ("mfma", 44100, 16000, {}, "resample_mfma")]


@pytest.mark.parametrize("which,orig,new,switches,kernel", RESAMPLERS, ids=[r[0] for r in RESAMPLERS])
def test_resample_reads_and_writes_behind_every_mark(bufs, which, orig, new, switches, kernel):
    with _env(switches):
        r = A.HipResampleTensor(orig, new)
    assert r.kernel_name == kernel, r.kernel_name
    lens = [4097, 16001, 2561, 52345, 255, 70001, 8191]
    xs = [_sig(300 + i, n) for i, n in enumerate(lens)]
    out_lens = [int(n) for n in r.output_lengths(np.array(lens))]
    pi, po = LB.place(lens), LB.place(out_lens)
    LB.check(pi), LB.check(po)

    def run(src, dst, ioffs, ooffs):
        _put(src, ioffs, xs)
        stream = torch.cuda.current_stream().cuda_stream
        io, oo, ln = _lib.i64(ioffs), _lib.i64(ooffs), _lib.i64(lens)
        r.lib.check("hipfeat_resample", r.handle, src.data_ptr(), _lib.addr(io), _lib.addr(ln), len(lens), dst.data_ptr(), _lib.addr(oo), stream)
        torch.cuda.synchronize()
        ys = _get(dst, ooffs, out_lens)
        assert all(bool(torch.isfinite(y).all()) for y in ys) and _not_nan(dst) == sum(out_lens)
        _outside_is_untouched(src, ioffs, lens)  # the inputs' buffer is only read
        return ys

    near = run(torch.full((pi.near_size,), FILL, device="cuda"), torch.full((po.near_size,), float("nan"), device="cuda"), pi.near, po.near)
    for x, y in zip(xs, near):
        want = resample_ref.resample(x, orig, new, dtype=np.float64)
        assert y.numel() == len(want) and np.abs(y.cpu().numpy() - want).max() <= 1e-5, (which, len(x))
    wave, out = bufs.filled_wave(), bufs.nan_out()
    try:
        far = run(wave, out, pi.far, po.far)
    finally:
        _clear(wave, pi.far, lens)
    for i, (a, b) in enumerate(zip(far, near)):
        assert torch.equal(a, b), (which, i, pi.roles[i], pi.marks[i])
    _report(f"hipfeat_resample {kernel}", read_to=pi.far[-1] + lens[-1] - 1, wrote_to=po.far[-1] + out_lens[-1] - 1)


def test_minibatch_pair_with_the_cuts_at_the_marks_and_the_tail_above_2_31(bufs):
    from test_gpu_minibatch import _round3_route

    ex = _extractor("fft512c-fbank80")
    lens = np.array([24001, 16001, 40001, 9001, 31001, 60001, 12001], dtype=np.int64)
    fac = np.array([1.0, 0.9, 1.1, 1.0, 1.1, 0.9, 1.0])
    xs = [_sig(500 + i, n) for i, n in enumerate(lens)]
    p = LB.place(lens.tolist())
    LB.check(p)
    bank = A.HipSpeedBank([0.9, 1.1], 16000, "cuda")
    idx = bank.index_of(fac)
    tail_floats = A.perturbed_tail_floats(lens, fac, 16000)

    def run(arena, offs, front):
        offs = _lib.i64(offs)
        _put(arena, offs, xs)
        feats, frames, po, pl = bank.extract_collated(ex.plan, arena, offs, lens, idx, front, LOG_EPSILON)
        torch.cuda.synchronize()
        po, pl = po.copy(), pl.copy()
        assert all(int(o) >= front for o, f in zip(po, fac) if f != 1.0) and all(int(o) == int(q) for o, q, f in zip(po, offs, fac) if f == 1.0)
        tail = [(int(o), int(n)) for o, n, f in zip(po, pl, fac) if f != 1.0]
        _outside_is_untouched(arena, list(offs) + [o for o, _ in tail], list(lens) + [n for _, n in tail])
        return feats, np.asarray(frames).copy(), _get(arena, po, pl), po, pl

    front_n = (p.near_size + 3) & ~3
    arena_n = torch.full((front_n + tail_floats,), FILL, device="cuda")
    feats_n, frames_n, waves_n, po_n, pl_n = run(arena_n, p.near, front_n)
    # the bar of tests/test_gpu_minibatch.py: bit-identical to one hipfeat_resample launch per factor + hipfeat_extract_collated
    clean = torch.full_like(arena_n, FILL)
    _put(clean, p.near, xs)
    want_feats, want_frames, want_waves = _round3_route(ex, clean, _lib.i64(p.near), lens, fac, front_n)
    assert np.array_equal(frames_n, want_frames) and torch.equal(feats_n, want_feats)
    assert all(torch.equal(a, b) for a, b in zip(waves_n, want_waves))
    front = (p.far[-1] + int(lens[-1]) + 3) & ~3  # 2^31 + a little: the perturbed tail lies wholly above 2^31
    assert front > 2 ** 31 and front + tail_floats <= LB.BUFFER_ELEMS
    wave = bufs.filled_wave()
    try:
        feats, frames, waves, po, pl = run(wave, p.far, front)
    finally:
        bufs.wave_is_filled = False  # (the tail was written: fill again)
    assert np.array_equal(frames, frames_n) and np.array_equal(pl, pl_n) and torch.equal(feats, feats_n)
    assert np.array_equal((po - front)[fac != 1.0], (po_n - front_n)[fac != 1.0])
    assert all(torch.equal(a, b) for a, b in zip(waves, waves_n))
    _report("hipfeat_minibatch_run (prep + feature launch)", read_to=int((po + pl).max()) - 1, wrote_to=int((po + pl).max()) - 1)
    bank.close()


def test_mix_tracks_at_the_marks_and_the_mixed_cuts_above_2_31(bufs):
    from test_gpu_mix import _check_against_rule

    lens = [9001, 30001, 257, 20001, 257, 40001, 12289]
    p = LB.place(lens)
    LB.check(p)
    used = [0, 1, 3, 5, 6]  # control, astride 2^29, astride 2^30, astride 2^31, behind 2^31
    x = {i: _sig(600 + i, lens[i], 0.6 if i in (3, 5, 6) else 0.3) for i in used}
    # (source item or -1 = a padding track, samples, offset in the cut, SNR) per track; the reference track of every cut is its first
    cuts = [[(5, lens[5], 0, None), (1, lens[1], 4000, 10.0)],
            [(3, lens[3], 0, None), (-1, 25000, 0, None)],  # a padding track: src_off = -1, upper dword all ones
            [(6, lens[6], 0, None), (0, lens[0], 1000, 5.0)]]
    first = [0, 2, 4, 6]
    sl = [n for c in cuts for _, n, _, _ in c]
    do = [o for c in cuts for _, _, o, _ in c]
    snrs = [s for c in cuts for _, _, _, s in c]
    refs = [0, 0, 0]
    rule_cuts = [([(n if i < 0 else x[i], o, s) for i, n, o, s in c], 0) for c in cuts]
    tail_floats = A.mixed_tail_floats(first, sl, do)

    def run(arena, offs, front):
        so = [-1 if i < 0 else int(offs[i]) for c in cuts for i, _, _, _ in c]
        _put(arena, [offs[i] for i in used], [x[i] for i in used])
        mo, ml = A.mix_in_arena(arena, first, so, sl, do, snrs, refs, None, front)
        torch.cuda.synchronize()
        assert all(int(o) >= front and int(o) % 4 == 0 for o in mo)
        _outside_is_untouched(arena, [offs[i] for i in used] + list(mo), [lens[i] for i in used] + list(ml))
        return _get(arena, mo, ml), mo.copy(), ml.copy()

    front_n = (p.near_size + 3) & ~3
    near, mo_n, ml_n = run(torch.full((front_n + tail_floats,), FILL, device="cuda"), p.near, front_n)
    _check_against_rule(rule_cuts, [None] * 3, [y.cpu().numpy() for y in near])  # the bar of tests/test_gpu_mix.py for synthetic cuts
    plain = mix_tracks(rule_cuts[1][0], -1)  # no SNR in this cut: the plain sum (here: the speech, then zeros), bit for bit
    assert np.array_equal(near[1].cpu().numpy(), plain) and len(plain) == 25000
    front = (p.far[-1] + lens[-1] + 3) & ~3
    assert front > 2 ** 31 and front + tail_floats <= LB.BUFFER_ELEMS
    wave = bufs.filled_wave()
    try:
        far, mo, ml = run(wave, p.far, front)
    finally:
        bufs.wave_is_filled = False
    assert np.array_equal(ml, ml_n) and np.array_equal(mo - front, mo_n - front_n)
    for i, (a, b) in enumerate(zip(far, near)):
        assert torch.equal(a, b), (i, float((a - b).abs().max()))
    _report("hipfeat_mix_run (energies + mix)", read_to=p.far[6] + lens[6] - 1, wrote_to=int((mo + ml).max()) - 1)


def test_reverb_source_impulse_response_and_output_at_different_marks(bufs):
    from test_gpu_reverb import _rir, _signal

    rng = np.random.default_rng(31)
    lens = [9, 4097, 300, 300, 300, 20001, 9]
    p = LB.place(lens)
    LB.check(p)
    # item A: source astride 2^29, impulse response behind 2^30; item B (normalised): source astride 2^31, impulse response astride 2^30;
    # both outputs above 2^31.  300 taps: a second chunk of 256 taps.
    src = {1: _signal(rng, lens[1]), 5: _signal(rng, lens[5])}
    hs_a, shift_a = A.scaled_rir(_rir(rng, 300, 40))
    hs_b, shift_b = A.scaled_rir(_rir(rng, 300, 299))
    items = [(src[1], hs_a, shift_a, False), (src[5], hs_b, shift_b, True)]
    where = [(1, 4), (5, 3)]  # (placement of the source, of the impulse response)
    n = [len(it[0]) for it in items]
    tail_floats = A.reverb_tail_floats(n)

    def run(arena, offs, front):
        so, ro = [offs[s] for s, _ in where], [offs[r] for _, r in where]
        _put(arena, so + ro, [it[0] for it in items] + [it[1] for it in items])
        oo = A.reverb_in_arena(arena, so, n, ro, [300, 300], [it[2] for it in items], [int(it[3]) for it in items], front)
        torch.cuda.synchronize()
        assert all(int(o) >= front and int(o) % 4 == 0 for o in oo)
        _outside_is_untouched(arena, so + ro + list(oo), n + [300, 300] + n)
        return _get(arena, oo, n), oo.copy()

    front_n = (p.near_size + 3) & ~3
    near, oo_n = run(torch.full((front_n + tail_floats,), FILL, device="cuda"), p.near, front_n)
    for (xx, hs, shift, norm), y in zip(items, near):  # the two audio bars of tests/test_gpu_reverb.py
        truth = RV.exact(xx, hs, shift, norm)
        rel, mx = RV.distances(y.cpu().numpy(), truth)
        bar_rel, bar_max = RV.bars(*RV.distances(RV.fft32(xx, hs, shift, norm), truth), truth)
        assert rel <= bar_rel and mx <= bar_max, (len(xx), norm, rel, bar_rel, mx, bar_max)
    front = (p.far[-1] + lens[-1] + 3) & ~3
    assert front > 2 ** 31 and front + tail_floats <= LB.BUFFER_ELEMS
    wave = bufs.filled_wave()
    try:
        far, oo = run(wave, p.far, front)
    finally:
        bufs.wave_is_filled = False
    assert np.array_equal(oo - front, oo_n - front_n)
    for i, (a, b) in enumerate(zip(far, near)):
        assert torch.equal(a, b), (i, float((a - b).abs().max()))
    _report("hipfeat_reverb_run (convolution + gain)", read_to=p.far[5] + lens[5] - 1, wrote_to=int(oo[-1]) + n[-1] - 1)


with open(os.path.join(GOLDEN, "level.json")) as _f:
    _SOFT_FIGURES = {c["name"]: c for c in json.load(_f)["soft_cases"]}
_SOFT = {c[0]: c for c in LV.SOFT_CASES}
FOUR_OPS = [("volume", -1.3), ("volume", 0.9), ("clip", True, 20.0, True), ("volume", 1.1)]  # tests/test_gpu_level.py::EXACT_PROGRAMS[-1]


def test_level_in_place_and_out_of_place_behind_every_mark(bufs):
    lens = [257, 70001, 4099, 12289, 12289, 70001, 70001]
    p = LB.place(lens)
    LB.check(p)
    soft_long, soft_short = _SOFT["soft_n70001_g3_r"], _SOFT["soft_n4099_g0_n"]
    # (source placement, destination placement, samples, program, soft-clip case or None)
    items = [(0, 0, LV.signal(700, lens[0], 0.5), [("volume", 0.37)], None),
             (1, 6, LV.signal(soft_long[1], soft_long[2], soft_long[3]), soft_long[4], soft_long[0]),   # astride 2^29 -> behind 2^31
             (2, 2, LV.signal(soft_short[1], soft_short[2], soft_short[3]), soft_short[4], soft_short[0]),  # in place behind 2^29
             (3, 4, LV.signal(703, lens[3], 0.5), FOUR_OPS, None),                                      # astride 2^30 -> behind 2^30
             (5, 5, LV.signal(705, lens[5], 0.5), FOUR_OPS, None)]                                      # in place astride 2^31
    assert all(len(x) == lens[s] == lens[d] for s, d, x, _, _ in items)

    def run(arena, offs):
        so, do = [offs[s] for s, _, _, _, _ in items], [offs[d] for _, d, _, _, _ in items]
        _put(arena, so, [x for _, _, x, _, _ in items])
        got = A.level_in_arena(arena, so, [len(x) for _, _, x, _, _ in items], [prog for _, _, _, prog, _ in items], do)
        torch.cuda.synchronize()
        assert got.tolist() == do
        windows = sorted(set(so + do))
        _outside_is_untouched(arena, windows, [lens[offs.index(o)] for o in windows])
        for (s, d, x, _, _), o in zip(items, so):  # the source of an out-of-place item is only read
            if s != d:
                assert np.array_equal(arena[o : o + len(x)].cpu().numpy(), x)
        return _get(arena, do, [len(x) for _, _, x, _, _ in items])

    near = run(torch.full((p.near_size,), FILL, device="cuda"), p.near)
    for (_, _, x, prog, soft), y in zip(items, near):
        y = y.cpu().numpy()
        if soft is None:  # SCALE and hard CLIP: the model, bit for bit (tests/test_gpu_level.py)
            assert np.array_equal(y, LV.model32(x, prog)), prog
        else:  # soft CLIP: the recorded figures of the reference
            truth = LV.exact(x, prog)
            got_max, got_rel = LV.distances(y, truth)
            bar_max, bar_rel = LV.soft_bars(_SOFT_FIGURES[soft]["ref_max_abs"], _SOFT_FIGURES[soft]["ref_rel_l2"], truth)
            assert got_max <= bar_max and got_rel <= bar_rel, (soft, got_max, bar_max, got_rel, bar_rel)
    wave = bufs.filled_wave()
    try:
        far = run(wave, p.far)
    finally:
        _clear(wave, p.far, lens)
    for i, (a, b) in enumerate(zip(far, near)):
        assert torch.equal(a, b), (i, items[i][3])
    _report("hipfeat_level_run (peaks + ops)", read_to=p.far[5] + lens[5] - 1, wrote_to=p.far[6] + lens[6] - 1)


# ---- flat sizes past 2^31 -----------------------------------------------------------------------------------------------------------
def _tile(dst, period):
    """dst (1-D) <- the 1-D tensor `period` repeated, the last repetition cut; in pieces of under 2^28 elements"""
    n, k = dst.numel(), period.numel()
    per = max(1, (CHUNK // k)) * k
    for a in range(0, n, per):
        piece = dst[a : min(a + per, n)]
        whole = piece.numel() // k
        if whole:
            piece[: whole * k].view(whole, k).copy_(period[None, :].expand(whole, k))
        if piece.numel() % k:
            piece[whole * k :].copy_(period[: piece.numel() - whole * k])


def _is_periodic(t, first):
    """Every block of first.numel() elements of the 1-D tensor `t` equals `first` bit for bit (the incomplete last one its prefix)."""
    n, k = t.numel(), first.numel()
    per = max(1, (CHUNK // k)) * k
    ok = True
    for a in range(0, n, per):
        piece = t[a : min(a + per, n)]
        whole = piece.numel() // k
        if whole:
            ok = ok and bool((piece[: whole * k].view(whole, k) == first[None, :]).all())
        if piece.numel() % k:
            ok = ok and bool((piece[whole * k :] == first[: piece.numel() - whole * k]).all())
    return ok


@pytest.mark.parametrize("inverse", [0, 1], ids=["forward", "inverse"])
def test_global_mvn_past_2_31_elements(bufs, inverse):
    z = np.load(os.path.join(GOLDEN, "specaug.npz"))
    means, stds = z["mvn_means"].astype(np.float32), z["mvn_stds"].astype(np.float32)
    F, block_rows = 80, 4096
    rows = -(-2 ** 31 // F) + 1001
    n = rows * F
    assert 2 ** 31 < n <= LB.BUFFER_ELEMS
    block = (np.random.RandomState(80).randn(block_rows, F) * 3 - 8).astype(np.float32)
    want = (block * stds + means) if inverse else ((block - means) / stds)  # numpy's two float32 operations
    assert want.dtype == np.float32
    src, dst = bufs.wave[:n], bufs.nan_out()[:n]
    bufs.wave_is_filled = False
    _tile(src, torch.from_numpy(block.reshape(-1)).cuda())
    d_means, d_stds = torch.from_numpy(means).cuda(), torch.from_numpy(stds).cuda()
    _lib.load().check("hipfeat_global_mvn", src.data_ptr(), dst.data_ptr(), d_means.data_ptr(), d_stds.data_ptr(), rows, F, inverse, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    first = dst[: block_rows * F]
    assert np.array_equal(first.cpu().numpy().reshape(block_rows, F), want)
    assert _is_periodic(dst, first)
    assert _not_nan(bufs.out) == n  # nothing behind the last row
    _report(f"hipfeat_global_mvn inverse={inverse}", read_to=n - 1, wrote_to=n - 1)


def _half_specials():
    """The special values of tests/test_gpu_host_pipeline.py::test_float_to_half_on_the_device_and_the_half_pipeline (ties, subnormals,
    overflow to inf) padded with its noise to 2^16 values."""
    special = np.concatenate([np.float32([0.0, -0.0, 65504.0, 65520.0, 1e-8, 6e-5, -23.025851, 1e9, -1e9]), (np.arange(4096, dtype=np.float32) + 0.5) / 1024.0])
    rest = np.random.RandomState(0).randn(65536 - len(special)).astype(np.float32) * 10
    return np.concatenate([rest, special]).astype(np.float32)


def test_float_to_half_past_2_31_elements(bufs):
    n = 2 ** 31 + 12345
    vals = _half_specials()
    with np.errstate(over="ignore"):
        want = vals.astype(np.float16).view(np.int16)
    src = bufs.wave[:n]
    bufs.wave_is_filled = False
    _tile(src, torch.from_numpy(vals).cuda())
    out16 = bufs.out.view(torch.int16)
    out16[: n + 4096].fill_(0x7E00)  # a half NaN as the poison, also behind the end
    dst = out16[:n]
    _lib.load().check("hipfeat_float_to_half", src.data_ptr(), dst.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    first = dst[:65536]
    assert np.array_equal(first.cpu().numpy(), want)
    assert _is_periodic(dst, first)
    assert bool((out16[n : n + 4096] == 0x7E00).all())  # nothing behind the end
    _report("hipfeat_float_to_half", read_to=n - 1, wrote_to=n - 1)


def test_pcm16_to_float_past_2_31_elements(bufs):
    n = 2 ** 31 + 12345
    allv = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).cuda()
    pcm = bufs.wave.view(torch.int16)[:n]
    bufs.wave_is_filled = False
    _tile(pcm, allv)
    out = bufs.nan_out()
    dst = out[:n]
    _lib.load().check("hipfeat_pcm16_to_float", pcm.data_ptr(), dst.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    first = dst[:65536]
    assert torch.equal(first, allv.float() / 32768.0)
    assert _is_periodic(dst, first)
    assert _not_nan(out) == n
    _report("hipfeat_pcm16_to_float", read_to=n - 1, wrote_to=n - 1)


@pytest.mark.parametrize("B,T,F", [(103, 262144, 80), (102, 260000, 81)], ids=["F80-float4", "F81-scalar"])
def test_specaug_past_2_31_elements(bufs, B, T, F):
    """Every sequence holds the same (T, F) block and the same descriptors: one warp segment of 5000 rows across a tile boundary, two time
    masks (one touching row T - 1), two frequency masks.  > 2560 tiles per sequence: the mask kernel's partial-sum loop takes a second trip."""
    n = B * T * F
    assert 2 ** 31 < n <= LB.BUFFER_ELEMS
    rows_per_tile = 8192 // F
    tiles = -(-T // rows_per_tile)
    assert tiles > 2560  # (kernel_specaug.hpp: `for (i = threadIdx.x; i < tiles; i += 256)` with partial sums of 256 x 10 tiles and more)
    start = 40 * rows_per_tile - 2500  # rows [start, start + 5000) cross tile boundaries
    block = (np.random.RandomState(F).randn(T, F) * 3 - 8).astype(np.float32)
    segs = np.array([(b, start, 5000, 2400, 2650) for b in range(B)], dtype=_lib.WARP_SEGMENT_DTYPE)
    per_seq = [(1, 1000, 1037), (1, T - 30, T), (2, 5, 17), (2, F - 9, F)]
    masks = np.array([(b,) + m for b in range(B) for m in per_seq], dtype=_lib.MASK_DTYPE)
    want = specaug_ref.apply(block[None], [segs[:1]], masks[: len(per_seq)])[0]
    src, dst = bufs.wave[:n].view(B, T, F), bufs.nan_out()[:n].view(B, T, F)
    bufs.wave_is_filled = False
    _tile(bufs.wave[:n], torch.from_numpy(block.reshape(-1)).cuda())
    lib = _lib.load()
    lib.check("hipfeat_specaug", src.data_ptr(), dst.data_ptr(), B, T, F, _lib.addr(segs), len(segs), _lib.addr(masks), len(masks), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = dst[0].cpu().numpy()
    assert np.abs(got - want).max() <= 2e-5, np.abs(got - want).max()  # the bar of tests/test_gpu_specaug.py
    assert not np.array_equal(got[start : start + 5000], block[start : start + 5000])  # (the segment was warped)
    bad = [b for b in range(1, B) if not torch.equal(dst[b], dst[0])]
    assert not bad, bad
    assert _not_nan(bufs.out) == n and _is_periodic(bufs.wave[:n], bufs.wave[: T * F])  # nothing behind the end; the input is only read
    _report(f"hipfeat_specaug F={F} (specaug_warp_kernel<{4 if F % 4 == 0 else 1}> + specaug_mask_kernel)", read_to=n - 1, wrote_to=n - 1)


# ---- guards: tables are built, nothing is launched, no large memory -------------------------------------------------------------------
def test_layouts_refuse_what_one_launch_cannot_index():
    ex = _extractor("fft512c-fbank80")
    plan, lib = ex.plan, ex.plan.lib
    h = np.zeros(1, dtype=np.uint64)

    def create(lens):
        lens = _lib.i64(lens)
        offs = np.zeros(len(lens), dtype=np.int64)  # aliased: nothing is read
        st = lib.raw("hipfeat_layout_create", plan.handle, len(lens), _lib.addr(offs), _lib.addr(lens), None, None, 80, None, _lib.addr(h))
        if st == 0:
            lib.check("hipfeat_layout_destroy", int(h[0]))
        return st, lib.last_error()

    # 700 cuts of INT32_MAX samples, one of them a hop shorter: a ragged batch is laid out by frame quads, 700 x 3 355 444 of them
    lens = np.full(700, INT32_MAX, dtype=np.int64)
    lens[-1] -= 160
    st, msg = create(lens)
    assert st == _lib.ERR_INVALID and "batch too large for one launch" in msg, (st, msg)
    # equal cuts are laid out by workgroups (two rounds of a wave's four frames at the least): 700 of them are a valid layout ...
    assert create(np.full(700, INT32_MAX, dtype=np.int64))[0] == 0
    # ... and the same guard stops a batch of more of them
    st, msg = create(np.full(700 * 4096, INT32_MAX, dtype=np.int64))
    assert st == _lib.ERR_INVALID and "batch too large for one launch" in msg, (st, msg)
    st, msg = create([2 ** 31])  # a cut of 2^31 samples
    assert st == _lib.ERR_INVALID and "out of range" in msg, (st, msg)
    assert create([INT32_MAX])[0] == 0  # ... and the largest cut there is
    offs, one = np.zeros(1, dtype=np.int64), np.array([2 ** 31], dtype=np.int64)
    x = torch.zeros(16, device="cuda")
    assert lib.raw("hipfeat_extract", plan.handle, x.data_ptr(), _lib.addr(offs), _lib.addr(one), None, 1, x.data_ptr(), None, 80, None) == _lib.ERR_INVALID


def test_plans_refuse_items_longer_than_half_of_int32_max():
    too_long = INT32_MAX // 2 + 1
    lib = _lib.load()
    x = torch.zeros(16, device="cuda")
    r = A.get_or_create_resampler(17600, 16000)
    offs, lens = np.zeros(1, dtype=np.int64), np.array([too_long], dtype=np.int64)
    assert lib.raw("hipfeat_resample", r.handle, x.data_ptr(), _lib.addr(offs), _lib.addr(lens), 1, x.data_ptr(), _lib.addr(offs), None) == _lib.ERR_INVALID
    assert "out of range" in lib.last_error()
    with pytest.raises(_lib.HipFeatError) as e:
        A.get_or_create_mixer("cuda").plan([0, 1], [0], [too_long], [0], tail_start=2 ** 40)
    assert e.value.status == _lib.ERR_INVALID and "out of range" in str(e.value)
    with pytest.raises(_lib.HipFeatError) as e:
        A.get_or_create_reverb("cuda").plan([0], [too_long], [2 ** 35], [300], [0], tail_start=2 ** 40)
    assert e.value.status == _lib.ERR_INVALID and "both must be" in str(e.value)
    with pytest.raises(_lib.HipFeatError) as e:
        A.get_or_create_level("cuda").plan([0], [too_long], [[("volume", 0.5)]])
    assert e.value.status == _lib.ERR_INVALID and "must be 1 ..." in str(e.value)
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0


def test_runs_refuse_an_arena_that_ends_before_their_items():
    """Plans whose items sit behind 2^31, run with arena_floats = 2^31 - 1: refused before anything is enqueued."""
    lib = _lib.load()
    x = torch.zeros(16, device="cuda")
    small, far = INT32_MAX, 2 ** 31 + 8
    mixer, reverb, level = A.HipMixer("cuda"), A.HipReverb("cuda"), A.HipLevel("cuda")  # private ones: a refused run leaves its plan outstanding
    ticket, _, _, info = mixer.plan([0, 1], [far], [1000], [0], tail_start=far + 1000)
    assert int(info[1]) > 2 ** 31
    assert lib.raw("hipfeat_mix_run", mixer.handle, ticket, x.data_ptr(), small, None) == _lib.ERR_INVALID and "arena holds" in lib.last_error()
    ticket, _, info = reverb.plan([far], [1000], [far + 1000], [300], [0], tail_start=far + 1300)
    assert int(info[1]) > 2 ** 31
    assert lib.raw("hipfeat_reverb_run", reverb.handle, ticket, x.data_ptr(), small, None) == _lib.ERR_INVALID and "arena holds" in lib.last_error()
    ticket, info = level.plan([far], [1000], [[("clip", True, 0.0, True)]])
    assert int(info[1]) == far + 1000
    assert lib.raw("hipfeat_level_run", level.handle, ticket, x.data_ptr(), small, None) == _lib.ERR_INVALID and "arena holds" in lib.last_error()
    ex = _extractor("fft512c-fbank80")
    bank = A.HipSpeedBank([0.9], 16000, "cuda")
    offs, lens, idx = np.array([far], dtype=np.int64), np.array([16000], dtype=np.int64), np.array([0], dtype=np.int32)
    res, info = np.empty((3, 1), dtype=np.int64), np.zeros(4, dtype=np.int64)
    lib.check("hipfeat_minibatch_plan", bank.handle, ex.plan.handle, 1, _lib.addr(offs), _lib.addr(lens), _lib.addr(idx), None, far + 16000, 0, 0, None,
              _lib.addr(res[0]), _lib.addr(res[1]), _lib.addr(res[2]), None, _lib.addr(info))
    assert int(info[1]) > 2 ** 31 and int(res[0, 0]) >= far + 16000
    assert lib.raw("hipfeat_minibatch_run", bank.handle, int(info[0]), x.data_ptr(), small, x.data_ptr(), int(info[2]), LOG_EPSILON, None) == _lib.ERR_INVALID
    assert "arena holds" in lib.last_error()
    for obj in (bank, mixer, reverb, level):
        obj.close()
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0  # nothing ran
