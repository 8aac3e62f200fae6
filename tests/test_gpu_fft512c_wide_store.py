"""GPU: the 16-byte feature store of fft512c_kernel (transposed filterbank accumulators: lane = 4 slot + frame, register = filter, one
global_store_dwordx4 per lane and accumulator set) next to the one-dword-per-frame epilogue it replaces for filter counts that are a
multiple of 4.  Both routes multiply and add the same floats in the same order, so every comparison between them is ``array_equal``.
The plan's route is chosen at creation: HIPFEAT_NO_WIDE_STORE (routing switch) keeps the dword epilogue, and the wide route says
``store=16B`` in ``kernel_name``.

  frame counts    1, 2, 3, 4, 5, 31, 32, 33, 65, 600: one, two and three live frames in a cut's last round, cuts of one round, several
                  workgroups; once as one ragged batch (the frame-quad instance, where the geometry has one) and once as a uniform batch
                  of 33-frame cuts (workgroups per cut)
  filter counts   80 (two accumulator sets), 40 (one set), 23 (not a multiple of 4: the switch changes nothing, and nothing may differ)
  frame lengths   20 ms, 25 ms, 32 ms (10 / 13 / 16 input rows).  A 32 ms frame takes fft512c with the 5 ms shift only (LDS budget), and
                  needs more reflected samples than a cut of one or two frames has, so its batches run under the zero-padding edge rule
  guards          padded rows through the C ABI (row stride M, M + 1, M + 3, M + 4) over a sentinel: the columns from M on and the rows
                  past a cut's last frame keep the sentinel's bits; a row stride beyond the wide store's 32-bit lane offset
  collation       the fill rows of the collated batch are LOG_EPSILON bit for bit
  oracle          one 80-filter batch under the bar of tests/test_gpu_parity.py
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from _golden import ref32
from _hip import make_hip
from lhotse_amd import _lib
from lhotse_amd.compat import LOG_EPSILON
from oracle.kaldi_ref import RefConfig, RefExtractor

pytestmark = pytest.mark.gpu

FRAME_COUNTS = [1, 2, 3, 4, 5, 31, 32, 33, 65, 600]
GEOMETRIES = {"20ms": (0.020, 0.01, 10), "25ms": (0.025, 0.01, 13), "32ms": (0.032, 0.005, 16)}  # frame length, shift, input rows
SENTINEL = 0x7FC0BEEF  # a quiet NaN no kernel produces
WIDE_MAX_STRIDE = 1 << 22  # kMel4WideMaxStride


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        os.environ.pop(name, None) if old is None else os.environ.__setitem__(name, old)


def _pair(cfg, rows=13, **extra):
    """(default route, HIPFEAT_NO_WIDE_STORE route) of one configuration, both fft512c"""
    wide = make_hip("fbank", cfg, **extra)
    name_w = wide.kernel_name
    with _env("HIPFEAT_NO_WIDE_STORE", "1"):
        dword = make_hip("fbank", cfg, **extra)
        name_d = dword.kernel_name  # (plans are created lazily: touch it while the switch is set)
    M = cfg.get("num_filters", 80)
    for n in (name_w, name_d):
        assert n.startswith("fft512c_kernel<%d> fbank" % rows), n
    assert ("store=16B" in name_w) == (M % 4 == 0) and "store=16B" not in name_d, (name_w, name_d)
    return wide, dword


def _waves(seed, frame_counts, shift):
    rs = np.random.RandomState(seed)
    return [(rs.rand(k * shift).astype(np.float32) - 0.5) for k in frame_counts]


@pytest.mark.parametrize("M", [80, 40, 23])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_wide_route_equals_the_dword_route(geometry, M):
    frame_length, frame_shift, rows = GEOMETRIES[geometry]
    cfg = dict(frame_length=frame_length, frame_shift=frame_shift, num_filters=M)
    rule = "batch_zero_pad" if geometry == "32ms" else "reflect"
    wide, dword = _pair(cfg, rows, edge_rule=rule)
    shift = int(round(16000 * frame_shift))
    ragged = _waves(5, FRAME_COUNTS, shift)
    uniform = _waves(6, [33] * 9, shift)
    for what, items in (("ragged", ragged), ("uniform", uniform)):
        a, b = wide.extract_batch(items, 16000), dword.extract_batch(items, 16000)
        assert len(a) == len(b) == len(items)
        for w, fa, fb in zip(items, a, b):
            ctx = (geometry, M, what, len(w) // shift)
            assert fa.shape == fb.shape == (len(w) // shift, M), (ctx, fa.shape, fb.shape)
            assert np.isfinite(fa).all(), ctx
            assert np.array_equal(fa, fb), (ctx, float(np.abs(fa - fb).max()))
    if rule == "reflect":  # a cut on its own: one cut per launch, workgroups per cut
        for w, fa in zip(ragged, wide.extract_batch(ragged, 16000)):
            assert np.array_equal(wide.extract(w, 16000), fa), (geometry, M, len(w) // shift)


def _padded_run(plan, waves, stride, gap):
    """hipfeat_extract into rows of `stride` floats over a sentinel, `gap` untouched rows after every cut -> (int32 view of the buffer, first rows, frames)"""
    lens = np.array([len(w) for w in waves], dtype=np.int64)
    frames = [int(t) for t in plan.frame_counts(lens, None)]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    rows, r = [], 0
    for t in frames:
        rows.append(r)
        r += t + gap
    wave = torch.from_numpy(np.concatenate(waves)).cuda()
    out = torch.full((r * stride,), SENTINEL, dtype=torch.int32, device="cuda")
    plan.lib.check("hipfeat_extract", plan.handle, wave.data_ptr(), _lib.addr(_lib.i64(offs)), _lib.addr(_lib.i64(lens)), None, len(lens), out.data_ptr(),
                   _lib.addr(_lib.i64(rows)), int(stride), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.view(r, stride), rows, frames


def _check_guards(plan, waves, stride, dense, ctx):
    M = plan.feature_dim
    out, rows, frames = _padded_run(plan, waves, stride, gap=2)
    touched = torch.zeros(out.shape, dtype=torch.bool, device="cuda")
    for r, t, want in zip(rows, frames, dense):
        touched[r : r + t, :M] = True
        got = out[r : r + t, :M].contiguous().view(torch.float32).cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (ctx, stride, t)
    assert bool((out[~touched] == SENTINEL).all()), (ctx, stride, "a guard column or a row past a cut's end was written")
    assert bool((out[touched] != SENTINEL).all()), (ctx, stride)


@pytest.mark.parametrize("shape", ["ragged", "uniform"])
@pytest.mark.parametrize("M", [80, 40])
def test_padded_rows_keep_their_guards(M, shape):
    wide, dword = _pair(dict(num_filters=M))
    waves = _waves(7, FRAME_COUNTS[:-1] if shape == "ragged" else [33] * 5, 160)
    dense = [np.ascontiguousarray(y) for y in dword.extract_batch(waves, 16000)]
    for stride in (M, M + 1, M + 3, M + 4):
        _check_guards(wide.plan, waves, stride, dense, ("wide", M, shape))
    _check_guards(dword.plan, waves, M + 3, dense, ("dword", M, shape))


def test_row_stride_beyond_the_32_bit_lane_offset():
    """From kMel4WideMaxStride floats per row on the plan launches its dword-store twin: the same bits, the same guards."""
    wide, dword = _pair({})
    waves = _waves(8, [5, 3], 160)
    dense = [np.ascontiguousarray(y) for y in dword.extract_batch(waves, 16000)]
    _check_guards(wide.plan, waves, WIDE_MAX_STRIDE - 1, dense, ("wide", "last stride of the 16-byte store"))
    _check_guards(wide.plan, waves, WIDE_MAX_STRIDE, dense, ("wide", "first stride of the twin"))


@pytest.mark.parametrize("M", [80, 40])
def test_collated_fill_rows_are_log_epsilon(M):
    wide, dword = _pair(dict(num_filters=M))
    waves = _waves(9, [3, 65, 1, 34, 600, 2], 160)
    a, la = wide.extract_collated(waves, 16000)
    b, lb = dword.extract_collated(waves, 16000)
    assert la.tolist() == lb.tolist() == [3, 65, 1, 34, 600, 2] and a.shape == b.shape == (6, 600, M)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    eps_bits = int(np.float32(LOG_EPSILON).view(np.int32))
    single = wide.extract_batch(waves, 16000)
    for i, t in enumerate(la.tolist()):
        assert bool((a[i, t:].view(torch.int32) == eps_bits).all()), (M, i)
        assert np.array_equal(a[i, :t].cpu().numpy(), single[i]), (M, i)


def test_wide_route_meets_the_parity_bar():
    from test_gpu_parity import assert_parity

    wide, _ = _pair({})
    waves = _waves(10, FRAME_COUNTS, 160)
    rc = RefConfig(kind="fbank")
    o32, o64 = ref32(rc), RefExtractor(rc, np.float64)
    for w, got in zip(waves, wide.extract_batch(waves, 16000)):
        want, truth = o32.extract(w), o64.extract(w)
        assert got.shape == want.shape
        assert_parity(got, want, truth, ("wide_store", len(w)), suite="wide_store", kernel=wide.kernel_name, kind="fbank")
