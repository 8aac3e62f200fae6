"""GPU: fft512c_kernel with the 16-byte exchange reads (rows of 36 dwords, eight ds_read_b128 per half) and with the filterbank
instances that run the schedule's own steps per accumulator set ({16, 12} for 80 and 72 filters, {16, 8} for 64) at the smallest shapes
that take every path of the round:

  cuts            1, 3, 4, 5, 32, 33 and 65 frames: a partly filled quad, one full round of all eight waves, a wave's second and third
                  round -- each cut on its own (workgroups per cut), all of them as one ragged batch (the frame-quad instance, where the
                  geometry has one) and as the rows of one zero-padded batch (the edge rule's per-lane loads)
  filter counts   80, 72, 64
  frame lengths   25 ms and 20 ms (13 and 10 input rows)
  store           the one-dword-per-frame twin (row stride >= 2^22 floats) on a 4-frame cut

Every output is held against the generic kernel (HIPFEAT_FORCE_GENERIC=1 in a fresh plan) under the bound the fft512c agreement tests
use (tests/test_gpu_fft512c_round.py: norm-wise, oracle/parity_bar.py::REL_L2_TOL), and bit for bit against the instance that walks all
16 steps of both sets (HIPFEAT_NO_FIXED_SCHEDULE, routing switch): a dropped step is fmaf(0, P, acc) with P finite and acc >= +0.
"""
import numpy as np
import pytest
import torch

from _hip import make_hip
from oracle import parity_bar
from test_gpu_fft512c_wide_store import SENTINEL, WIDE_MAX_STRIDE, _env, _padded_run

pytestmark = pytest.mark.gpu

FRAME_COUNTS = [1, 3, 4, 5, 32, 33, 65]
GEOMETRIES = {"25ms": (0.025, 13), "20ms": (0.020, 10)}
STEPS = {80: (16, 12), 72: (16, 12), 64: (16, 8)}
SHIFT = 160


def _waves(seed, frame_counts):
    rs = np.random.RandomState(seed)
    return [(rs.rand(k * SHIFT).astype(np.float32) - 0.5) for k in frame_counts]


def _plans(cfg, rows, M, rule):
    """(default route, all-16-steps route, generic kernel) of one configuration"""
    fast = make_hip("fbank", cfg, edge_rule=rule)
    with _env("HIPFEAT_NO_FIXED_SCHEDULE", "1"):
        full = make_hip("fbank", cfg, edge_rule=rule)
        name_full = full.kernel_name  # (plans are created lazily: touch it while the switch is set)
    with _env("HIPFEAT_FORCE_GENERIC", "1"):
        slow = make_hip("fbank", cfg, edge_rule=rule)
        assert "generic" in slow.kernel_name, slow.kernel_name
    for n in (fast.kernel_name, name_full):
        assert n.startswith("fft512c_kernel<%d> fbank" % rows) and "store=16B" in n and "mel4=2x%d" % sum(STEPS[M]) in n, n
    return fast, full, slow


def _agree(fa, fb, fg, ctx):
    assert fa.shape == fb.shape == fg.shape, (ctx, fa.shape, fg.shape)
    assert np.isfinite(fa).all(), ctx
    rel = np.linalg.norm(fa.astype(np.float64) - fg) / np.linalg.norm(fg.astype(np.float64))
    assert rel <= parity_bar.REL_L2_TOL, (ctx, rel)
    assert np.array_equal(fa, fb), (ctx, float(np.abs(fa - fb).max()))


@pytest.mark.parametrize("M", list(STEPS))
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_cuts_alone_and_in_a_ragged_batch(geometry, M):
    frame_length, rows = GEOMETRIES[geometry]
    fast, full, slow = _plans(dict(frame_length=frame_length, num_filters=M), rows, M, "reflect")
    waves = _waves(3, FRAME_COUNTS)
    a, b, g = (p.extract_batch(waves, 16000) for p in (fast, full, slow))  # one ragged batch
    assert len(a) == len(b) == len(g) == len(waves)
    for w, fa, fb, fg in zip(waves, a, b, g):
        ctx = (geometry, M, len(w) // SHIFT)
        assert fa.shape == (len(w) // SHIFT, M), ctx
        _agree(fa, fb, fg, ctx + ("ragged",))
        alone = fast.extract(w, 16000)  # a cut on its own: workgroups per cut
        _agree(alone, full.extract(w, 16000), fg, ctx + ("alone",))
        assert np.array_equal(alone, fa), ctx


@pytest.mark.parametrize("M", list(STEPS))
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_rows_of_a_padded_batch(geometry, M):
    frame_length, rows = GEOMETRIES[geometry]
    fast, full, slow = _plans(dict(frame_length=frame_length, num_filters=M), rows, M, "batch_zero_pad")
    waves = _waves(4, FRAME_COUNTS)
    lens = torch.tensor([len(w) for w in waves], dtype=torch.int32)
    padded = torch.zeros(len(waves), int(lens.max()))
    for i, w in enumerate(waves):
        padded[i, : len(w)] = torch.from_numpy(w)
    a, b, g = (list(p.extract_batch(padded, 16000, lengths=lens)) for p in (fast, full, slow))
    assert len(a) == len(b) == len(g) == len(waves)
    for w, fa, fb, fg in zip(waves, a, b, g):
        fa, fb, fg = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (fa, fb, fg))
        _agree(fa, fb, fg, (geometry, M, len(w) // SHIFT, "padded"))


@pytest.mark.parametrize("M", list(STEPS))
def test_dword_store_twin_on_a_four_frame_cut(M):
    """From kMel4WideMaxStride floats per row on the plan launches the dword-store twin, which walks all 16 steps: the same bits."""
    fast, full, slow = _plans(dict(num_filters=M), 13, M, "reflect")
    waves = _waves(5, [4])
    dense = fast.extract_batch(waves, 16000)
    _agree(dense[0], full.extract_batch(waves, 16000)[0], slow.extract_batch(waves, 16000)[0], (M, "dense"))
    for stride in (WIDE_MAX_STRIDE - 1, WIDE_MAX_STRIDE):
        out, first_rows, frames = _padded_run(fast.plan, waves, stride, gap=0)
        assert frames == [4] and first_rows == [0]
        got = out[:4, :M].contiguous().view(torch.float32).cpu().numpy()
        assert np.array_equal(got.view(np.int32), np.ascontiguousarray(dense[0]).view(np.int32)), (M, stride)
        assert bool((out[:4, M : M + 64] == SENTINEL).all()) and bool((out[:4, -64:] == SENTINEL).all()), (M, stride)
