"""GPU: one ragged ``HipWav2FFT`` output of more than 2^31 floats, in the manner of tests/test_gpu_stft_large.py (the marks are float indices
of the OUTPUT).

Two rows at a 1 ms shift; the first is full (2.1 M frames of 514 floats), so the second row of the (2, Tmax, 257) output lies past float
2^31 -- and it is SHORT: 5000 frames of its own, then padding rows to the end of the tensor.  Its frames (the first, and the last with
the row's own right reflection at ``lengths[1]``) are held to ``ref32`` and the truth of the row alone with the bars of
tests/_stft_ref.py; every padding row behind them, the frame that holds float 2^31 included, is ``padding_value + 0j`` exactly; the
first row's frames around float 2^29 and 2^30 are those of the uniform test; the samples behind ``lengths[1]`` are NaN and never read."""
import numpy as np
import pytest
import torch

import _large_buffers as LB
import _stft_ref as R
import lhotse_amd as LA

pytestmark = pytest.mark.gpu
NEED_FREE = 12 << 30
T, SHIFT, N, FFT = 2_100_000, 16, 400, 512
WIDTH = FFT + 2
T1 = 5000


def test_a_ragged_spectrum_whose_short_second_row_lies_past_2_31_floats():
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"the large ragged test needs 12 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    cfg = R.config(16000, frame_shift=0.001)
    assert R.K.window_sizes(cfg) == (N, SHIFT, FFT)
    S, S1 = T * SHIFT + 3, T1 * SHIFT + 5
    assert R.K.num_frames(S, N, SHIFT, False) == T and R.K.num_frames(S1, N, SHIFT, False) == T1 and (T + T1) * WIDTH < LB.MARKS[2] < 2 * T * WIDTH
    gen = torch.Generator(device="cuda").manual_seed(37)
    x = 0.1 * torch.randn((2, S), device="cuda", generator=gen) + 0.05
    x[1, S1:] = float("nan")
    y, out_lens = LA.HipWav2FFT(frame_shift=0.001)(x, [S, S1], -1.5)
    assert tuple(y.shape) == (2, T, FFT // 2 + 1) and y.dtype == torch.complex64 and y.numel() * 2 > LB.MARKS[2] and out_lens.tolist() == [T, T1]
    yr = torch.view_as_real(y)
    # the padding rows of the second row: all of them past float 2^31 - (T1 rows), every one (-1.5, +0.0)
    pad = yr[1, T1:]
    assert (pad[..., 0] == -1.5).all() and (pad[..., 1].view(torch.int32) == 0).all()
    g = LB.MARKS[2] // WIDTH
    assert divmod(g, T)[0] == 1  # float 2^31 lies in the second row
    left = (N - SHIFT) // 2
    snip = R.config(16000, frame_shift=0.001, snip_edges=True)
    cases = []
    row1 = x[1, :S1].cpu().numpy()[None]
    # the second row against the row alone: its first frames (a prefix has the same left reflection) and its last (its own right reflection)
    cases.append(("row 1, first frames", 1, 0, 4, cfg, row1[:, : 40 * SHIFT], 0))
    m = T1 - 40
    suffix = row1[:, m * SHIFT:]
    assert R.K.num_frames(suffix.shape[1], N, SHIFT, False) == 40
    cases.append(("row 1, last frames", 1, T1 - 4, 4, cfg, suffix, 36))
    for mark in LB.MARKS[:2]:  # the first row's frames that hold float 2^29 and 2^30
        f = mark // WIDTH
        assert f < T
        lo = (f - 1) * SHIFT - left
        cases.append((f"float {mark}", 0, f - 1, 4, snip, x[0, lo: lo + 3 * SHIFT + N].cpu().numpy()[None], 0))
    for label, row, f0, count, c, xs, skip in cases:
        got = y[row, f0: f0 + count].cpu().numpy()[None]
        assert np.isfinite(got.view(np.float32)).all(), label
        _, _, r = R.ref32(xs, c)
        _, _, t = R.truth(xs, c)
        R.hold(f"large ragged: {label} (frames {f0} ...)", got, r[:, skip: skip + count], t[:, skip: skip + count], energy_bin=True)
    print(f"[far] hipfeat_stft_run_ragged: wrote up to float {2 * T * WIDTH - 1} (2^31 + {2 * T * WIDTH - 1 - 2 ** 31})")
