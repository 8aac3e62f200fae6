"""GPU: one ``HipWav2FFT`` output of more than 2^31 floats (in the manner of tests/test_gpu_stats_large.py and tests/_large_buffers.py: the
marks are float indices of the OUTPUT).

Every element index of kernel_stft.hpp is 64-bit: (row T + frame) (fft + 2) passes 2^31 in the second row of this batch, and no other
test makes its upper dword non-zero.  A 1 ms shift keeps the input small (two rows of 33.6 M samples) while the output holds
2 x 2.1 M frames of 514 floats = 2^31 + 11.3 M floats (8.04 GiB).  The first frames of the first row, the frames around float 2^29, 2^30 and
2^31 and the last frames of the last row are held to ``ref32`` and the truth of the samples they cover (the bars of tests/_stft_ref.py)."""
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


def test_a_spectrum_of_more_than_2_31_floats():
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"the large STFT test needs 12 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    cfg = R.config(16000, frame_shift=0.001)
    assert R.K.window_sizes(cfg) == (N, SHIFT, FFT)
    S = T * SHIFT + 3
    assert R.K.num_frames(S, N, SHIFT, False) == T and 2 * T * WIDTH > LB.MARKS[2]
    gen = torch.Generator(device="cuda").manual_seed(31)
    x = 0.1 * torch.randn((2, S), device="cuda", generator=gen) + 0.05
    y = LA.HipWav2FFT(frame_shift=0.001)(x)
    assert tuple(y.shape) == (2, T, FFT // 2 + 1) and y.dtype == torch.complex64 and y.numel() * 2 > LB.MARKS[2]
    left = (N - SHIFT) // 2
    snip = R.config(16000, frame_shift=0.001, snip_edges=True)

    def interior(row, f0, count):  # frames f0 .. f0 + count - 1 of `row`, none of which touches an edge: the same samples with snip_edges
        lo = f0 * SHIFT - left
        assert lo >= 0 and lo + (count - 1) * SHIFT + N <= S
        return snip, x[row, lo: lo + (count - 1) * SHIFT + N].cpu().numpy()[None]

    cases = []
    # the first frames of the first row: a prefix has the same left reflection
    cases.append(("first frames", 0, 0, 4, cfg, x[0, : 40 * SHIFT].cpu().numpy()[None], 0))
    # the frames that hold float 2^29, 2^30 and 2^31 of the output
    for mark in LB.MARKS:
        g = mark // WIDTH
        row, f = divmod(g, T)
        assert g * WIDTH <= mark < (g + 1) * WIDTH and (mark < LB.MARKS[2] or row == 1)
        c, xs = interior(row, f - 1, 4)
        cases.append((f"float {mark}", row, f - 1, 4, c, xs, 0))
    # the last frames of the last row: a suffix that is shorter by whole shifts has the same right reflection
    m = T - 40
    suffix = x[1, m * SHIFT:].cpu().numpy()[None]
    assert R.K.num_frames(suffix.shape[1], N, SHIFT, False) == 40
    cases.append(("last frames", 1, T - 4, 4, cfg, suffix, 36))
    for label, row, f0, count, c, xs, skip in cases:
        got = y[row, f0: f0 + count].cpu().numpy()[None]
        _, _, r = R.ref32(xs, c)
        _, _, t = R.truth(xs, c)
        R.hold(f"large: {label} (row {row}, frames {f0} ...)", got, r[:, skip: skip + count], t[:, skip: skip + count], energy_bin=True)
    print(f"[far] hipfeat_stft_run: wrote up to float {2 * T * WIDTH - 1} (2^31 + {2 * T * WIDTH - 1 - 2 ** 31})")
