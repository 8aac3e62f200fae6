"""GPU: one ``HipWav2FFT.online_inference`` call whose output holds more than 2^31 floats and whose chunk starts more than 2^31 elements into
its tensor (in the manner of tests/test_gpu_stft_large.py: the marks are float indices of the OUTPUT).

Every element index of kernel_stream.hpp is 64-bit: (row T + frame) (fft + 2) passes 2^31 in the second row of this batch, and the chunk is a
view that begins behind float 2^31 of an (uninitialised) 8 GiB tensor, so a base pointer or an offset cut to 32 bits reads elsewhere.  A 1 ms
shift keeps the samples few (two rows of 33.6 M) while the output holds 2 x 2.1 M frames of 514 floats.  The first frames (inside the
caller-made context and across the seam), the frames around float 2^29, 2^30 and 2^31 and the last frames are held to ``ref32`` and the truth of
the samples of V they cover; the remainder is V[:, T s:] bit for bit."""
import pytest
import torch

import _large_buffers as LB
import _stft_ref as R
import _stream_ref as SR
import lhotse_amd as LA

pytestmark = pytest.mark.gpu
NEED_FREE = 22 << 30
T, SHIFT, N, FFT = 2_100_000, 16, 400, 512
WIDTH = FFT + 2
CONTEXT = 2 * N + 3


def test_a_streamed_spectrum_of_more_than_2_31_floats_from_a_chunk_behind_2_31_elements():
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"the large streaming test needs 22 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    cfg = R.config(16000, frame_shift=0.001)
    assert R.K.window_sizes(cfg) == (N, SHIFT, FFT)
    L = N + (T - 1) * SHIFT + 7
    S = L - CONTEXT
    assert SR.counts(L, N, SHIFT) == (T, N + 7 - SHIFT) and 2 * T * WIDTH > LB.MARKS[2]
    store = torch.empty(2 ** 31 + 5 + 2 * (S + 3), device="cuda")
    x = store[2 ** 31 + 5:].view(2, S + 3)[:, :S]  # rows with a stride of their own, the first one at an odd float offset past 2^31
    assert (x.data_ptr() - store.data_ptr()) // 4 > 2 ** 31 and x.data_ptr() % 8 == 4 and x.stride(0) == S + 3
    gen = torch.Generator(device="cuda").manual_seed(37)
    x.copy_(0.1 * torch.randn((2, S), device="cuda", generator=gen) + 0.05)
    context = 0.1 * torch.randn((2, CONTEXT), device="cuda", generator=gen) + 0.05
    y, remainder = LA.HipWav2FFT(frame_shift=0.001).online_inference(x, context)
    assert tuple(y.shape) == (2, T, FFT // 2 + 1) and y.dtype == torch.complex64 and y.numel() * 2 > LB.MARKS[2]
    assert tuple(remainder.shape) == (2, N + 7 - SHIFT) and torch.equal(remainder, x[:, S - (N + 7 - SHIFT):])

    def piece(row, f0, count):  # the samples of V that frames f0 .. f0 + count - 1 of `row` cover
        lo, hi = f0 * SHIFT, (f0 + count - 1) * SHIFT + N
        parts = [context[row, lo:min(hi, CONTEXT)]] if lo < CONTEXT else []
        if hi > CONTEXT:
            parts.append(x[row, max(lo - CONTEXT, 0): hi - CONTEXT])
        return torch.cat(parts).cpu().numpy()[None]

    cases = [("first frames (context)", 0, 0, 4), ("across the seam", 1, (CONTEXT - N) // SHIFT, 4 + N // SHIFT), ("last frames", 1, T - 4, 4)]
    for mark in LB.MARKS:
        g = mark // WIDTH
        row, f = divmod(g, T)
        assert g * WIDTH <= mark < (g + 1) * WIDTH and (mark < LB.MARKS[2] or row == 1)
        cases.append((f"float {mark}", row, f - 1, 4))
    for label, row, f0, count in cases:
        xs = piece(row, f0, count)
        assert xs.shape[1] == (count - 1) * SHIFT + N
        got = y[row, f0: f0 + count].cpu().numpy()[None]
        R.hold(f"large stream: {label} (row {row}, frames {f0} ...)", got, SR.ref32(xs, cfg)[2], SR.truth(xs, cfg)[2], energy_bin=True)
    print(f"[far] hipfeat_stream_run: wrote up to float {2 * T * WIDTH - 1} (2^31 + {2 * T * WIDTH - 1 - 2 ** 31}), chunk at float {(x.data_ptr() - store.data_ptr()) // 4}")
