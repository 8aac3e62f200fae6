"""GPU: one waveform gradient whose workspace passes 2^31 floats (in the manner of tests/test_gpu_stft_large.py: the marks are float
indices of the WORKSPACE of csrc/kernel_grad.hpp, (rows, T, Nr) with Nr = 400).

Every element index of the two gradient kernels is 64-bit: (row T + frame) Nr passes 2^31 inside this one row, and no other test makes
its upper dword non-zero.  A 1 ms shift keeps the input small (86.4 M samples) while the workspace holds 5.4 M frames of 400 floats =
2^31 + 12.5 M floats (8.05 GiB); the budget cannot split a single row, so it is one piece.  The cotangent is non-zero only in four frames
around float 2^29, 2^30 and 2^31 of the workspace and in the first and last four frames; the gradient under those frames equals, bit for
bit, the gradient of the same frames computed on a short excerpt, and every other sample's gradient is exactly zero."""
import warnings

import pytest
import torch

import _large_buffers as LB
import lhotse_amd as LA

pytestmark = pytest.mark.gpu
NEED_FREE = 16 << 30
T, SHIFT, N, M = 5_400_000, 16, 400, 80
LEFT = (N - SHIFT) // 2
SPAN = 3 * SHIFT + N  # samples under four consecutive frames


def gradient(layer, x, cot):
    x = x.detach().requires_grad_(True)
    y = layer(x)
    assert y.shape == cot.shape
    y.backward(cot)
    return x.grad


def test_a_workspace_of_more_than_2_31_floats():
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"the large gradient test needs 16 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    S = T * SHIFT
    assert (S + SHIFT // 2) // SHIFT == T and T * N > LB.MARKS[2]
    gen = torch.Generator(device="cuda").manual_seed(33)
    x = torch.rand((1, S), device="cuda", generator=gen) - 0.5
    far = LA.HipWav2LogFilterBank(frame_shift=0.001).differentiable_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        snip = LA.HipWav2LogFilterBank(frame_shift=0.001, snip_edges=True).differentiable_()
    seeds = torch.randn((5, 4, M), device="cuda", generator=gen)
    firsts = [0] + [mark // N - 1 for mark in LB.MARKS] + [T - 4]  # the first of the four frames of every place
    assert all(f * N <= mark < (f + 4) * N for f, mark in zip(firsts[1:4], LB.MARKS))
    cot = torch.zeros((1, T, M), device="cuda")
    for f, seed in zip(firsts, seeds):
        cot[0, f: f + 4] = seed
    g = gradient(far, x, cot)
    del cot
    assert g.shape == (1, S) and torch.isfinite(g).all()
    rest = g.clone()
    # the first frames: a prefix has the same left reflection
    prefix = x[:, : 40 * SHIFT]
    c = torch.zeros((1, 40, M), device="cuda")
    c[0, :4] = seeds[0]
    hi = 3 * SHIFT - LEFT + N
    assert torch.equal(g[:, :hi], gradient(far, prefix, c)[:, :hi])
    rest[:, :hi] = 0
    # the frames that hold float 2^29, 2^30 and 2^31 of the workspace: the same samples with snip_edges
    for f, seed in zip(firsts[1:4], seeds[1:4]):
        lo = f * SHIFT - LEFT
        assert lo > 0 and lo + SPAN < S
        got = gradient(snip, x[:, lo: lo + SPAN], seed[None])
        assert got.any() and torch.equal(g[:, lo: lo + SPAN], got), f
        rest[:, lo: lo + SPAN] = 0
    # the last frames: a suffix that is shorter by whole shifts has the same right reflection
    suffix = x[:, (T - 40) * SHIFT:]
    c = torch.zeros((1, 40, M), device="cuda")
    c[0, 36:] = seeds[4]
    lo = 4 * SHIFT + LEFT  # samples from the first one under frame T - 4 on
    assert torch.equal(g[:, S - lo:], gradient(far, suffix, c)[:, -lo:])
    rest[:, S - lo:] = 0
    assert not rest.any()  # a zero cotangent leaves exactly zero
