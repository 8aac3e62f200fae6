"""GPU: the FFT route of ``hipfeat_reverb_run`` on an arena of more than 2^31 floats -- one item whose source, impulse response, output
AND spectra workspace all lie behind element 2^31 (offsets of odd alignment, as tests/_large_buffers.py places items behind a mark).  A
32-bit truncation of any of the offsets would read or write 2^31 elements lower: the output must equal, bit for bit, that of the same
item planned at the front of a small arena (same offsets modulo 4), and the floats where a truncated offset would land keep their fill."""
import numpy as np
import pytest
import torch

import _large_buffers as LB
from lhotse_amd import augmentation as A

pytestmark = pytest.mark.gpu
FILL = 777.0
N, TAPS, SHIFT = 5000, 2049, 1025  # 3 partitions, 6 input blocks, 5 output blocks; a block's first output at 3 mod 4


def test_an_item_whose_source_output_and_workspace_lie_past_2_31_floats():
    mark = LB.MARKS[2]
    rng = np.random.RandomState(4)
    x = torch.from_numpy(rng.rand(N).astype(np.float32) - np.float32(0.5)).cuda()
    rir = (rng.rand(TAPS).astype(np.float32) - np.float32(0.5)) * np.exp(-np.arange(TAPS) / 300.0).astype(np.float32)
    rir[SHIFT] = 1.0
    hs, shift = A.scaled_rir(rir)
    assert shift == SHIFT
    hs = torch.from_numpy(hs).cuda()
    tail_floats = A.reverb_fft_tail_floats([N], [TAPS], [SHIFT])
    rv = A.get_or_create_reverb("cuda:0")

    def run(arena, src, rir_at, tail_start):
        arena[src : src + N] = x
        arena[rir_at : rir_at + TAPS] = hs
        ticket, offs, info = rv.plan([src], [N], [rir_at], [TAPS], [SHIFT], [1], tail_start, "fft")
        assert int(info[1]) == ((tail_start + 3) & ~3) + tail_floats - 3 and int(info[1]) <= arena.numel()
        assert int(info[4]) == 3 + 6 and int(info[5]) == 5 and int(info[7]) == 1
        rv.run(ticket, arena)
        torch.cuda.synchronize()
        return int(offs[0]), arena[int(offs[0]) : int(offs[0]) + N].cpu().numpy()

    far_src, far_rir = mark + 1, mark + 1 + N + 2  # both of odd alignment
    far_tail = far_rir + TAPS + 1
    near_src, near_rir = 40000 + 1, 40000 + 1 + N + 2
    near_tail = near_rir + TAPS + 1
    assert far_src % 4 == near_src % 4 and far_rir % 4 == near_rir % 4 and far_tail % 4 == near_tail % 4
    assert far_tail + tail_floats <= LB.BUFFER_ELEMS
    _, small = run(torch.full((near_tail + tail_floats + 8,), FILL, device="cuda"), near_src, near_rir, near_tail)
    assert np.isfinite(small).all() and np.abs(small).max() > 0
    arena = torch.empty(LB.BUFFER_ELEMS, dtype=torch.float32, device="cuda")
    low = far_tail + tail_floats - mark + 64  # where truncated offsets would land: everything above, 2^31 elements lower
    arena[:low] = FILL
    out_at, big = run(arena, far_src, far_rir, far_tail)
    assert out_at > mark
    assert np.array_equal(big.view(np.uint32), small.view(np.uint32))
    assert bool((arena[:low] == FILL).all()), "a float was written 2^31 elements below its place"
    assert bool((arena[far_src : far_src + N] == x).all()) and bool((arena[far_rir : far_rir + TAPS] == hs).all())
    del arena
