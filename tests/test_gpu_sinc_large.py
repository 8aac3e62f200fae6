"""GPU: ``hipfeat_sinc_run`` on an arena of more than 2^31 floats -- one row whose INPUT lies behind element 2^31 and one whose OUTPUT
does (8000:4673, 16 000 samples each; offsets of odd alignment, as tests/_large_buffers.py places items behind a mark).  A 32-bit
truncation of either offset would read or write 2^31 elements lower: the outputs must be within 1e-5 of the float64 truth and equal, bit
for bit, to those of the same rows in a small arena, and the floats around the low windows must keep their fill."""
import numpy as np
import pytest
import torch

import _large_buffers as LB
import _sinc_ref as SR
from lhotse_amd import augmentation as A

pytestmark = pytest.mark.gpu
ABS_TOL = 1e-5
FILL = 777.0
RATES = (16000, 9346)
N = 16000


def test_rows_whose_input_or_output_lies_past_2_31_floats():
    mark = LB.MARKS[2]
    out_n = SR.resampled_length(N, *SR.geometry(*RATES)[:2])
    #            input              output
    far = [(mark + 1, 7), (40003, mark + 20002)]  # row 0 reads behind 2^31, row 1 writes behind 2^31
    near = [(40000 + 1, 7), (60003, 80002)]  # the same rows in a small arena, same offsets modulo 4
    assert all(a % 4 == c % 4 and b % 4 == d % 4 for (a, b), (c, d) in zip(far, near))
    assert far[0][0] > mark and far[1][1] > mark and far[1][1] + out_n <= LB.BUFFER_ELEMS
    rng = np.random.RandomState(3)
    xs = [torch.from_numpy(rng.rand(N).astype(np.float32) - np.float32(0.5)).cuda() for _ in range(2)]
    truth = [SR.resample(x.cpu().numpy(), *RATES) for x in xs]
    sinc = A.get_or_create_sinc()

    def run(arena, where):
        for (i, _), x in zip(where, xs):
            arena[i : i + N] = x
        ticket, planned, info = sinc.plan([i for i, _ in where], [N, N], [RATES, RATES], [o for _, o in where], arena.numel())
        assert planned.tolist() == [out_n, out_n] and info[1] == max(max(i + N, o + out_n) for i, o in where)
        sinc.run(ticket, arena)
        torch.cuda.synchronize()
        return [arena[o : o + out_n].cpu().numpy() for _, o in where]

    small = run(torch.full((100000,), FILL, device="cuda"), near)
    for y, want in zip(small, truth):
        assert np.abs(y - want).max() <= ABS_TOL
    arena = torch.empty(LB.BUFFER_ELEMS, dtype=torch.float32, device="cuda")
    arena[:200000] = FILL  # where a truncated offset would land: (mark + 1) - 2^31 = 1, (mark + 20002) - 2^31 = 20002
    big = run(arena, far)
    for y, s, want in zip(big, small, truth):
        assert np.abs(y - want).max() <= ABS_TOL and np.array_equal(y.view(np.uint32), s.view(np.uint32))
    low = arena[:200000].cpu().numpy()
    keep = np.ones(200000, dtype=bool)
    keep[7 : 7 + out_n] = False  # row 0's output
    keep[40003 : 40003 + N] = False  # row 1's input
    assert np.all(low[keep] == FILL), "a float outside the rows was written below 2^31"
    assert np.array_equal(low[40003 : 40003 + N], xs[1].cpu().numpy())
    del arena
