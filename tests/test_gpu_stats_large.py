"""GPU: the statistics launches over a feature buffer of more than 2^31 elements (in the manner of tests/test_gpu_featmix_large.py).

StCut::first_elem = first_row * row_stride is 64-bit; no other test makes its upper dword non-zero.  One binary16 buffer of 2^31 + 2^24
elements (4.03 GiB) holds two short cuts: one at its start, one whose first element lies behind element 2^31 (byte 2^32).  Each is held
to the reference statement on the same values (the bar of tests/test_gpu_stats.py) and is bit-equal to the same cut run from a small
buffer at the same alignment."""
import numpy as np
import pytest
import torch

import _large_buffers as LB
import _stats_ref as S

import lhotse_amd as LA
from test_gpu_stats import bits, hold_to_the_bar, reference_over, same_bits

pytestmark = pytest.mark.gpu
NEED_FREE = 6 << 30
F = 80


def test_a_cut_behind_element_2_31_of_a_binary16_buffer():
    free = torch.cuda.mem_get_info()[0]
    if free < NEED_FREE:
        pytest.skip(f"the large statistics test needs 6 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    rng = np.random.RandomState(5)
    frames = [300, 517]  # (more than one block each)
    mats = [(rng.standard_normal((n, F)) * 2.5 - 8.0).astype(np.float16) for n in frames]
    first_row = [3, 2 ** 31 // F + 5]
    assert first_row[1] * F > 2 ** 31 and (first_row[1] + frames[1]) * F <= LB.BUFFER_ELEMS
    big = torch.empty(LB.BUFFER_ELEMS, dtype=torch.float16, device="cuda")  # (rows outside the two cuts are never read)
    for r, m in zip(first_row, mats):
        big[r * F: (r + len(m)) * F] = torch.from_numpy(m.reshape(-1)).cuda()
    rows = big[: (LB.BUFFER_ELEMS // F) * F].view(-1, F)
    both = LA.HipStatsAccumulator(F)
    both.update(rows, frames, first_row=first_row)
    wide = [m.astype(np.float32) for m in mats]
    hold_to_the_bar("two cuts, one behind element 2^31", both, reference_over(F, wide), wide)
    for r, m, w in zip(first_row, mats, wide):
        far = LA.HipStatsAccumulator(F)
        far.update(rows, [len(m)], first_row=[r])
        hold_to_the_bar(f"the cut at row {r}", far, reference_over(F, [w]), [w])
        near = LA.HipStatsAccumulator(F)
        near.update(torch.from_numpy(m).cuda())
        assert same_bits(bits(far), bits(near)), r
    print(f"[far] hipfeat_stats_update: read up to element {(first_row[1] + frames[1]) * F - 1} (2^31 + {(first_row[1] + frames[1]) * F - 1 - 2 ** 31})")
