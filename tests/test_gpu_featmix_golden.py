"""GPU: the feature-mix launches on every golden group (tests/golden/featmix.json + .npz: the byte arena and the table
``HipPrecomputedFeatures`` made, and what the REFERENCE returned for the same cuts).  Copy-form rows are bit-equal to the reference;
fold-form rows are within the bar -- per element ``|out - truth| <= max(2 x reference_max_abs, 2 x spacing(float32(|truth|)))``, truth =
the float64 statement of tests/_featmix_ref.py -- and the measured distance is printed next to the reference's.  The binary16 route
(the fixtures as stored) and the float32 route (the same values widened) give the same bits."""
import numpy as np
import pytest
import torch

import _featmix_ref as R

from lhotse_amd import augmentation as A

pytestmark = pytest.mark.gpu
GROUPS = ["right", "left", "both", "cutmix", "snr_first", "pad_value", "off_by_one", "truncated", "k2"]


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _run(arena, table, F, row_frames):
    host = np.concatenate([arena, np.zeros(-len(arena) % 16, dtype=np.uint8)])
    out, lens = A.featmix_in_arena(torch.from_numpy(host).cuda(), table, F, row_frames)
    torch.cuda.synchronize()
    return out.cpu().numpy(), lens


@pytest.mark.parametrize("name", GROUPS)
def test_every_golden_group_is_within_the_bar(golden, name):
    g = golden[name]
    got, lens = _run(g["arena"], g["table"], g["F"], g["row_frames"])
    assert lens.dtype == np.int32 and lens.tolist() == [c.num_frames for c in g["table"]]
    R.check_against_golden(g, got, name)
    wide, table = R.widened(g["arena"], g["table"], g["F"])
    again, _ = _run(wide, table, g["F"], g["row_frames"])
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), "the binary16 and the float32 route differ"
