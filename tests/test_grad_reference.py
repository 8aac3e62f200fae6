"""CPU, against tests/golden/grad.npz (the live reference's autograd; written by tests/_grad_golden.py in the authoring container): the
restatement ``_grad_ref.forward`` reproduces the reference's gradients in float32 and in float64.

It gathers the frames through an index map and builds bin 0 / column 0 with ``cat`` where the reference strides, flips, concatenates and
assigns in place, so its sums run in the reference's order only where torch happens to pick the same kernels: the gradient is held to
4 ulp of max |g| of its dtype per row (float32: 4.8e-7 max |g|; float64: 8.9e-16 max |g|) and is bit for bit in most cases.
"""
import numpy as np
import pytest
import torch

import _grad_ref as GR

pytestmark = pytest.mark.reference


@pytest.fixture(scope="module")
def gold():
    return GR.load_golden()


def test_the_file_holds_every_case_and_stays_small(gold):
    import os

    assert os.path.getsize(GR.GOLDEN) < 1_000_000 and len(GR.CASES) == 24
    assert {GR.CASES[n][0] for n in GR.CASES} == set(GR.CLASSES)
    for name in GR.CASES:
        x = gold[f"{name}/x"]
        assert np.array_equal(x, GR.case_input(name)) and x.shape[0] == 3 and not x[1].any() and np.abs(x).max() <= 0.75
        assert gold[f"{name}/g32"].dtype == np.float32 and gold[f"{name}/g64"].dtype == np.float64
        assert (f"{name}/gap32" in gold) == (name in GR.LINEAR)


@pytest.mark.parametrize("name", sorted(GR.CASES))
def test_the_restatement_reproduces_the_live_gradient(gold, name):
    cls, kw = GR.CASES[name]
    x, cots = gold[f"{name}/x"], GR.golden_cotangents(gold, name)
    for dtype, key, ulp in ((torch.float32, "g32", 2.0 ** -23), (torch.float64, "g64", 2.0 ** -52)):
        g, want = GR.gradient(cls, kw, x, cots, dtype), gold[f"{name}/{key}"]
        assert g.dtype == want.dtype
        off = np.abs(g.astype(np.float64) - want.astype(np.float64)).max(axis=1)
        scale = np.abs(want).max(axis=1)
        print(f"[grad-ref] {name} {key}: equal {np.array_equal(g, want)}  max |diff| / max |g| per row {off / np.where(scale > 0, scale, 1.0)} (ulp {ulp:.3g})")
        assert (off <= 4.0 * ulp * scale).all(), (name, key)
        assert not g[scale == 0].any()
