"""GPU: the seeded sweep of tests/_grad_sweep.py through ``differentiable_()`` -- the waveform gradient of csrc/kernel_grad.hpp over the
option surface (frame geometry with N == fft, odd N and shift == N, every window, the energy floors, both mel scales, 64 / 65 / 128
filters, empty filters, a partly floored mel row, no lifter, odd pad lengths), one case per index of the kept list.

Each case is one forward and backward on a (3, S) batch of 6 to 9 frames, held with ``_grad_ref.hold`` -- per row E(device) <= max(2 E(g32),
1e-6) against the float64 autograd of the restatement -- and the differentiable forward's outputs are the plain layer's bits.
tests/test_grad_sweep_reference.py (CPU) holds the kept list to the conditions under which that bar means something.
"""
import warnings

import pytest
import torch

import _grad_ref as GR
import _grad_sweep as SW
import lhotse_amd as LA
from test_gpu_grad import poison

pytestmark = pytest.mark.gpu

WORST = {}  # class -> the worst E(device) / E(g32) of its cases so far, printed with every case


@pytest.mark.parametrize("i", SW.KEPT)
def test_sweep_case(i):
    ref = SW.reference(i)
    cls, kw, x = ref["cls"], ref["kw"], ref["x"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = getattr(LA, "Hip" + cls)(**kw)
    layer = GR.hip_layer(cls, kw)
    poison(x.shape)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    outs = GR.outputs(layer(xt))
    want = GR.outputs(plain(xt.detach()))
    assert len(outs) == len(want) == len(ref["cots"])
    for a, b in zip(outs, want):
        assert a.requires_grad and torch.equal(a.detach(), b)
    torch.autograd.backward(list(outs), [torch.from_numpy(c).cuda() for c in ref["cots"]])
    g = xt.grad.cpu().numpy()
    label = f"sweep {i} {cls} {GR.sizes(kw, cls)}"
    worst = GR.hold(label, g, ref["g32"], ref["g64"])
    WORST[cls] = max(WORST.get(cls, 0.0), worst)
    print(f"[grad-sweep] {label}: worst E(device) / E(g32) where the reference's error sets the bar: {worst:.3g}; {cls} so far {WORST[cls]:.3g}")
