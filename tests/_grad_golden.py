"""Writes tests/golden/grad.npz: what the LIVE six layers' autograd returned for ``_grad_ref.CASES`` (authoring container only: needs the
real lhotse).

    python tests/_grad_golden.py

Per case ``<name>/x`` is the (3, S) float32 input, ``<name>/cot0`` (and ``<name>/cot1`` for the log-energies of ``Wav2Win``) the cotangent
of each differentiable output, ``<name>/g32`` the gradient of sum <out, cot> with respect to ``x`` from the float32 layer and ``<name>/g64``
the same from ``layer.to(torch.float64)`` on the same float32 samples.  For the linear cases ``<name>/gap32`` is the relative gap between
<forward(x), cot> and <x, g32>, both accumulated in float64, of the float32 layer.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import _grad_ref as GR  # noqa: E402


def live_gradient(L, name, x, cots, dtype):
    """(gradient, the cotangents used, <out, cot> in float64): ``cots`` None draws them for the outputs' shapes."""
    cls, kw = GR.CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        layer = getattr(L, cls)(**kw).to(dtype)
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    outs = GR.outputs(layer(xt))
    if cots is None:
        cots = GR.case_cotangents(name, [tuple(o.shape) for o in outs])
    GR.pairing(outs, cots, dtype).backward()
    pair = float(GR.pairing([o.detach() for o in outs], cots, torch.float64))
    return xt.grad.numpy(), cots, pair


def main() -> None:
    from _dropin_support import import_lhotse

    import_lhotse()
    import lhotse.features.kaldi.layers as L

    arrays = {}
    for name in sorted(GR.CASES):
        x = GR.case_input(name)
        g32, cots, pair = live_gradient(L, name, x, None, torch.float32)
        g64, _, _ = live_gradient(L, name, x, cots, torch.float64)
        arrays[f"{name}/x"] = x
        for i, c in enumerate(cots):
            arrays[f"{name}/cot{i}"] = c
        arrays[f"{name}/g32"], arrays[f"{name}/g64"] = g32, g64
        if name in GR.LINEAR:
            back = float((x.astype(np.float64) * g32.astype(np.float64)).sum())
            arrays[f"{name}/gap32"] = np.float64(abs(pair - back) / abs(pair))
        e = GR.row_error(g32, g64)
        print(f"{name}: S {x.shape[1]}  E(g32) per row {np.array2string(e, precision=3)}  zero rows {[b for b in range(3) if not g64[b].any()]}")
    np.savez_compressed(GR.GOLDEN, **arrays)
    print(GR.GOLDEN, os.path.getsize(GR.GOLDEN), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
