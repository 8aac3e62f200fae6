#!/usr/bin/env python3
"""
TEST INFRASTRUCTURE -- generates tests/golden/stft.npz: what the REFERENCE's own ``Wav2Win`` and ``Wav2FFT``
(lhotse/features/kaldi/layers.py:59-324) return for the handful of configurations of tests/_stft_ref.py::GOLDEN_CASES, 3-5 frames each.

Needs the real lhotse (authoring container only):

    python tools/make_golden_stft.py

Per case: ``<case>/x`` (B, S) float32 input; ``<case>/frames`` (B, T, pad_length) float32 and ``<case>/log_energy`` (B, T) float32 (when
the case wants energies) of ``Wav2Win(pad_length=..., return_log_energy=...)``; ``<case>/spectrum`` (B, T, fft / 2 + 1) complex64 of
``Wav2FFT(use_energy=...)``.  Data only.  Asserted here for every case: ``_stft_ref.ref32`` equals the live layers bit for bit.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import _stft_ref as R
    from oracle.make_golden import import_reference

    import_reference()
    from lhotse.features.kaldi.layers import Wav2FFT, Wav2Win

    arrays = {}
    for name in sorted(R.GOLDEN_CASES):
        cfg, pad, x = R.golden_case(name)
        kw = R.layer_kwargs(cfg)
        with warnings.catch_warnings(), torch.no_grad():
            warnings.simplefilter("ignore")
            frames, log_e = Wav2Win(pad_length=pad, return_log_energy=cfg.use_energy, **kw)(torch.from_numpy(x))
            spectrum = Wav2FFT(round_to_power_of_two=True, use_energy=cfg.use_energy, **kw)(torch.from_numpy(x))
        r_frames, r_log_e, _ = R.ref32(x, cfg, pad)
        _, _, r_spectrum = R.ref32(x, cfg)
        assert np.array_equal(frames.numpy(), r_frames) and np.array_equal(spectrum.numpy(), r_spectrum), name
        assert (log_e is None) == (r_log_e is None) and (log_e is None or np.array_equal(log_e.numpy(), r_log_e)), name
        arrays[f"{name}/x"] = x
        arrays[f"{name}/frames"] = frames.numpy()
        arrays[f"{name}/spectrum"] = spectrum.numpy()
        if log_e is not None:
            arrays[f"{name}/log_energy"] = log_e.numpy()
        print(f"{name}: x {x.shape} frames {tuple(frames.shape)} spectrum {tuple(spectrum.shape)} {spectrum.dtype}")
    path = os.path.join(ROOT, "tests", "golden", "stft.npz")
    np.savez_compressed(path, **arrays)
    print("stft.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
