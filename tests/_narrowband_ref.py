"""TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

The statement of ``Narrowband(codec="mulaw", source_sampling_rate=sr, restore_orig_sr=r)`` (lhotse/augmentation/torchaudio.py:337-378) in
numpy float64 for one row taken alone: ``_sinc_ref.resample`` down to 8 kHz, the text of torchaudio's ``MuLawEncoding(256)`` /
``MuLawDecoding(256)`` (no clamp, the cast truncates toward zero), ``_sinc_ref.resample`` back up, cut to the row's length.  Needs
neither lhotse nor torchaudio.
"""
import numpy as np

import _sinc_ref as SR

MU = 255.0


def decode(codes):
    v = np.asarray(codes, dtype=np.float64) / MU * 2 - 1
    return np.sign(v) * (np.exp(np.abs(v) * np.log1p(MU)) - 1) / MU


def narrowband(x, sr: int, restore: bool, filters=None):
    """-> (result float64, u float64: the code values of the 8 kHz samples before truncation).  ``filters``: (window(sr, 8000),
    window(8000, sr)) computed before."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    down, up = filters if filters is not None else (None, None)
    d = x if sr == 8000 else SR.resample(x, sr, 8000, down)
    u = (np.sign(d) * np.log1p(MU * np.abs(d)) / np.log1p(MU) + 1) / 2 * MU + 0.5
    q = decode(np.trunc(u))
    if not restore or sr == 8000:
        return q, u
    z = SR.resample(q, 8000, sr, up)
    assert len(z) >= len(x)
    return z[: len(x)], u
