"""CPU: tests/golden/stft.npz (written by tools/make_golden_stft.py from the LIVE ``Wav2Win`` / ``Wav2FFT``) holds the inputs the tests
regenerate from their seeds, outputs of the shapes the layers document, and values that the float64 truth and ``ref32`` on this machine
agree with.  ``ref32`` equals the live layers bit for bit where they run (tests/test_stft_reference.py); here, on any CPU, it is held to
the stored values to 1e-6 of a frame's norm, because torch's FFT and reductions may take another instruction path on another CPU."""
import os

import numpy as np
import pytest

import _stft_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stft.npz")


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_the_goldens_are_the_cases_and_agree_with_both_statements(name):
    arrays = np.load(GOLDEN)
    cfg, pad, x = R.golden_case(name)
    n, shift, fft = R.K.window_sizes(cfg)
    B, T = R.GOLDEN_CASES[name][3]
    assert 3 <= T <= 5 and np.array_equal(arrays[f"{name}/x"], x) and x.dtype == np.float32
    frames, spectrum = arrays[f"{name}/frames"], arrays[f"{name}/spectrum"]
    assert frames.shape == (B, T, pad) and frames.dtype == np.float32
    assert spectrum.shape == (B, T, fft // 2 + 1) and spectrum.dtype == np.complex64
    r_frames, r_log_e, _ = R.ref32(x, cfg, pad)
    _, _, r_spectrum = R.ref32(x, cfg)
    t_frames, t_log_e, _ = R.truth(x, cfg, pad)
    _, _, t_spectrum = R.truth(x, cfg)
    assert R.frame_error(r_frames, frames) <= 1e-6 and R.frame_error(r_spectrum, spectrum) <= 1e-6
    # the stored values against the truth: bar 1 of the GPU tests (hold with y = r = the golden)
    R.hold(f"golden {name} frames", frames, frames, t_frames)
    R.hold(f"golden {name} spectrum", spectrum, spectrum, t_spectrum, energy_bin=cfg.use_energy)
    if cfg.use_energy:
        log_e = arrays[f"{name}/log_energy"]
        assert log_e.shape == (B, T) and log_e.dtype == np.float32 and np.abs(log_e - r_log_e).max() <= 1e-5
        R.hold_energy(f"golden {name} log-energy", log_e, t_log_e)
        # bin 0 is the log-energy of the frame padded to fft_length, `log_e` that of the frame padded to `pad`: with raw_energy=False torch
        # sums rows of another length, in another order
        assert np.abs(spectrum[:, :, 0].real - log_e).max() <= 1e-5 and not spectrum[:, :, 0].imag.any()
    else:
        assert f"{name}/log_energy" not in arrays


def test_the_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(GOLDEN) < 256 * 1024
    arrays = np.load(GOLDEN, allow_pickle=False)
    assert {k.split("/")[0] for k in arrays.files} == set(R.GOLDEN_CASES)
    assert all(arrays[k].dtype in (np.float32, np.complex64) for k in arrays.files)
