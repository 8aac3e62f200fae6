"""CPU: tests/golden/stream.npz (written by tests/_stream_golden.py from the LIVE layers' ``online_inference``) holds the inputs the tests
regenerate from their seeds and, per call of each chunk sequence, an output and a remainder that the restated framing of
tests/_stream_ref.py reproduces: the remainders exactly (they are slices), the outputs to the bars the device is held to."""
import os

import numpy as np
import pytest

import _stft_ref as R
import _stream_ref as SR
from oracle import kaldi_ref as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream.npz")


def case_sizes(name):
    cls, kw, _, _ = SR.GOLDEN_CASES[name]
    cfg = K.RefConfig(kind="spectrogram", sampling_rate=kw.get("sampling_rate", 16000))
    n, shift, fft = K.window_sizes(cfg)
    return n, shift, fft


def check_call(name, i, V, T, out, log_e):
    """One call's stored output against the statements on V."""
    cls, kw, batch, _ = SR.GOLDEN_CASES[name]
    n, shift, fft = case_sizes(name)
    if cls == "Wav2Win":
        cfg = SR.stft_config(kw, "return_log_energy")
        pad = kw.get("pad_length", n)
        r_frames, r_log_e, _ = SR.ref32(V, cfg, pad)
        t_frames, t_log_e, _ = SR.truth(V, cfg, pad)
        assert out.shape == (batch, T, pad) and out.dtype == np.float32 and R.frame_error(r_frames, out) <= 1e-6
        R.hold(f"golden {name}/{i} frames", out, out, t_frames)
        assert (log_e is not None) == cfg.use_energy
        if log_e is not None:
            assert log_e.shape == (batch, T) and np.abs(log_e - r_log_e).max() <= 1e-5
            R.hold_energy(f"golden {name}/{i} log-energy", log_e, t_log_e)
    elif cls == "Wav2FFT":
        cfg = SR.stft_config(kw, "use_energy")
        assert out.shape == (batch, T, fft // 2 + 1) and out.dtype == np.complex64 and R.frame_error(SR.ref32(V, cfg)[2], out) <= 1e-6
        R.hold(f"golden {name}/{i} spectrum", out, out, SR.truth(V, cfg)[2], energy_bin=cfg.use_energy)
    else:
        cfg = SR.golden_feature_config(name)
        want = SR.features_truth(V, cfg)
        assert out.dtype == np.float32 and out.shape == want.shape and out.shape[:2] == (batch, T)
        for b in range(batch):
            SR.hold_features(SR.KINDS[cls], cfg.use_energy, out[b].astype(np.float64), want[b])


@pytest.mark.parametrize("name", sorted(SR.GOLDEN_CASES))
def test_the_goldens_are_the_cases_and_the_restated_stream_reproduces_them(name):
    arrays = np.load(GOLDEN)
    cls, kw, batch, sizes = SR.GOLDEN_CASES[name]
    n, shift, _ = case_sizes(name)
    x = SR.golden_input(name)
    assert x.dtype == np.float32 and np.array_equal(arrays[f"{name}/x"], x)
    frames = 0
    for i, (chunk, context, V, T, remainder) in enumerate(SR.walk(x, sizes, n, shift, kw.get("snip_edges", False))):
        assert T >= 1 and np.array_equal(arrays[f"{name}/{i}/remainder"], remainder)
        key = f"{name}/{i}/log_energy"
        check_call(name, i, V, T, arrays[f"{name}/{i}/out"], arrays[key] if key in arrays.files else None)
        frames += T
    assert f"{name}/{len(sizes)}/out" not in arrays.files and 5 <= frames <= 9


def test_the_fixture_is_small_and_holds_data_only():
    assert os.path.getsize(GOLDEN) < 300 * 1024
    arrays = np.load(GOLDEN, allow_pickle=False)
    assert {k.split("/")[0] for k in arrays.files} == set(SR.GOLDEN_CASES)
    assert all(arrays[k].dtype in (np.float32, np.complex64) for k in arrays.files)
