"""CPU, under the real lhotse (authoring container only): ``HipWav2Win`` / ``HipWav2FFT`` have the reference's constructor and attributes,
and ``_stft_ref.ref32`` -- the statement the GPU tests hold the device to -- equals the live ``Wav2Win`` / ``Wav2FFT`` with torch.equal on
the configurations of tests/test_gpu_stft.py."""
import inspect
import warnings

import numpy as np
import pytest
import torch

import _stft_ref as R

pytestmark = pytest.mark.reference


@pytest.fixture(scope="module")
def ref():
    from _dropin_support import import_lhotse

    import_lhotse()
    import lhotse.features.kaldi.layers as L

    import lhotse_amd as LA

    return LA, L


@pytest.mark.parametrize("mine,theirs", [("HipWav2Win", "Wav2Win"), ("HipWav2FFT", "Wav2FFT")])
def test_signatures_and_attributes_are_the_references(ref, mine, theirs):
    LA, L = ref
    # (lhotse_amd.layers postpones the evaluation of its annotations: eval_str resolves them to the objects the reference's carry)
    assert inspect.signature(getattr(LA, mine).__init__, eval_str=True) == inspect.signature(getattr(L, theirs).__init__, eval_str=True)
    assert inspect.signature(getattr(LA, mine), eval_str=True) == inspect.signature(getattr(L, theirs), eval_str=True)
    for kw in ({}, {"sampling_rate": 22050, "frame_shift": 0.0125, "window_type": "hamming", "energy_floor": 0.0, "raw_energy": False, "dither": 0.5},
               {"sampling_rate": 8000, "remove_dc_offset": False, "preemph_coeff": 0.0}):
        a, b = getattr(LA, mine)(**kw), getattr(L, theirs)(**kw)
        names = [k for k in vars(b) if not k.startswith("_") and k != "training" and not isinstance(vars(b)[k], torch.nn.Module)]
        names += ["sampling_rate", "frame_length", "frame_shift", "remove_dc_offset", "preemph_coeff", "window_type", "dither"]
        assert len(names) >= 8
        for k in names:
            assert getattr(a, k) == getattr(b, k), (mine, k)
        wa, wb = (a, b) if mine == "HipWav2Win" else (a.wav2win, b.wav2win)
        for k in ("_length", "_shift", "pad_length", "snip_edges", "energy_floor", "raw_energy", "return_log_energy"):
            assert getattr(wa, k) == getattr(wb, k), (mine, k)
        assert torch.equal(wa._window.data, wb._window.data) and not wa._window.requires_grad
        assert list(a.state_dict()) == list(b.state_dict())
        if mine == "HipWav2Win":
            assert str(a) == str(b).replace("Wav2Win(", "HipWav2Win(", 1)
        else:
            assert a.fft_length == b.fft_length and a.use_energy == b.use_energy
    with pytest.warns(UserWarning, match="snip_edges=True is generally incompatible"):
        getattr(LA, mine)(snip_edges=True)
    if mine == "HipWav2Win":
        assert LA.HipWav2Win(pad_length=777).pad_length == L.Wav2Win(pad_length=777).pad_length == 777
        for cls in (LA.HipWav2Win, L.Wav2Win):
            with pytest.raises(AssertionError, match="cannot be smaller than N = 400"):
                cls(pad_length=399)
    else:
        assert LA.HipWav2FFT(round_to_power_of_two=False).fft_length == L.Wav2FFT(round_to_power_of_two=False).fft_length == 400


@pytest.mark.parametrize("rate,n,fft", R.RATES, ids=[str(r[0]) for r in R.RATES])
def test_ref32_is_the_live_reference_bit_for_bit(ref, rate, n, fft):
    LA, L = ref
    for i, cfg in enumerate(R.option_grid(rate)):
        nn, shift, ff = R.K.window_sizes(cfg)
        assert (nn, ff) == (n, fft)
        all_lengths = R.lengths(n, shift, cfg.snip_edges)
        x = R.signal(i, 1 + 2 * (i % 2), all_lengths[i % len(all_lengths)])
        kw = R.layer_kwargs(cfg)
        with warnings.catch_warnings(), torch.no_grad():
            warnings.simplefilter("ignore")
            live = L.Wav2FFT(use_energy=cfg.use_energy, **kw)(torch.from_numpy(x))
            _, _, spectrum = R.ref32(x, cfg)
            assert live.dtype == torch.complex64 and torch.equal(live, torch.from_numpy(spectrum)), (i, cfg)
            for pad in (n, n + 1, fft):
                frames, log_e = L.Wav2Win(pad_length=pad, return_log_energy=cfg.use_energy, **kw)(torch.from_numpy(x))
                r_frames, r_log_e, _ = R.ref32(x, cfg, pad)
                assert torch.equal(frames, torch.from_numpy(r_frames)), (i, pad, cfg)
                assert (log_e is None) == (r_log_e is None) and (log_e is None or torch.equal(log_e, torch.from_numpy(r_log_e))), (i, pad, cfg)


def test_ref32_on_the_edge_shapes(ref):
    LA, L = ref
    for rate, n, fft in R.RATES:
        cfg = R.config(rate)
        _, shift, _ = R.K.window_sizes(cfg)
        kw = R.layer_kwargs(cfg)
        shortest = R.shortest_reflectable(n, shift)
        zero = np.zeros((3, 5 * shift), dtype=np.float32)
        zero[1] = R.signal(1, 1, 5 * shift)[0]
        for x in [R.signal(3, 3, s) for s in R.lengths(n, shift, False)] + [R.signal(4, 2, shortest), zero]:
            with torch.no_grad():
                live = L.Wav2FFT(**kw)(torch.from_numpy(x))
                frames, log_e = L.Wav2Win(pad_length=n + 1, return_log_energy=True, **kw)(torch.from_numpy(x))
            r_frames, r_log_e, _ = R.ref32(x, cfg, n + 1)
            assert torch.equal(live, torch.from_numpy(R.ref32(x, cfg)[2])) and torch.equal(frames, torch.from_numpy(r_frames))
            assert torch.equal(log_e, torch.from_numpy(r_log_e))
        # the all-zero row: zero frames, and the floor of the log-energy
        assert not frames[0].any() and not frames[2].any() and float(log_e[0, 0]) == np.float32(np.log(cfg.energy_floor))
        with pytest.raises(ValueError):
            R.truth(R.signal(5, 1, shortest - 1), cfg)
