"""CPU: the gradient sweep of tests/_grad_sweep.py against the restatement alone, so that tests/test_gpu_grad_sweep.py cannot pass vacuously.

The device is held to ``max(2 E(g32), 1e-6)``, which is a bar only where the float32 autograd ``g32`` is itself accurate and where the
float64 gradient does not sit on a discontinuity that float32 may fall on the other side of.  Every condition here is on the reference,
never on the device: the cap on E(g32), the margins from MEL_FLOOR and log(energy_floor), that the excluded cases are few and each really
breaks a condition, and that the kept list reaches the branches of csrc/kernel_grad.hpp the sweep exists for.
"""
import numpy as np
import pytest

import _grad_ref as GR
import _grad_sweep as SW


@pytest.fixture(scope="module")
def refs():
    return {i: SW.reference(i) for i in range(SW.NUM_CASES)}


@pytest.fixture(scope="module")
def kept(refs):
    return [refs[i] for i in SW.KEPT]


def test_the_case_list_is_seeded_and_has_the_input_shape_of_the_issue():
    assert SW.NUM_CASES == 160 and len(SW.KEPT) + len(SW.EXCLUDED) == 160 and set(SW.EXCLUDED) <= set(range(160))
    for i in range(SW.NUM_CASES):
        cls, kw = SW.sweep_case(i)
        assert (cls, kw) == SW.sweep_case(i) and kw.get("round_to_power_of_two", True)
        n, shift, fft = GR.sizes(kw, cls)
        x = SW.sweep_input(i)
        assert x.dtype == np.float32 and x.shape[0] == 3 and n + 5 * shift <= x.shape[1] < n + 6 * shift and shift <= n
        assert 6 <= GR.num_frames(x.shape[1], n, shift, kw["snip_edges"]) <= 9  # (9: a 32 ms frame on an 8 ms shift, without snip_edges)
        assert cls == "Wav2Win" or fft in SW.FFT_SIZES
        assert np.array_equal(x, SW.sweep_input(i))
        peak = np.abs(x).max(axis=1)
        assert 0.5 < peak[0] <= 0.75 and peak[1] <= 0.02 * 0.75 and peak[2] <= 3e-4 * 0.75


def test_every_kept_case_is_a_bar_and_every_excluded_one_is_not(refs):
    worst, reasons = 0.0, {}
    for i in range(SW.NUM_CASES):
        why = SW.why_excluded(refs[i])
        if why is not None:
            reasons[i] = why
        else:
            worst = max(worst, float(refs[i]["e32"].max()))
            assert np.isfinite(refs[i]["g64"]).all() and np.isfinite(refs[i]["g32"]).all()
    smallest = min(r["mel_margin"] for i, r in refs.items() if i not in reasons)
    print(f"[grad-sweep] kept {len(SW.KEPT)}  excluded {len(SW.EXCLUDED)}  worst E(g32) of a kept row {worst:.3g}  smallest kept mel margin {smallest:.3g}")
    for i, why in sorted(reasons.items()):
        print(f"[grad-sweep] case {i} {refs[i]['cls']} breaks a condition: {why} (listed: {SW.EXCLUDED.get(i)})")
    assert set(reasons) == set(SW.EXCLUDED), (reasons, SW.EXCLUDED)  # nothing is kept that breaks one, nothing is excluded for convenience
    assert len(SW.EXCLUDED) <= 0.05 * SW.NUM_CASES
    assert worst <= SW.CAP and smallest >= SW.MARGIN


def test_every_kept_row_has_a_gradient_to_be_held_to(kept):
    """No kept case is vacuous: a row whose float64 gradient is zero is held to exact zeros only, and that is for the targeted tests."""
    for r in kept:
        assert np.linalg.norm(r["g64"], axis=1).min() > 0.0, (r["cls"], r["kw"])


def test_coverage_of_the_kept_list(kept):
    def some(pred):
        return sum(1 for r in kept if pred(r, r["cls"], r["kw"], GR.sizes(r["kw"], r["cls"])))

    for cls in GR.CLASSES:
        assert some(lambda r, c, kw, z: c == cls) >= 15, cls
    for fft in SW.FFT_SIZES:
        assert some(lambda r, c, kw, z: c != "Wav2Win" and z[2] == fft), fft
    assert some(lambda r, c, kw, z: c != "Wav2Win" and z[0] == z[2]), "N == fft"
    assert some(lambda r, c, kw, z: z[0] % 2 == 1), "an odd N"
    assert some(lambda r, c, kw, z: z[0] % 2 == 1 and c != "Wav2Win"), "an odd N in a spectral class"
    assert some(lambda r, c, kw, z: z[1] == z[0]), "shift == N"
    for window in SW.WINDOWS:
        assert some(lambda r, c, kw, z: kw["window_type"] == window), window
    for m in (64, 65, 128):
        assert some(lambda r, c, kw, z: kw.get("num_filters") == m), m
    assert some(lambda r, c, kw, z: r["empty_filters"] > 0), "a filterbank with an empty filter"
    for norm in (False, True):
        assert some(lambda r, c, kw, z: kw.get("torchaudio_compatible_mel_scale") is False and kw["norm_filters"] == norm), ("HTK", norm)
    assert some(lambda r, c, kw, z: kw.get("cepstral_lifter") == 0), "cepstral_lifter == 0"
    assert some(lambda r, c, kw, z: r["mel_floored"] is not None and ((r["mel_floored"] > 0) & (r["mel_floored"] < 1)).any()), "a partly mel-floored row"
    assert some(lambda r, c, kw, z: r["energy_floored"] is not None and r["energy_floored"].max() == 1 and r["energy_floored"].min() == 0), \
        "rows on both sides of the energy floor"
    assert some(lambda r, c, kw, z: c == "Wav2Win" and z[2] % 2 == 1), "Wav2Win with an odd pad_length"
    assert some(lambda r, c, kw, z: c == "Wav2Win" and z[0] > 1024), "Wav2Win with N > 1024"
    # the remaining values of the option table, each at least once
    for key, values in (("preemph_coeff", (0.97, 0.0, 0.9)), ("energy_floor", (GR.EPSILON, 0.0, 1e-3, 1.0)), ("low_freq", (20.0, 0.0, 60.0)),
                        ("high_freq", (-400.0, 0.0, -100.0)), ("cepstral_lifter", (22, 10, 0)), ("remove_dc_offset", (False, True)),
                        ("snip_edges", (False, True)), ("raw_energy", (False, True)), ("use_fft_mag", (False, True))):
        for v in values:
            assert some(lambda r, c, kw, z: kw.get(key) == v and type(kw.get(key)) is type(v)), (key, v)
