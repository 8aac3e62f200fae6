"""CPU: every input of tests/_whisper_cases.py does what it claims, proved from the float64 oracle alone (oracle/whisper_ref.py) --
conditions on the reference, not measurements of the kernels.  tests/test_gpu_whisper_clamp.py relies on them to land on the code
paths of the Whisper normalisation (kernel_whisper3.hpp section 6, whisper_norm_kernel)."""
import numpy as np
import pytest

import _whisper_cases as WC
from lhotse_amd import constants as C
from oracle import whisper_ref as W

MELS = (80, 128, 81, 127, 23)   # every filter count tests/test_gpu_whisper_clamp.py uses
USED = {  # case -> filter counts it is run with on the GPU
    "mid": MELS, "tail": (80, 128), "head": (80, 128), "spots": (80, 128), "tail_odd": (81, 127, 23), "long_odd": (23,),
    "dropped": (80, 128, 81), "loud": (80, 128, 81), "pad_only": (80, 81),
}
PAIRS = [(name, m) for name, ms in USED.items() for m in ms]


@pytest.mark.parametrize("n_mels", MELS)
def test_the_package_and_the_oracle_build_the_same_filterbank(n_mels):
    """BIT FOR BIT (both evaluate librosa's formula in float64 and round once), so the GPU tests may take the oracle's filters."""
    mine = C.make_slaney_mel(n_mels, W.N_FFT, W.SAMPLING_RATE)
    assert mine.dtype == np.float32 and mine.shape == (201, n_mels)
    assert np.array_equal(mine.T, WC.filters(n_mels))


def test_every_case_is_used_and_shaped_as_it_says():
    assert set(USED) == set(WC.CASES)
    for c in WC.CASES.values():
        x = WC.signal(c.name)
        assert x.dtype == np.float32 and len(x) == c.num_samples and len(x) // 160 == c.frames
        assert len(x) % 160 >= 80 and c.rows == c.frames + 1, "every case ends with the zero padding row"
    assert WC.CASES["tail_odd"].frames % 4 != 0 and all((WC.CASES["tail_odd"].frames * m) % 4 != 0 for m in (81, 127, 23))
    assert (WC.CASES["long_odd"].frames * 23) % 4 != 0 and WC.CASES["long_odd"].frames * 23 // 4 > 24576  # kKeep x 1024 of whisper_norm_kernel
    assert WC.CASES["mid"].frames * 80 // 4 <= 24576 < WC.CASES["mid"].frames * 128 // 4                    # held in registers / two reads
    assert WC.CASES["pad_only"].frames % 64 == 0
    for k in (1, 17):
        lens = WC.boundary_lengths(k)
        f0 = 4 * k  # the wave's first frame: its span is the samples f0 * 160 - 200 .. + 880
        assert [f0 * 160 - 200 + 880 <= s for s in lens] == [False, True, True]


@pytest.mark.parametrize("name,n_mels", PAIRS, ids=["%s-%d" % p for p in PAIRS])
def test_case_does_what_it_claims(name, n_mels):
    c = WC.CASES[name]
    x = WC.signal(name)
    raw = WC.raw_log_mel(x, n_mels)
    truth, _ = WC.reference(name, n_mels)
    # the restated front end IS the oracle's: clamp + affine + padding row on top of it reproduce log_mel_spectrogram
    assert raw.shape == (c.frames, n_mels) and np.allclose(WC.finish(raw, c.rows), truth, rtol=0, atol=1e-12)
    assert raw.min() > -9.0, "a decade above the 1e-10 mel floor: the floor must not stand in for the clamp"
    level = raw.max() - 8.0
    under = float((raw < level).mean())
    if c.acts:
        assert 0.05 <= under <= 0.95, under
        assert np.abs(raw - level).min() >= WC.MARGIN
        assert abs((truth[: c.frames].max() - truth[: c.frames].min()) - 2.0) < 1e-12
    else:
        assert under == 0.0 and raw.min() > level + 0.25
    for fpw, classes in c.blocks:
        assert WC.classify(raw, fpw) == classes, (fpw, WC.classify(raw, fpw))
    if c.blocks and name not in ("spots", "pad_only"):  # (those two: partial blocks only, by their purpose)
        assert any(set(classes) == {"n", "p", "a"} for _, classes in c.blocks), "a block wholly under the clamp, one partly and one not at all"
    if name == "loud":
        assert (raw.max() - 4.0) / 4.0 >= 0.25  # the clamp level in output units: max(0, c) != 0
        assert float(np.abs(x).max()) > 1e4
    if name == "dropped":
        # frame `frames` (dropped by the reference) is the only one that sees the burst: frame frames - 1 ends at sample frames * 160 + 39
        assert np.abs(x[c.frames * 160 + 40:]).max() > 1e5
        quiet = x.copy()
        quiet[c.frames * 160 + 40:] = 0.0
        assert np.allclose(WC.raw_log_mel(quiet, n_mels)[: c.frames], raw, rtol=0, atol=1e-9), "the kept frames do not see the burst"
        with_dropped = WC.raw_log_mel(x, n_mels, keep_dropped=True)
        assert with_dropped.shape[0] == c.frames + 1 and np.allclose(with_dropped[:-1], raw, rtol=0, atol=1e-9)
        wrong = WC.finish(raw, c.rows, cut_max=with_dropped.max())
        moved = np.abs(wrong - truth)[: c.frames] >= 0.1
        assert moved.mean() >= 0.10, moved.mean()   # (measured: 53 % of the elements, by up to 1.2)


def test_white_noise_alone_never_reaches_the_clamp():
    """Why the earlier strided / repeated-launch tests never changed a value in the sweep: plain noise spans under 5 decades."""
    raw = WC.raw_log_mel(WC.noise(160000, 0.8, 11), 80)
    assert raw.max() - raw.min() < 5.5
