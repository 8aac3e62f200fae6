"""GPU: one round of the wave-autonomous kernels (fft512c at 16 kHz, fft256c at 8 kHz) at its edges.

The first FFT pass never reads the rows of a frame that are zero by construction, the LDS exchange between the passes is one
instruction sequence with a single wait, the lane table comes in one 16-byte read per set and the window reads stay in flight over the
request for the next span.  None of that may change a value, so every case runs the fast route next to the generic kernel
(HIPFEAT_FORCE_GENERIC=1 in a fresh plan) and next to oracle/kaldi_ref.py in float64, under the parity statement of oracle/parity_bar.py
as it stands (ref32 = the reference's own float32 arithmetic); the two kernels are held to its norm-wise clause against each other.

  frame lengths   20 ms (10 live rows), 24 ms (12 full rows and an empty 13th), 25 ms (row 12 half masked), 32 ms (16 rows: no pruning)
  modes           fbank 80 (two accumulator sets), fbank 23 (one set), MFCC 40 x 40, MFCC 23 x 13
  inputs          seeded noise, an all-zero cut, a cut that is -0.0 throughout, an impulse at sample 0 and one at the last sample of a frame
  options         remove_dc_offset on / off  x  preemph_coeff 0.97 / 0
  cut lengths     1, 3, 4, 5, 31, 32, 33, 257 frames (fewer than 4 frames, one round, an edge round followed by an interior one, the last
                  wave of a workgroup), each cut on its own, all of them as one ragged batch (frame-quad layout where the instance has
                  one) and as one zero-padded batch

At 16 kHz a 32 ms frame with the 10 ms shift is over the kernel's LDS budget (eight spans of 3 shifts + 512 samples) and goes to the
16-frame-tile kernel; with a 5 ms shift it takes the 16-row instance of fft512c, so that is the shift of the 32 ms cases there.  A 32 ms
frame needs more samples of reflection on either side than a one-frame cut has: the reference raises there, so at 32 ms the one-frame cut
appears in the zero-padded batch only.
"""
import numpy as np
import pytest

from _golden import ref32 as ref32_of
from _hip import make_hip
from oracle import parity_bar
from oracle.kaldi_ref import RefConfig, RefExtractor, window_sizes

pytestmark = pytest.mark.gpu

FRAME_LENGTHS = [0.020, 0.024, 0.025, 0.032]
MODES = {
    "fbank80": ("fbank", {}),
    "fbank23": ("fbank", {"num_filters": 23}),
    "mfcc40x40": ("mfcc", {"num_filters": 40, "num_ceps": 40}),
    "mfcc23": ("mfcc", {"num_filters": 23}),
}
OPTIONS = [(True, 0.97), (True, 0.0), (False, 0.97), (False, 0.0)]
MODES_8K = {"fbank80": ("fbank", {}), "fbank40": ("fbank", {"num_filters": 40})}  # the filterbanks that take fft256c there
FRAME_COUNTS = [1, 3, 4, 5, 31, 32, 33, 257]


def _frame_shift(sr, frame_length):
    return 0.005 if (sr, frame_length) == (16000, 0.032) else 0.01


def _waves(sr, frame_length):
    n, shift, _ = window_sizes(RefConfig(sampling_rate=sr, frame_length=frame_length, frame_shift=_frame_shift(sr, frame_length)))
    rs = np.random.RandomState(11)
    waves = [(rs.rand(k * shift).astype(np.float32) - 0.5) for k in FRAME_COUNTS]
    zero = np.zeros(max(5, (n + shift - 1) // shift + 3) * shift, dtype=np.float32)  # a few frames: frame 2 lies inside
    first = zero.copy()
    first[0] = 0.5
    last = zero.copy()
    last[2 * shift - (n - shift) // 2 + n - 1] = 0.5  # tap N - 1 of frame 2
    return waves + [zero, -zero, first, last]


def _judge(got, want, truth, log_mel, ctx):
    f = parity_bar.fold([parity_bar.figures(g, w, t, log_mel=log_mel) for g, w, t in zip(got, want, truth)])
    v = parity_bar.verdict(f)
    assert v["pass_rel_l2"] and v["pass_linear"] and v["pass_elementwise"], (ctx, v, f)


def _check_round(sr, frame_length, mode, kernel_prefix, monkeypatch):
    kind, extra = (MODES if sr == 16000 else MODES_8K)[mode]
    waves = _waves(sr, frame_length)
    n, shift, _ = window_sizes(RefConfig(sampling_rate=sr, frame_length=frame_length, frame_shift=_frame_shift(sr, frame_length)))
    reflectable = [w for w in waves if (n - shift) // 2 <= len(w)]  # (the reference raises on the others)
    assert len(reflectable) >= len(waves) - 1
    for dc, pre in OPTIONS:
        cfg = dict(sampling_rate=sr, frame_length=frame_length, frame_shift=_frame_shift(sr, frame_length), remove_dc_offset=dc, preemph_coeff=pre, **extra)
        rc = RefConfig(kind=kind, **cfg)
        o64, o32 = RefExtractor(rc, np.float64), ref32_of(rc)
        for rule, items in (("reflect", reflectable), ("batch_zero_pad", waves)):
            ctx = (sr, frame_length, mode, dc, pre, rule)
            fast = make_hip(kind, cfg, edge_rule=rule)
            assert fast.kernel_name.startswith(kernel_prefix), (ctx, fast.kernel_name)
            monkeypatch.setenv("HIPFEAT_FORCE_GENERIC", "1")
            slow = make_hip(kind, cfg, edge_rule=rule)
            assert "generic" in slow.kernel_name, (ctx, slow.kernel_name)
            monkeypatch.delenv("HIPFEAT_FORCE_GENERIC")
            a, b = fast.extract_batch(items, sr), slow.extract_batch(items, sr)
            want, truth = o32.extract_batch(items, rule), o64.extract_batch(items, rule)
            assert len(a) == len(b) == len(items)
            for w, fa, fb, wa, tr in zip(items, a, b, want, truth):
                assert fa.shape == fb.shape == wa.shape == tr.shape, (ctx, len(w))
                assert np.isfinite(fa).all(), (ctx, len(w))
                rel = np.linalg.norm(fa.astype(np.float64) - fb) / np.linalg.norm(fb.astype(np.float64))
                assert rel <= parity_bar.REL_L2_TOL, (ctx, len(w), rel)
            _judge(a, want, truth, kind == "fbank", ctx + ("fast",))
            _judge(b, want, truth, kind == "fbank", ctx + ("generic",))
            if rule == "reflect":  # a cut on its own (one cut per launch, no frame-quad layout) == the cut inside the ragged batch, bit for bit
                for w, fa in zip(items, a):
                    assert np.array_equal(fast.extract(w, sr), fa), (ctx, len(w))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("frame_length", FRAME_LENGTHS)
def test_fft512c_round_edges(frame_length, mode, monkeypatch):
    _check_round(16000, frame_length, mode, "fft512c_kernel", monkeypatch)


@pytest.mark.parametrize("mode", list(MODES_8K))
@pytest.mark.parametrize("frame_length", FRAME_LENGTHS)
def test_fft256c_round_edges(frame_length, mode, monkeypatch):
    """The same list at 8 kHz, with the filterbanks that take the wave-autonomous kernel there."""
    _check_round(8000, frame_length, mode, "fft256c_kernel", monkeypatch)

