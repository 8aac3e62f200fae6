"""GPU: the plans behind a stalled stream (the scenario: tests/_stalled_stream.py::run_scenario): ``extract_batch`` on
device tensors, ragged and uniform, at 16 kHz (fft512c); the same on a Whisper plan, whose fused normalisation block is armed by the
staging copy itself; a Whisper plan's ``run_collated`` (hipfeat_extract_collated: descriptors staged through the plan's ring, a padding
launch, the feature launch); and the launch pair of the on-the-fly mini-batch (``HipSpeedBank.extract_collated``: hipfeat_minibatch_plan
/ _run), which is what ``FusedMiniBatch`` runs for a collated batch.

P and Q are two batches of one extractor with different cut tables.  The waveforms arrive by a copy on the stalled stream into NaN-filled
buffers, so a descriptor copy, a padding launch or a feature launch on another stream reads NaN or is overwritten.  References and bars:
tests/test_gpu_parity.py::assert_parity against the float32 and float64 oracles (fbank), tests/test_gpu_whisper.py::_close (Whisper), and
for the mini-batch pair the per-factor route of tests/test_gpu_minibatch.py bit for bit plus the parity bar on the cuts that are not
resampled.  Each of these tests claims bit-equality between runs of the same call, so the stalled results are held to the bits of the
synchronised run."""
import numpy as np
import pytest
import torch

import test_gpu_minibatch as MB
import test_gpu_parity as TP
import test_gpu_whisper as TW
from _golden import ref32
from _stalled_stream import Call, run_scenario
from oracle import whisper_ref as W
from oracle.kaldi_ref import RefConfig, RefExtractor

import lhotse_amd as LA
from lhotse_amd import augmentation as A

pytestmark = pytest.mark.gpu
RING_ROUNDS = 2  # x (P, Q) = the 4 slots of a plan's ring
BANK_ROUNDS = 8  # x (P, Q) = the 16 slots of a speed bank


def _waves(seed, lens):
    rs = np.random.RandomState(seed)
    return [rs.rand(n).astype(np.float32) - np.float32(0.5) for n in lens]


def _batch_call(ex, waves, uniform, check_one):
    """``extract_batch`` on device tensors: a list of 1-D tensors (ragged) or one (B, T) tensor (uniform) -> device tensors."""
    lens = [len(w) for w in waves]
    bounds = np.concatenate([[0], np.cumsum(lens)])

    def run(bufs):
        flat = bufs["wave"]
        if uniform:
            out = ex.extract_batch(flat.view(len(lens), lens[0]), 16000)
            return list(out) if isinstance(out, (list, tuple)) else [out[b] for b in range(len(lens))]
        return list(ex.extract_batch([flat[bounds[b]: bounds[b + 1]] for b in range(len(lens))], 16000))

    def check(got):
        assert len(got) == len(waves)
        for w, o in zip(waves, got):
            check_one(w, o.numpy())

    return Call({"wave": torch.from_numpy(np.concatenate(waves))}, {}, run, check)


@pytest.mark.parametrize("shape", ["ragged", "uniform"])
def test_extract_batch_fbank(shape):
    ex = LA.HipFbank()
    assert ex.kernel_name.startswith("fft512c"), ex.kernel_name
    o32, o64 = ref32(RefConfig(kind="fbank")), RefExtractor(RefConfig(kind="fbank"), np.float64)

    def check_one(w, o):
        want = o32.extract(w)
        assert o.shape == want.shape
        TP.assert_parity(o, want, o64.extract(w), ("stalled stream", len(w)), suite="stalled_stream", kernel=ex.kernel_name)

    if shape == "ragged":
        P, Q = _waves(1, [1601, 400, 160 * 33, 7777]), _waves(2, [161, 160 * 32 + 79, 1599, 3000, 140])
    else:
        P, Q = _waves(3, [5200] * 3), _waves(4, [1601] * 5)
    run_scenario(f"extract_batch fbank {shape}", _batch_call(ex, P, shape == "uniform", check_one), _batch_call(ex, Q, shape == "uniform", check_one), RING_ROUNDS)


def _whisper_check(w, o):
    filters = W.slaney_mel_filters()
    TW._close(o, W.log_mel_spectrogram(w, filters, dtype=np.float32), W.log_mel_spectrogram(w, filters, dtype=np.float64), len(w))


def test_extract_batch_whisper():
    ex = LA.HipWhisperFbank()
    assert ex.kernel_name.startswith("whisper3_kernel"), ex.kernel_name  # the kernel with the fused normalisation
    P = _batch_call(ex, [w * np.float32(s) for w, s in zip(_waves(5, [8079, 201, 16000]), (0.5, 1.0, 0.1))], False, _whisper_check)
    Q = _batch_call(ex, [w * np.float32(s) for w, s in zip(_waves(6, [4000, 8080, 3000, 12345]), (1.0, 0.02, 0.9, 0.3))], False, _whisper_check)
    run_scenario("extract_batch whisper ragged", P, Q, RING_ROUNDS)


def _collated_call(ex, waves, pad_value):
    lens = np.array([len(w) for w in waves], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum((lens + 3) & ~3)[:-1]]).astype(np.int64)
    host = np.zeros(int(offs[-1] + lens[-1]), dtype=np.float32)
    for o, w in zip(offs, waves):
        host[o: o + len(w)] = w

    def run(bufs):
        out, frames = ex.plan.run_collated(bufs["wave"], offs, lens, None, pad_value)
        assert frames.tolist() == [W.num_rows(len(w)) for w in waves]
        return [out]

    def check(got):
        for b, w in enumerate(waves):
            t = W.num_rows(len(w))
            _whisper_check(w, got[0][b, :t].numpy())
            assert bool((got[0][b, t:] == np.float32(pad_value)).all())

    return Call({"wave": torch.from_numpy(host)}, {}, run, check)


def test_run_collated_whisper():
    """hipfeat_extract_collated (a Whisper plan keeps the three-launch route: tests/test_gpu_whisper.py)."""
    ex = LA.HipWhisperFbank()
    P = _collated_call(ex, _waves(7, [8079, 201, 16000]), LA.compat.LOG_EPSILON)
    Q = _collated_call(ex, _waves(8, [3000, 8080, 4000, 1234, 640]), -1.5)
    run_scenario("run_collated whisper", P, Q, RING_ROUNDS)


def _minibatch_call(ex, bank, seed, n, factors):
    rs = np.random.RandomState(seed)
    lens = rs.randint(2000, 9000, size=n).astype(np.int64)
    fac = rs.choice(factors, size=n)
    fac[: len(factors)] = factors
    offs = np.concatenate([[0], np.cumsum((lens + 3) & ~3)[:-1]]).astype(np.int64)
    front = int(offs[-1] + lens[-1])
    host = np.zeros(((front + 3) & ~3) + A.perturbed_tail_floats(lens, fac, 16000), dtype=np.float32)
    host[:front] = rs.uniform(-0.5, 0.5, size=front).astype(np.float32)
    index = bank.index_of(fac)
    o32, o64 = ref32(RefConfig(kind="fbank")), RefExtractor(RefConfig(kind="fbank"), np.float64)

    def run(bufs):
        feats, frames, po, pl = bank.extract_collated(ex.plan, bufs["arena"], offs, lens, index, front, MB.LOG_EPSILON)
        return [feats] + [bufs["arena"][int(o): int(o) + int(m)] for o, m, f in zip(po, pl, fac) if f != 1.0]

    def check(got):
        want_feats, frames, want_waves = MB._round3_route(ex, torch.from_numpy(host).cuda(), offs, lens, fac, front)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want_feats.cpu())  # features AND padding rows
        resampled = [w.cpu() for w, f in zip(want_waves, fac) if f != 1.0]
        assert len(resampled) == len(got) - 1 and all(torch.equal(a, b) for a, b in zip(got[1:], resampled))
        for b in np.flatnonzero(fac == 1.0):
            w = host[offs[b]: offs[b] + lens[b]]
            TP.assert_parity(got[0][b, : frames[b]].numpy(), o32.extract(w), o64.extract(w), ("stalled stream mini-batch", int(b)), suite="stalled_stream",
                             kernel=ex.kernel_name)

    return Call({"arena": torch.from_numpy(host)}, {}, run, check)


@pytest.mark.parametrize("tables", ["staged", "kernel-arguments"])
def test_minibatch_pair(monkeypatch, tables):
    if tables == "staged":
        monkeypatch.setenv("HIPFEAT_MB_NO_INLINE", "1")  # read when the bank is created
    ex = LA.HipFbank()
    bank = A.HipSpeedBank([0.9, 1.0, 1.1], 16000, "cuda")
    run_scenario(f"mini-batch pair, {tables}", _minibatch_call(ex, bank, 9, 5, [0.9, 1.0, 1.1]), _minibatch_call(ex, bank, 10, 7, [1.1, 1.0]), BANK_ROUNDS)
    bank.close()
