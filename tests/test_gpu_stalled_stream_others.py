"""GPU: the entry points without tickets behind a stalled stream (the scenario: tests/_stalled_stream.py::run_scenario):
``HipResampleTensor.run`` (hipfeat_resample, a resampler's ring of 4), ``apply_specaug`` (hipfeat_specaug, its ring of 4),
``HipGlobalMVN`` (hipfeat_global_mvn), hipfeat_pcm16_to_float, hipfeat_float_to_half and ``HipStatsAccumulator.update``.

The two conversions have no Python wrapper of their own (the extractors call them in the middle of larger methods), so they are called as
tests/test_gpu_collated.py and tests/test_gpu_host_pipeline.py call them, on torch's current stream.  The accumulator's calls are for ONE
stream at a time (include/hipfeat.h), so its scenario has no second stream, and its result is its state, read after the stalled stream
has been waited for.  References and bars are those of each kind's own GPU test; every kind claims run-to-run bit-equality there
(resample: test_fast_and_generic_kernels_are_bit_identical; specaug: "a second run of the same call returns the same bits"; global MVN:
torch bit for bit; stats: "bit-identical from run to run"), and the conversions are exact."""
import time

import numpy as np
import pytest
import torch

import _specaug_cases as C
import _stats_gpu as G
import test_gpu_resample
import test_gpu_specaug_edges as E
from _stalled_stream import Call, Stall, run_scenario, side_streams, stall_ms_for

from lhotse_amd import _lib, augmentation as A
from lhotse_amd.signal_transforms import apply_specaug
from lhotse_amd.stats import HipStatsAccumulator
from oracle import resample_ref as R

pytestmark = pytest.mark.gpu
RING_ROUNDS = 2  # x (P, Q) = the 4 slots of a plan's, a resampler's or the specaug ring
NAN = float("nan")


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


# ---- HipResampleTensor ----------------------------------------------------------------------------------------------------------
def _resample_call(r, seed, lens):
    rng = np.random.RandomState(seed)
    xs = [rng.rand(n).astype(np.float32) - np.float32(0.5) for n in lens]
    offsets = np.cumsum([0] + lens[:-1]).astype(np.int64)

    def run(bufs):
        out, out_offs, out_lens = r.run(bufs["wave"], offsets, np.asarray(lens, dtype=np.int64))
        return [out[o : o + n] for o, n in zip(out_offs.tolist(), out_lens.tolist())]

    def check(got):
        for x, y in zip(xs, got):
            want = R.resample(x, r.orig_freq, r.new_freq, dtype=np.float64)
            assert y.numel() == len(want) and np.abs(y.numpy() - want).max() <= test_gpu_resample.ABS_TOL, len(x)

    return Call({"wave": torch.from_numpy(np.concatenate(xs))}, {}, run, check)


@pytest.mark.parametrize("orig,new,kernel", [(17600, 16000, "resample_fast<11,10,7>"), (16000, 22050, None)])
def test_resample_tensor(orig, new, kernel):
    r = A.HipResampleTensor(orig, new)
    assert not r.bankless and (kernel is None or r.kernel_name == kernel)
    run_scenario(f"resample {orig}->{new} ({r.kernel_name})", _resample_call(r, 61, [4097, 37, 160]), _resample_call(r, 62, [23, 1, 4095, 300, 2]), RING_ROUNDS)
    r.close()


# ---- specaug --------------------------------------------------------------------------------------------------------------------
def _specaug_call(i):
    name, x, segs, masks = E._ring_call(i)  # (2, 50, 16) with its own segments and masks

    def run(bufs):
        return [apply_specaug(bufs["x"], [segs], masks)]

    def check(got):
        E.judge(name, x, [segs], masks, got[0].numpy())

    return Call({"x": torch.from_numpy(x)}, {}, run, check)


def test_specaug():
    run_scenario("specaug", _specaug_call(0), _specaug_call(2), RING_ROUNDS)


# ---- global MVN -----------------------------------------------------------------------------------------------------------------
def _mvn_call(case, inverse):
    """The statistics live on the device (``.cuda()``): a module that keeps them on the host copies them over in every call, and that copy
    from pageable memory waits for the stream -- torch's semantics, not the library's."""
    name, x, means, stds = case
    mvn = E._mvn(means, stds).cuda()
    want = E._torch_cpu(x, means, stds)[inverse]

    def run(bufs):
        return [mvn.inverse(bufs["x"]) if inverse else mvn(bufs["x"])]

    def check(got):
        assert C.same_bits_nan_by_position(got[0].numpy(), want), name

    return Call({"x": torch.from_numpy(x)}, {}, run, check)


def test_global_mvn():
    by_dim = {c[1].shape[1]: c for c in sorted(E.MVN, key=lambda c: c[1].shape[0])}  # per F the case of the most rows
    run_scenario("global_mvn", _mvn_call(by_dim[80], 0), _mvn_call(by_dim[3], 1), 1)
    torch.cuda.synchronize()


# ---- the two conversions --------------------------------------------------------------------------------------------------------
def _pcm_call(seed, n):
    pcm = np.random.RandomState(seed).randint(-32767, 32768, size=n).astype(np.int16)  # (-32768 is the poison of the input buffer)

    def run(bufs):
        _lib.load().check("hipfeat_pcm16_to_float", bufs["pcm"].data_ptr(), bufs["out"].data_ptr(), n, _stream())
        return [bufs["out"]]

    def check(got):
        assert np.array_equal(got[0].numpy(), pcm.astype(np.float32) / np.float32(32768.0))

    return Call({"pcm": torch.from_numpy(pcm)}, {"out": ((n,), torch.float32, NAN)}, run, check)


def test_pcm16_to_float():
    run_scenario("pcm16_to_float", _pcm_call(71, 4097), _pcm_call(72, 1023), 1)


def _half_call(seed, n):
    rs = np.random.RandomState(seed)
    x = (rs.randn(n) * 10.0 ** rs.uniform(-6, 5, size=n)).astype(np.float32)  # normal, subnormal and overflowing binary16 values

    def run(bufs):
        _lib.load().check("hipfeat_float_to_half", bufs["x"].data_ptr(), bufs["out"].data_ptr(), n, _stream())
        return [bufs["out"]]

    def check(got):
        with np.errstate(over="ignore"):
            assert np.array_equal(got[0].view(torch.int16).numpy(), x.astype(np.float16).view(np.int16))

    return Call({"x": torch.from_numpy(x)}, {"out": ((n,), torch.float16, 0x7FFF)}, run, check)


def test_float_to_half():
    run_scenario("float_to_half", _half_call(73, 4099), _half_call(74, 513), 1)


# ---- HipStatsAccumulator.update -------------------------------------------------------------------------------------------------
def test_stats_update():
    """Steps 1 - 3 and 5: P and Q are two packed updates with different cut tables; the state after (reset, P, Q) behind the stall is,
    bit for bit, the state after the same three calls made with a synchronise behind each."""
    F = 23
    rng = np.random.default_rng(81)
    updates = []
    for frames in ([300, 1, 257], [5, 256, 2, 40, 513]):
        mats = [rng.standard_normal((n, F)).astype(np.float32) * 3 + 1 for n in frames]
        updates.append((mats, torch.from_numpy(np.concatenate(mats)).pin_memory(), frames))
    acc = HipStatsAccumulator(F, "cuda:0")

    def enqueue(bufs):
        for (_, host, frames), dev in zip(updates, bufs):
            dev.copy_(host, non_blocking=True)
        for (_, _, frames), dev in zip(updates, bufs):
            acc.update(dev, frames)

    poisoned = lambda: [torch.full(host.shape, NAN, dtype=torch.float32, device="cuda") for _, host, _ in updates]  # noqa: E731
    for _ in range(8):  # 16 updates: every slot of the accumulator's ring has made its first allocation, and the slab is there
        acc.reset()
        bufs = poisoned()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enqueue(bufs)
        enqueue_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
    want = G.bits(acc)
    all_mats = updates[0][0] + updates[1][0]
    assert want[0] == sum(len(m) for m in all_mats)
    G.hold_to_the_bar("stalled stream", acc, G.reference_over(F, all_mats), all_mats)
    acc.reset()
    bufs = poisoned()
    torch.cuda.synchronize()
    S = side_streams()[0]
    ms = stall_ms_for(enqueue_ms)
    print(f"stats update: warm-up enqueue {enqueue_ms:.3f} ms, stall {ms:.0f} ms")
    stall = Stall(S, ms)
    with torch.cuda.stream(S):
        enqueue(bufs)
    assert stall.still_stalled(), "the host did not finish enqueuing the two updates while the stream was stalled"
    S.synchronize()
    with torch.cuda.stream(S):
        got = G.bits(acc)
    assert G.same_bits(got, want)
    acc.close()
