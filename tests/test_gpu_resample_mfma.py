"""GPU: the matrix-core resampler (resample_mfma_kernel) for ratios with many phases.

Its contract is the summation order of resample_kernel (accumulator from 0, taps ascending, one fma per tap), so its outputs must be
EQUAL to the generic kernel's (``torch.equal``), not merely close; the generic kernel's own bar against the float64 oracle
(``ABS_TOL`` of tests/test_gpu_resample.py: the reference's float32 bank, only the summation order differs from conv1d) then holds
for it as well.  Which kernel ran is read from ``HipResampleTensor.kernel_name``."""
import numpy as np
import pytest
import torch

import _resample_rates as RATES

from lhotse_amd import _lib, augmentation as A
from oracle import resample_ref as R

pytestmark = pytest.mark.gpu
ABS_TOL = 1e-5  # tests/test_gpu_resample.py
MFMA_RATES, IDS = RATES.ROUTED, RATES.ROUTED_IDS


def pair(orig, new, monkeypatch):
    """(resampler on the kernel the library routes the ratio to, the same ratio forced onto the generic kernel)"""
    routed = A.HipResampleTensor(orig, new)
    monkeypatch.setenv("HIPFEAT_RESAMPLE_GENERIC", "1")
    generic = A.HipResampleTensor(orig, new)
    monkeypatch.delenv("HIPFEAT_RESAMPLE_GENERIC")
    return routed, generic


def input_length_for(orig, nw, out_len):
    """An input length whose output has `out_len` samples, or, where no input gives it (an up-sampling ratio makes output lengths
    in steps of more than one), the nearest one it can have from above."""
    n = (out_len * orig) // nw
    while R.resampled_length(n, orig, nw) < out_len:
        n += 1
    while n > 0 and R.resampled_length(n - 1, orig, nw) >= out_len:
        n -= 1
    return n


def hops_per_workgroup(orig, kw):
    """resample_tables.hpp: 16 hops times the most hop tiles (4, 2, 1) whose input span fits 64 KiB of LDS"""
    kwp = -(-kw // 16) * 16
    return next(16 * ht for ht in (4, 2, 1) if 4 * (((16 * ht - 1) * orig + kwp + 3) & ~3) <= 65536)


def edge_lengths(orig, nw, kw):
    """Input lengths whose outputs are 0 and 1 samples, nw - 1 / nw / nw + 1, 16 k nw - 1 / 16 k nw / 16 k nw + 1 (k = 1, 2, 4, 8: whole
    hop tiles, with one sample less and one more) and three workgroups plus an odd remainder."""
    outs = [0, 1, nw - 1, nw, nw + 1]
    for k in (1, 2, 4, 8):
        outs += [16 * k * nw - 1, 16 * k * nw, 16 * k * nw + 1]
    outs.append(3 * hops_per_workgroup(orig, kw) * nw + 77)
    lens = [input_length_for(orig, nw, o) for o in outs]
    got = [R.resampled_length(n, orig, nw) for n in lens]
    if nw < orig:  # down-sampling reaches every output length
        assert got == outs
    else:
        assert all(0 <= g - o < -(-nw // orig) for g, o in zip(got, outs))
    return lens


@pytest.fixture(scope="module")
def batches():
    """Per ratio: the ragged inputs (fixed seed) -- made once, shared, never changed."""
    out = {}
    for orig, new in MFMA_RATES + RATES.EXTRA:
        kernel, _, o, n = A.constants.sinc_resample_kernel(orig, new)
        rng = np.random.RandomState(orig % 991 + new % 13)
        lens = edge_lengths(o, n, kernel.shape[1])
        assert lens[0] == 0  # a cut without samples: no output, no workgroup
        out[(orig, new)] = [(rng.rand(m).astype(np.float32) - 0.5) for m in lens]
    return out


def mfma_pair(orig, new, monkeypatch):
    """(resampler on the matrix-core kernel, the same ratio on the generic kernel, "routed" or "forced": whether the library put the ratio
    on the matrix cores by its own rule or HIPFEAT_RESAMPLE_MFMA=1 did)"""
    routed, generic = pair(orig, new, monkeypatch)
    if routed.kernel_name == "resample_mfma":
        return routed, generic, "routed"
    monkeypatch.setenv("HIPFEAT_RESAMPLE_MFMA", "1")
    forced = A.HipResampleTensor(orig, new)
    monkeypatch.delenv("HIPFEAT_RESAMPLE_MFMA")
    return forced, generic, "forced"


def check_against_generic_and_oracle(mfma, generic, xs, orig, new):
    ys, gs = mfma.resample_batch(xs), generic.resample_batch(xs)
    assert len(ys) == len(gs) == len(xs)
    for x, y, g in zip(xs, ys, gs):
        assert y.numel() == g.numel() == R.resampled_length(len(x), mfma.orig, mfma.new)
        assert torch.equal(y, g), (len(x), float((y - g).abs().max()))
        if len(x):
            want = R.resample(x, orig, new, dtype=np.float64)
            err = float(np.abs(y.cpu().numpy() - want).max())
            assert err <= ABS_TOL, (len(x), err)
    # a cut resampled alone equals the same cut inside the batch (its workgroups do not see their neighbours)
    for i in (3, len(xs) - 1):
        assert torch.equal(mfma.resample_batch([xs[i]])[0], ys[i])


@pytest.mark.parametrize("orig,new", MFMA_RATES, ids=IDS)
def test_many_phase_ratios_run_on_the_matrix_core_kernel(orig, new, monkeypatch):
    routed, generic = pair(orig, new, monkeypatch)
    assert routed.kernel_name == "resample_mfma"
    assert generic.kernel_name == "resample_generic"


def test_other_ratios_keep_their_kernels(monkeypatch):
    assert A.HipResampleTensor(17600, 16000).kernel_name == "resample_fast<11,10,7>"
    assert A.HipResampleTensor(14400, 16000).kernel_name == "resample_fast<9,10,7>"
    assert A.HipResampleTensor(48000, 16000).kernel_name.startswith("resample_fast<3,1,")
    assert A.HipResampleTensor(8000, 16000).kernel_name.startswith("resample_fast<1,2,")
    assert A.HipResampleTensor(16000, 44100).kernel_name == "resample_generic"  # 160:441: an even hop stays on the generic kernel
    assert A.HipResampleTensor(16000, 22050).kernel_name == "resample_generic"
    monkeypatch.setenv("HIPFEAT_RESAMPLE_GENERIC", "1")
    assert A.HipResampleTensor(17600, 16000).kernel_name == "resample_generic"


@pytest.mark.parametrize("orig,new", MFMA_RATES, ids=IDS)
def test_mfma_equals_generic_and_both_meet_the_oracle_bar(orig, new, batches, monkeypatch):
    xs = batches[(orig, new)]
    routed, generic = pair(orig, new, monkeypatch)
    assert routed.kernel_name == "resample_mfma" and generic.kernel_name == "resample_generic"
    check_against_generic_and_oracle(routed, generic, xs, orig, new)


def test_the_instance_with_one_hop_tile_per_workgroup(batches, monkeypatch):
    """16000 -> 11025 = 640:441: a hop of 640 samples leaves room for ONE tile of 16 hops in 64 KiB of LDS -- resample_mfma_kernel<1>,
    which none of the routed ratios instantiates (hop tiles 2, 2, 2, 4).  The hop is even, so the switch puts it there.  28 phase
    tiles, the last one with 9 of its 16 phases (the `ph < nw` guard), 42 trips of the tap loop."""
    orig, new = RATES.ONE_HOP_TILE
    mfma, generic, how = mfma_pair(orig, new, monkeypatch)
    assert how == "forced" and mfma.kernel_name == "resample_mfma" and generic.kernel_name == "resample_generic"
    assert (mfma.orig, mfma.new, mfma.kernel.shape[1]) == (640, 441, 658) and hops_per_workgroup(640, 658) == 16
    check_against_generic_and_oracle(mfma, generic, batches[(orig, new)], orig, new)


@pytest.mark.parametrize("rates,reduced,tiles", [(RATES.ONE_PHASE_TILE, (49, 16), 1), (RATES.FOUR_PHASE_TILES, (147, 64), 4)], ids=["49:16", "147:64"])
def test_no_more_phase_tiles_than_waves(rates, reduced, tiles, batches, monkeypatch):
    """49:16: ONE phase tile, so waves 1-3 of every workgroup find no work behind the staging barrier; 147:64: exactly one tile per wave.
    Both have an odd hop and at least 16 phases: the library's own rule routes them (printed: which of the two happened)."""
    orig, new = rates
    mfma, generic, how = mfma_pair(orig, new, monkeypatch)
    print(f"{reduced[0]}:{reduced[1]} runs on {mfma.kernel_name} ({how})")
    assert mfma.kernel_name == "resample_mfma" and generic.kernel_name == "resample_generic"
    assert (mfma.orig, mfma.new) == reduced and -(-mfma.new // 16) == tiles
    check_against_generic_and_oracle(mfma, generic, batches[(orig, new)], orig, new)


def test_forced_onto_an_even_hop_it_still_equals_generic(monkeypatch):
    """160:441 stays on the generic kernel by the routing rule; HIPFEAT_RESAMPLE_MFMA=1 (the switch tools/bench_resample_rates.py times it
    with) puts it on the matrix-core kernel, where the same contract holds."""
    assert RATES.EVEN_HOP == (16000, 44100)
    monkeypatch.setenv("HIPFEAT_RESAMPLE_MFMA", "1")
    forced = A.HipResampleTensor(16000, 44100)
    fast = A.HipResampleTensor(17600, 16000)
    monkeypatch.delenv("HIPFEAT_RESAMPLE_MFMA")
    assert forced.kernel_name == "resample_mfma" and fast.kernel_name == "resample_fast<11,10,7>"
    generic = A.HipResampleTensor(16000, 44100)
    assert generic.kernel_name == "resample_generic"
    rng = np.random.RandomState(4)
    xs = [(rng.rand(n).astype(np.float32) - 0.5) for n in (1, 159, 160, 161, 5119, 5120, 5121, 30011, 0)]
    for x, y, g in zip(xs, forced.resample_batch(xs), generic.resample_batch(xs)):
        assert y.numel() == R.resampled_length(len(x), 160, 441) and torch.equal(y, g), len(x)


@pytest.mark.parametrize("orig,new", [(44100, 16000), (11025, 16000), RATES.ONE_HOP_TILE], ids=["441:160", "441:640", "640:441"])
def test_in_place_arena_form(orig, new, batches, monkeypatch):
    """d_in == d_out: the cuts in the front of one buffer, the outputs behind all of them, as perturb_speed_in_arena calls it."""
    xs = [x for x in batches[(orig, new)] if len(x)]
    routed, generic, how = mfma_pair(orig, new, monkeypatch)
    assert routed.kernel_name == "resample_mfma" and how == ("forced" if (orig, new) == RATES.ONE_HOP_TILE else "routed")
    lens = np.array([len(x) for x in xs], dtype=np.int64)
    offs = np.zeros(len(xs), dtype=np.int64)
    np.cumsum(((lens + 3) & ~3)[:-1], out=offs[1:])
    tail = int(offs[-1] + lens[-1] + 3) & ~3
    out_lens = routed.output_lengths(lens)
    out_offs = np.zeros(len(xs), dtype=np.int64)
    np.cumsum(((out_lens + 3) & ~3)[:-1], out=out_offs[1:])
    out_offs += tail
    total = int(out_offs[-1] + out_lens[-1])
    host = np.full(total, np.nan, dtype=np.float32)
    for x, o in zip(xs, offs):
        host[o : o + len(x)] = x
    arena = torch.from_numpy(host).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    routed.lib.check("hipfeat_resample", routed.handle, arena.data_ptr(), _lib.addr(offs), _lib.addr(lens), len(xs), arena.data_ptr(),
                     _lib.addr(out_offs), int(stream))
    got = arena.cpu()
    assert np.array_equal(got[:tail].numpy().view(np.uint32), host[:tail].view(np.uint32))  # the inputs are untouched
    for x, o, n, g in zip(xs, out_offs, out_lens, generic.resample_batch(xs)):
        assert torch.equal(got[o : o + n], g.cpu()), len(x)
