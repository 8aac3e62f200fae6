"""GPU: the sinc resampler without a filter bank (sinc_kernel through ``hipfeat_sinc_*``) against the banded float64 truth of
tests/_sinc_ref.py, which tests/test_sinc_tables.py pins against the oracle.

Bars.  Weights: the device evaluates the reference's formula in float64 and rounds once to float32, as numpy does in ``_sinc_ref``; two
correctly working float64 libms give the same float32 but for rounding ties (a share of about 1e-8), so a weight may differ by at most
1 ulp and at most 1e-4 of a ratio's non-zero weights may differ at all (any float32 intermediate would make about half of them differ).
Outputs: max_abs <= 1e-5 for |x| <= 0.5, the bar of tests/test_gpu_resample.py (``ABS_TOL``): only the float32 summation differs."""
import numpy as np
import pytest
import torch

import _sinc_ref as SR
from lhotse_amd import _lib, augmentation as A

pytestmark = pytest.mark.gpu
ABS_TOL = 1e-5
LENS = [0, 1, 2, 37, 255, 256, 257, 4673, 8000, 8001, 16000, 52345]
WEIGHT_RATES = [(16000, 9346), (9346, 16000), (16000, 7002), (16000, 15998), (48000, 7000), (44100, 16000)]
RATES = WEIGHT_RATES + [(7, 16)]
FILL = 777.0
_FILTERS, _WEIGHT_DIFF = {}, {}


def filt(rates):
    if rates not in _FILTERS:
        _FILTERS[rates] = SR.window(*rates)
    return _FILTERS[rates]


def ulps_apart(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def weight_diff(rates):
    """-> (non-zero weights of the ratio, how many the device rounds otherwise than numpy, the largest distance in ulp); cached"""
    if rates not in _WEIGHT_DIFF:
        first, want, width, orig, new = filt(rates)
        w, f, wd = A.get_or_create_sinc().weights(*rates)
        torch.cuda.synchronize()
        assert wd == width and tuple(w.shape) == (new, 2 * width + 2) and np.array_equal(f.cpu().numpy(), first)
        apart = ulps_apart(w.cpu().numpy(), want.astype(np.float32))
        _WEIGHT_DIFF[rates] = (int((want != 0).sum()), int((apart > 0).sum()), int(apart.max()))
    return _WEIGHT_DIFF[rates]


@pytest.fixture(scope="module")
def signals():
    rng = np.random.RandomState(11)
    return [(rng.rand(n).astype(np.float32) - np.float32(0.5)) for n in LENS]


@pytest.fixture(scope="module")
def truth(signals):
    """float64 truth of every (ratio, row), computed once"""
    return {r: [SR.resample(x, *r, filt=filt(r)) for x in signals] for r in RATES}


def launch(rows, sinc=None):
    """rows: [(samples, (src, dst))] -> (outputs, info): all rows in ONE launch of one arena; inputs at offsets of every alignment, outputs
    behind them, everything else must keep FILL."""
    sinc = sinc or A.get_or_create_sinc()
    in_off, pos = [], 5
    for k, (x, _) in enumerate(rows):
        pos += (k % 4 - pos) % 4  # offsets modulo 4: 0, 1, 2, 3, 0, ...
        in_off.append(pos)
        pos += len(x) + 3
    out_len = [SR.resampled_length(len(x), *SR.geometry(*r)[:2]) for x, r in rows]
    out_off = []
    for k, n in enumerate(out_len):
        pos += ((k + 1) % 4 - pos) % 4
        out_off.append(pos)
        pos += n + 3
    host = np.full(pos + 64, FILL, dtype=np.float32)
    for o, (x, _) in zip(in_off, rows):
        host[o : o + len(x)] = x
    arena = torch.from_numpy(host).cuda()
    ticket, planned, info = sinc.plan(in_off, [len(x) for x, _ in rows], [r for _, r in rows], out_off, arena.numel())
    assert planned.tolist() == out_len and info[1] <= arena.numel()
    sinc.run(ticket, arena)
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    outs = [got[o : o + n].copy() for o, n in zip(out_off, out_len)]
    for o, n in zip(out_off, out_len):
        got[o : o + n] = host[o : o + n]
    assert np.array_equal(got, host), "something outside the output rows was written"
    return outs, info


@pytest.mark.parametrize("rates", WEIGHT_RATES, ids=["%d-%d" % r for r in WEIGHT_RATES])
def test_weights_are_the_float64_formula_rounded_once(rates):
    nonzero, differ, worst = weight_diff(rates)
    print(f"{rates[0]} -> {rates[1]}: {nonzero} non-zero weights, {differ} differ from numpy's float32, at most {worst} ulp")
    assert worst <= 1 and differ <= 1e-4 * nonzero


def test_outputs_of_one_launch_with_mixed_ratios(signals, truth):
    rows = [(x, r) for r in RATES for x in signals]
    outs, info = launch(rows)
    assert info[3] == 86  # the widest window of the launch: 48000 -> 7000
    worst = {}
    for (x, r), y, want in zip(rows, outs, [t for r in RATES for t in truth[r]]):
        assert y.shape == want.shape and y.dtype == np.float32
        if len(want):
            worst[r] = max(worst.get(r, 0.0), float(np.abs(y - want).max()))
    print({"%d-%d" % r: "%.2e" % v for r, v in worst.items()})
    assert max(worst.values()) <= ABS_TOL, worst


@pytest.mark.parametrize("rates", RATES, ids=["%d-%d" % r for r in RATES])
def test_outputs_with_one_ratio_alone_in_a_launch(signals, truth, rates):
    outs, _ = launch([(x, rates) for x in signals])
    for y, want in zip(outs, truth[rates]):
        assert y.shape == want.shape and (len(want) == 0 or np.abs(y - want).max() <= ABS_TOL)
    again, _ = launch([(x, rates) for x in signals])  # two runs give equal bits
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(outs, again))


def test_a_row_does_not_depend_on_its_neighbours_in_the_launch(signals):
    """the same rows alone, and among rows of other ratios at other offsets: equal bits"""
    mine = [(signals[-1], (16000, 9346)), (signals[7], (9346, 16000))]
    alone, _ = launch(mine)
    among, _ = launch([(signals[5], (48000, 7000)), mine[0], (signals[9], (7, 16)), mine[1], (signals[8], (44100, 16000))])
    assert np.array_equal(alone[0].view(np.uint32), among[1].view(np.uint32)) and np.array_equal(alone[1].view(np.uint32), among[3].view(np.uint32))


@pytest.mark.parametrize("rates", [(44100, 16000), (16000, 22050)], ids=["44100-16000", "16000-22050"])
def test_chain_contract_with_the_dense_resampler(signals, rates):
    """For identical weights the outputs are those of ``hipfeat_resample`` (the ascending-tap fmaf chain over the whole dense row), except
    for the sign of an exact zero."""
    dense = A.get_or_create_resampler(*rates)
    assert dense.kernel is not None and dense.kernel_name != "resample_sinc"
    want = [y.cpu().numpy() for y in dense.resample_batch(signals)]
    outs, _ = launch([(x, rates) for x in signals])
    nonzero, differ, _ = weight_diff(rates)
    print(f"{rates[0]} -> {rates[1]}: {differ} of {nonzero} weights differ -> the {'bit-for-bit' if differ == 0 else '1e-5'} case ran")
    for y, w in zip(outs, want):
        assert y.shape == w.shape
        if differ == 0:
            assert np.array_equal(y + np.float32(0), w + np.float32(0))  # (-0 + 0 = +0)
        elif len(w):
            assert np.abs(y.astype(np.float64) - w).max() <= ABS_TOL


def test_the_router_sends_large_banks_to_one_sinc_launch_and_leaves_the_others_alone(signals, truth, monkeypatch):
    small, big, big2 = (44100, 16000), (16000, 9346), (9346, 16000)
    assert A.resample_route(*small) == "bank" and A.resample_route(*big) == A.resample_route(*big2) == "sinc" and A.resample_route(48001, 6000) is None
    assert A.resample_route(48000, 6000) == "bank"  # 8:1, a bank of 106 floats: the window cap is the bankless kernel's alone
    xs = [signals[10], signals[11], signals[7], signals[9], signals[8], signals[3]]
    ratios = [small, big, None, big2, small, big]
    lens = np.array([len(x) for x in xs], dtype=np.int64)
    offs = np.zeros(len(xs), dtype=np.int64)
    np.cumsum(((lens + 3) & ~3)[:-1], out=offs[1:])
    front = int(offs[-1] + lens[-1])
    host = np.zeros(front + 3 + A.resampled_tail_floats(lens, ratios), dtype=np.float32)
    for o, x in zip(offs, xs):
        host[o : o + len(x)] = x
    lib = _lib.load()
    calls, check = [], lib.check
    monkeypatch.setattr(lib, "check", lambda name, *a: (calls.append(name), check(name, *a))[1])
    arena = torch.from_numpy(host).cuda()
    po, pl = A.resample_in_arena(arena, offs, lens, ratios, front)
    torch.cuda.synchronize()
    assert calls.count("hipfeat_sinc_run") == 1 and calls.count("hipfeat_sinc_plan") == 1 and calls.count("hipfeat_resample") == 1
    lo, ll, end = A.resample_layout(offs, lens, ratios, front)
    assert np.array_equal(po, lo) and np.array_equal(pl, ll) and end <= arena.numel() and po[2] == offs[2] and pl[2] == lens[2]
    got = arena.cpu().numpy()
    for i, r in enumerate(ratios):
        if r is not None:
            want = truth[r][LENS.index(len(xs[i]))]
            assert pl[i] == len(want) and np.abs(got[po[i] : po[i] + pl[i]] - want).max() <= ABS_TOL, (i, r)
    assert np.array_equal(got[:front], host[:front])  # the inputs are only read
    # the under-threshold rows: bit-equal to a call without the others
    calls.clear()
    only = [r if r == small else None for r in ratios]
    a2 = torch.from_numpy(host).cuda()
    p2, l2 = A.resample_in_arena(a2, offs, lens, only, front)
    torch.cuda.synchronize()
    assert "hipfeat_sinc_run" not in calls and calls.count("hipfeat_resample") == 1
    g2 = a2.cpu().numpy()
    for i in (0, 4):
        assert l2[i] == pl[i] and np.array_equal(g2[p2[i] : p2[i] + l2[i]].view(np.uint32), got[po[i] : po[i] + pl[i]].view(np.uint32))
    # sinc_in_arena: the same placement with every ratio on the bankless kernel, one launch
    calls.clear()
    a3 = torch.from_numpy(host).cuda()
    p3, l3 = A.sinc_in_arena(a3, offs, lens, ratios, front)
    torch.cuda.synchronize()
    assert calls.count("hipfeat_sinc_run") == 1 and "hipfeat_resample" not in calls and np.array_equal(p3, po) and np.array_equal(l3, pl)
    g3 = a3.cpu().numpy()
    for i in (1, 3, 5):
        assert np.array_equal(g3[p3[i] : p3[i] + l3[i]].view(np.uint32), got[po[i] : po[i] + pl[i]].view(np.uint32))
    for i in (0, 4):
        assert np.abs(g3[p3[i] : p3[i] + l3[i]] - truth[small][LENS.index(len(xs[i]))]).max() <= ABS_TOL
    with pytest.raises(ValueError, match="arena too small"):
        A.resample_in_arena(arena[: len(host) - 8], offs, lens, ratios, front)


def test_hip_resample_takes_the_bankless_kernel_for_a_large_bank(signals):
    fn = A.HipResample(11127, 16000)
    r = fn.resampler
    assert r.kernel_name == "resample_sinc" and r.kernel is None and (r.orig, r.new, r.width) == (11127, 16000, 7)
    assert A.get_or_create_resampler(11127, 16000) is r
    x = np.stack([signals[10], signals[10][::-1].copy()])
    y = fn(x, 11127)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (2, r.output_length(16000))
    f = SR.window(11127, 16000)
    for c in range(2):
        assert np.abs(y[c] - SR.resample(x[c], 11127, 16000, filt=f)).max() <= ABS_TOL
    yd = r(torch.from_numpy(x).cuda())
    assert yd.is_cuda and torch.equal(yd.cpu(), torch.from_numpy(y))
    ys = r.resample_batch([signals[3], signals[0], signals[6]])
    assert [int(t.numel()) for t in ys] == [r.output_length(n) for n in (37, 0, 257)]
    assert np.abs(ys[2].cpu().numpy() - SR.resample(signals[6], 11127, 16000, filt=f)).max() <= ABS_TOL
    small = A.get_or_create_resampler(17600, 16000)  # under the threshold: as before
    assert small.kernel is not None and small.kernel_name.startswith("resample_fast")
    with pytest.raises(_lib.HipFeatError, match="UNSUPPORTED"):
        A.HipResampleTensor(48001, 6000)


def test_plan_and_run_refusals_on_the_device(signals):
    sinc = A.HipSincResampler()
    try:
        def status(*a):
            with pytest.raises(_lib.HipFeatError) as e:
                sinc.plan(*a)
            return e.value.status, str(e.value)

        A_ = 1 << 20
        assert status([0], [16000], [(16000, 9346)], [15999], A_)[0] == _lib.ERR_INVALID  # output over its own input
        assert "overlaps the input" in status([0, 40000], [16000, 16000], [(16000, 9346)] * 2, [50000, 70000], A_)[1]
        assert "past the arena" in status([0], [16000], [(16000, 9346)], [16000], 25345)[1]
        assert "equal rates" in status([0], [16000], [(16000, 16000)], [16000], A_)[1]
        assert "positive" in status([0], [16000], [(0, 16000)], [16000], A_)[1]
        st, msg = status([0], [16000], [(48000, 6000)], [16000], A_)
        assert st == _lib.ERR_UNSUPPORTED and "window of 100 taps" in msg
        with pytest.raises(_lib.HipFeatError, match="UNSUPPORTED"):
            sinc.weights(48000, 6000)
        with pytest.raises(_lib.HipFeatError, match="INVALID"):
            sinc.weights(16000, 16000)
        arena = torch.zeros(16000 + 9346, device="cuda")
        arena[:16000] = torch.from_numpy(signals[10]).cuda()
        with pytest.raises(_lib.HipFeatError, match="not a planned resampling"):
            sinc.run(5, arena)
        ticket, _, info = sinc.plan([0], [16000], [(16000, 9346)], [16000], arena.numel())
        with pytest.raises(_lib.HipFeatError, match="arena holds"):
            sinc.run(ticket, arena[:-2])
        sinc.run(ticket, arena)  # the refused run left the ticket planned
        with pytest.raises(_lib.HipFeatError, match="not a planned resampling"):
            sinc.run(ticket, arena)  # a ticket runs once
        torch.cuda.synchronize()
        assert np.abs(arena[16000:].cpu().numpy() - SR.resample(signals[10], 16000, 9346)).max() <= ABS_TOL
        tickets = [sinc.plan([], [], [], [], 0)[0] for _ in range(16)]
        assert "16 planned resamplings are outstanding" in status([], [], [], [], 0)[1]
        for t in tickets:
            sinc.run(t, arena)  # plans of no rows: nothing is launched
        assert sinc.plan([], [], [], [], 0)[0] == tickets[-1] + 1
        sinc.run(tickets[-1] + 1, arena)
    finally:
        sinc.close()


def test_speed_factors_without_a_dense_bank_take_the_sinc_launch(signals, monkeypatch):
    """Speed(1.037) at 16 kHz is 16592 -> 16000 = 1037 : 1000, a bank of 1 051 000 floats: over the threshold, so no bank is built.  The
    speed path (``perturb_speed_in_arena``, ``HipSpeed``) serves it through the bankless kernel, in one launch with its like, next to the
    dense launches of 0.9 / 1.1; the mixed launch pair (``HipSpeedBank``) refuses it as it refuses every factor but 0.9 / 1.1."""
    sr = 16000
    assert A.resample_route(16592, sr) == A.resample_route(16656, sr) == "sinc" and A.resample_route(14400, sr) == "bank"
    xs = [signals[10], signals[8], signals[11], signals[9], signals[7]]
    factors = [1.037, 1.0, 0.9, 1.041, 1.037]
    lens = np.array([len(x) for x in xs], dtype=np.int64)
    offs = np.zeros(len(xs), dtype=np.int64)
    np.cumsum(((lens + 3) & ~3)[:-1], out=offs[1:])
    front = int(offs[-1] + lens[-1])
    host = np.zeros(front + 3 + A.perturbed_tail_floats(lens, factors, sr), dtype=np.float32)
    for o, x in zip(offs, xs):
        host[o : o + len(x)] = x
    lib = _lib.load()
    calls, check = [], lib.check
    monkeypatch.setattr(lib, "check", lambda name, *a: (calls.append(name), check(name, *a))[1])
    arena = torch.from_numpy(host).cuda()
    po, pl = A.perturb_speed_in_arena(arena, offs, lens, factors, sr, front)
    torch.cuda.synchronize()
    assert calls.count("hipfeat_sinc_run") == 1 and calls.count("hipfeat_resample") == 1
    lo, ll, _ = A.perturbed_layout(offs, lens, factors, sr, front)
    assert np.array_equal(po, lo) and np.array_equal(pl, ll)
    got = arena.cpu().numpy()
    for i, f in enumerate(factors):
        if f != 1.0:
            want = SR.resample(xs[i], round(sr * f), sr)  # (ceil(new * n / orig) samples: the sample or two over the cut's count come off later)
            assert pl[i] == len(want) >= A.perturb_num_samples(len(xs[i]), f) and np.abs(got[po[i] : po[i] + pl[i]] - want).max() <= ABS_TOL, (i, f)
    assert np.array_equal(got[:front], host[:front])
    y = A.HipSpeed(1.037)(signals[10][None, :], sr)
    assert y.dtype == np.float32 and np.array_equal(y[0], got[po[0] : po[0] + pl[0]])
    with pytest.raises(_lib.HipFeatError, match="UNSUPPORTED"):
        A.HipSpeedBank([1.037], sr)


def test_the_route_rule_states_what_the_dense_kernels_take():
    """``resample_route`` says "bank" exactly where ``hipfeat_resampler_create`` accepts the bank (small banks, built here)."""
    from lhotse_amd import constants as C

    lib = _lib.load()
    for src, dst in ((16000, 202), (16000, 404), (16000, 1000), (44100, 16000), (16000, 22050), (3001, 32), (16001, 8), (1000, 16000)):
        kernel, width, orig, new = C.sinc_resample_kernel(src, dst)
        assert kernel.size <= A.MAX_RESAMPLE_BANK_FLOATS
        out = np.zeros(1, dtype=np.uint64)
        st = lib.raw("hipfeat_resampler_create", orig, new, width, _lib.addr(kernel), 0, _lib.addr(out))
        assert st in (0, _lib.ERR_UNSUPPORTED) and (st == 0) == A._dense_kernel_fits(orig, new, width) == (A.resample_route(src, dst) == "bank"), (src, dst, st)
        if st == 0:
            lib.raw("hipfeat_resampler_destroy", int(out[0]))
    assert A.resample_route(16000, 202) is None and A.resample_route(16001, 8) is None  # neither kernel: such cuts are left to lhotse
