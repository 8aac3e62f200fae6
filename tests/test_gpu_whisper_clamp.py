"""GPU: the per-cut normalisation of the Whisper front end, one test per code path.

whisper3_kernel (kernel_whisper3.hpp, section 6) clamps the row blocks that hold something under cut_max - 8 through an 8-wide
sweep, a one-vector remainder loop, a scalar tail, or -- rows wider than the feature dimension, a row block off a 16-byte boundary
-- an element-wise sweep; whisper_norm_kernel (kernel_generic.hpp; behind HIPFEAT_WHISPER_VARIANT=2 and HIPFEAT_FORCE_GENERIC=1)
keeps short cuts in registers, reads long ones twice, and has its own strided branch and scalar tails.  Which path a launch takes
follows from the layout's frames per workgroup, which the ABI does not tell: every test works it out from tests/_layout_rounds.py
(held to layout_rounds.hpp by tests/test_layout_rounds.py) and ASSERTS the geometry it is meant for.  The inputs are those of
tests/_whisper_cases.py, whose purposes tests/test_whisper_cases.py proves on the CPU.

Every output is judged against the float64 oracle with the bar of tests/test_gpu_whisper.py (max(1e-4, 3 x the float32 oracle's
own distance)), lands in a NaN-filled buffer (fmaxf(NaN, c) = c: a sweep that strays writes a NUMBER), and is checked exactly for
  * the zero padding row, NaN everywhere outside the cuts' rows and columns,
  * max - min over the valid rows = 2 to 2^-20 where the clamp acts (the roundings of (cmax - 8) + 4 and cmax + 4 on |values| < 32
    add up to 2^-19, that is 2^-21 after the x 0.25; the bar is twice that), min >= max - 2 - 2^-20 always,
  * a cut inside a batch = the same cut alone, bit for bit."""
import os

import numpy as np
import pytest
import torch

import _layout_rounds as R
import _whisper_cases as WC
import lhotse_amd as LA
from lhotse_amd import _lib
from oracle import whisper_ref as W
from test_gpu_whisper import _close

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -20
GUARD = 4  # NaN rows in front of and behind the cuts (4 rows of any width are a multiple of 16 bytes)
ROUTES = {"auto": ({}, "whisper"), "w3": ({}, "whisper3_kernel"), "w2": ({"HIPFEAT_WHISPER_VARIANT": "2"}, "whisper_kernel2"), "generic": ({"HIPFEAT_FORCE_GENERIC": "1"}, "generic")}
_EX = {}
_ALONE = {}


def extractor(n_mels, route="w3"):
    if (n_mels, route) not in _EX:
        env, want = ROUTES[route]
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            ex = LA.HipWhisperFbank(LA.HipWhisperFbankConfig(num_filters=n_mels))
            name = ex.kernel_name  # (plans are created lazily: touch it while the switch is set)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        assert want in name, (n_mels, route, name)
        _EX[(n_mels, route)] = ex
    return _EX[(n_mels, route)]


def sig(key):
    return WC.signal(key) if isinstance(key, str) else WC.noise(*key)


def run(ex, keys, stride=None, starts=None, layout=False, d_wave=None, lens=None):
    """The cuts `keys`, packed back to back, through the C ABI into a NaN-filled (rows, stride) buffer; cut b starts at row starts[b]
    (default: packed behind GUARD rows).  Checks that nothing but the cuts' rows x M was written and returns the cuts' row slices."""
    M = ex.num_filters
    stride = stride or M
    if lens is None:
        xs = [sig(k) for k in keys]
        lens = _lib.i64([len(x) for x in xs])
        d_wave = torch.from_numpy(np.concatenate(xs)).cuda()
    offs = _lib.i64(np.concatenate([[0], np.cumsum(lens)[:-1]]))
    rows = (lens + 80) // 160
    if starts is None:
        starts = GUARD + np.concatenate([[0], np.cumsum(rows)[:-1]])
    starts = _lib.i64(starts)
    total = int((starts + rows).max()) + GUARD
    buf = torch.full((total, stride), float("nan"), device="cuda")
    plan, L = ex.plan, ex.plan.lib
    stream = torch.cuda.current_stream().cuda_stream
    if layout:
        h = np.zeros(1, dtype=np.uint64)
        L.check("hipfeat_layout_create", plan.handle, len(lens), _lib.addr(offs), _lib.addr(lens), None, _lib.addr(starts), stride, None, _lib.addr(h))
        L.check("hipfeat_extract_layout", plan.handle, int(h[0]), d_wave.data_ptr(), buf.data_ptr(), stream)
        torch.cuda.synchronize()
        L.check("hipfeat_layout_destroy", int(h[0]))
    else:
        L.check("hipfeat_extract", plan.handle, d_wave.data_ptr(), _lib.addr(offs), _lib.addr(lens), None, len(lens), buf.data_ptr(), _lib.addr(starts), stride, stream)
        torch.cuda.synchronize()
    covered = torch.zeros(total, dtype=torch.bool)
    for s, r in zip(starts.tolist(), rows.tolist()):
        assert not covered[s : s + r].any()
        covered[s : s + r] = True
    covered = covered.cuda()
    assert torch.isnan(buf[~covered]).all(), "rows outside the cuts were written"
    assert stride == M or torch.isnan(buf[:, M:]).all(), "columns beyond the feature dimension were written"
    assert not torch.isnan(buf[covered][:, :M]).any(), "rows of a cut were left unwritten"
    run.last = (buf, starts, rows)
    return [buf[s : s + r, :M] for s, r in zip(starts.tolist(), rows.tolist())]


def check(got, key, n_mels, ctx, acts):
    """one cut's rows against the oracles + the exact properties; prints the achieved error next to its bar"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    truth, ref32 = WC.reference(key, n_mels)
    n = len(sig(key))
    valid, rows = n // 160, W.num_rows(n)
    assert got.shape == (rows, n_mels) and got.dtype == np.float32, ctx
    assert rows == valid or (rows == valid + 1 and np.all(got[valid:] == 0.0)), (ctx, "the padding row is not zero")
    mx, mn = float(got[:valid].max()), float(got[:valid].min())
    assert mn >= mx - 2.0 - EPS, (ctx, mx, mn)
    if acts:
        assert abs((mx - mn) - 2.0) <= EPS, (ctx, mx, mn, (mx - mn) - 2.0)
    err, floor = float(np.abs(got - truth).max()), float(np.abs(ref32 - truth).max())
    print(f"[clamp] {ctx}: err {err:.3g} bar {max(1e-4, 3 * floor):.3g} (max - min) - 2 = {(mx - mn) - 2.0:.3g}")
    _close(got, ref32, truth, ctx)


def alone(ex, route, key):
    """the cut run alone (one launch of one cut; whisper3: 64 frames per workgroup), checked once and kept for the bit-for-bit comparisons"""
    k = (ex.num_filters, route, key)
    if k not in _ALONE:
        out = run(ex, [key])[0].cpu().numpy()
        acts = WC.CASES[key].acts if isinstance(key, str) else False
        check(out, key, ex.num_filters, ("alone", route, ex.num_filters, key), acts)
        _ALONE[k] = out
    return _ALONE[k]


def w3_fpw(ex, lens):
    return R.whisper3_frames_per_workgroup([W.num_rows(int(n)) for n in lens], ex.kernel_name)


def block_float4(case, fpw, n_mels):
    """float4 per row block that section 6 sweeps (the valid rows of the block)"""
    return [(min(f0 + fpw, case.frames) - f0) * n_mels // 4 for f0 in range(0, case.frames, fpw)]


# ---- whisper3: the sweep routes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [80, 128])
def test_w3_eight_wide_sweep_and_remainder(n_mels):
    """256 x blocks/CU cuts of 1100 frames fill every workgroup slot several times over, so the layout takes long workgroups (12
    rounds = 384 frames expected): a listed row block holds more than 7 x 512 float4 and enters the 8-wide loop, then the remainder."""
    ex = extractor(n_mels)
    assert ex.kernel_name.startswith("whisper3_kernel<%d>" % (2 if n_mels == 80 else 3))
    names = ["mid", "tail", "head", "spots"]
    B = 256 * R.blocks_per_cu(ex.kernel_name)
    S = WC.CASES["mid"].num_samples
    assert all(WC.CASES[n].num_samples == S for n in names)
    lens = _lib.i64([S] * B)
    fpw = w3_fpw(ex, lens)
    assert fpw * n_mels > 14336, (fpw, "the layout does not reach the 8-wide loop")
    seen, all_swept = set(), []
    for n in names:
        classes = WC.classify(WC.raw_log_mel(WC.signal(n), n_mels), fpw)
        f4 = block_float4(WC.CASES[n], fpw, n_mels)
        swept = [(c, q) for c, q in zip(classes, f4) if c != "n"]
        assert swept and all(q > 3584 for c, q in swept), (n, classes, f4)
        all_swept += [q for c, q in swept]
        seen |= set(classes)
        print(f"[clamp] 8-wide M={n_mels} {ex.kernel_name.split(' ')[-2]} rounds {fpw // 32} case {n}: blocks {classes} float4 {f4}")
    assert seen == {"n", "p", "a"} and any(q % 4096 for q in all_swept)  # ... and some block leaves work to the one-vector remainder loop
    d_wave = torch.from_numpy(np.concatenate([WC.signal(n) for n in names])).cuda().repeat(B // len(names))
    outs = run(ex, None, d_wave=d_wave, lens=lens)
    buf, starts, rows = run.last
    for i, n in enumerate(names):
        check(outs[i], n, n_mels, ("8-wide", n_mels, n), True)
        assert np.array_equal(outs[i].cpu().numpy(), alone(ex, "w3", n)), (n, "differs from the cut run alone")
    per = int(rows[0]) * len(names)
    tiled = buf[GUARD : GUARD + B * int(rows[0])].view(B // len(names), per, n_mels)
    assert torch.equal(tiled, tiled[:1].expand_as(tiled)), "a repeated cut differs from its first copy"


def test_w3_remainder_only_with_a_partial_last_block():
    """One cut: 2 rounds = 64 frames per workgroup (1280 float4: the 8-wide loop is never entered); the last row block of `tail` holds
    12 valid frames, all under the clamp."""
    ex = extractor(80)
    for n in ["tail", "mid", "head", "spots"]:
        c = WC.CASES[n]
        assert w3_fpw(ex, [c.num_samples]) == 64
        classes = dict(c.blocks)[64]
        assert max(block_float4(c, 64, 80)) <= 3584 and len(classes) == len(block_float4(c, 64, 80))
        alone(ex, "w3", n)
    assert 1 <= WC.CASES["tail"].frames % 64 <= 63 and dict(WC.CASES["tail"].blocks)[64][-1] == "a"
    assert dict(WC.CASES["head"].blocks)[64][0] == "a"


@pytest.mark.parametrize("n_mels", [81, 127])
def test_w3_dense_scalar_tail(n_mels):
    """Odd filter count, first cut of the buffer: every row block starts on a 16-byte boundary (64 x M floats), the last one -- 13 valid
    frames, listed -- is no whole number of float4 and ends in the scalar tail."""
    ex = extractor(n_mels)
    assert ex.kernel_name.startswith("whisper3_kernel"), ex.kernel_name
    c = WC.CASES["tail_odd"]
    assert w3_fpw(ex, [c.num_samples]) == 64 and dict(c.blocks)[64][-1] == "a"
    last = (c.frames % 64) * n_mels
    assert c.frames % 4 != 0 and last % 4 != 0
    out = alone(ex, "w3", "tail_odd")
    buf, starts, _ = run.last
    assert (buf.data_ptr() + 4 * int(starts[0]) * n_mels) % 16 == 0 and (64 * n_mels * 4) % 16 == 0
    assert out.shape == (c.rows, n_mels)
    print(f"[clamp] scalar tail M={n_mels}: last block {c.frames % 64} frames = {last // 4} float4 + {last % 4} floats")


def test_w3_elementwise_by_misaligned_base():
    """81 filters, a layout with explicit output rows, both cuts at ODD rows: 81 x odd floats are never a multiple of 4, and the row
    blocks (64 x 81 floats apart) inherit the misalignment -- the dense test fails on the address alone (the row stride equals M)."""
    ex = extractor(81)
    keys = ["loud", "tail_odd"]
    rows = [WC.CASES[k].rows for k in keys]
    starts = [GUARD + 1, GUARD + 1 + rows[0] + 1]  # (one NaN row between the cuts)
    assert all(s % 2 == 1 for s in starts) and w3_fpw(ex, [WC.CASES[k].num_samples for k in keys]) == 64
    outs = run(ex, keys, starts=starts, layout=True)
    buf = run.last[0]
    assert all((buf.data_ptr() + 4 * (s + 64 * j) * 81) % 16 != 0 for s in starts for j in range(18))
    for k, o in zip(keys, outs):
        check(o, k, 81, ("misaligned base", k), True)
        assert np.array_equal(o.cpu().numpy(), alone(ex, "w3", k)), k


@pytest.mark.parametrize("layout", [False, True], ids=["extract", "layout"])
@pytest.mark.parametrize("n_mels,stride,key", [(80, 96, "mid"), (81, 84, "tail_odd")])
def test_w3_elementwise_by_stride(n_mels, stride, key, layout):
    ex = extractor(n_mels)
    keys = [key, "loud"]
    assert w3_fpw(ex, [WC.CASES[k].num_samples for k in keys]) == 64
    for k, o in zip(keys, run(ex, keys, stride=stride, layout=layout)):
        check(o, k, n_mels, ("stride", n_mels, stride, k, layout), True)
        assert np.array_equal(o.cpu().numpy(), alone(ex, "w3", k)), k


# ---- whisper_norm_kernel (whisper2 and generic routes) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["w2", "generic"])
def test_norm_kernel_register_two_read_and_strided_routes(route):
    small, big = extractor(80, route), extractor(128, route)
    c = WC.CASES["mid"]
    assert c.frames * 80 // 4 <= 24576 < c.frames * 128 // 4  # kKeep x 1024 float4 stay in registers
    a80 = alone(small, route, "mid")    # held in registers
    a128 = alone(big, route, "mid")     # dense, two reads
    for k, o in zip(["mid", "loud"], run(small, ["mid", "loud"], stride=96)):  # strided
        check(o, k, 80, ("norm strided", route, k), True)
        assert np.array_equal(o.cpu().numpy(), alone(small, route, k)), k
    # the same arithmetic in another summation order: the fused kernel against the two-pass routes
    for m, a in ((80, a80), (128, a128)):
        d = float(np.abs(alone(extractor(m), "w3", "mid") - a).max())
        print(f"[clamp] whisper3 vs {route} M={m}: {d:.3g} (bar 1e-5)")
        assert d <= 1e-5, (route, m, d)


def test_norm_kernel_odd_filter_count():
    """23 filters fall to whisper2 (no matrix-core schedule): both scalar tails of whisper_norm_kernel (cut held in registers, cut read
    twice) and, for a second cut whose rows start off a 16-byte boundary, its element-wise branch."""
    assert extractor(23, "auto").kernel_name.startswith("whisper_kernel2"), extractor(23, "auto").kernel_name
    ex = extractor(23, "w2")
    short, long_ = WC.CASES["tail_odd"], WC.CASES["long_odd"]
    assert short.frames * 23 % 4 != 0 and short.frames * 23 // 4 <= 24576
    assert long_.frames * 23 % 4 != 0 and long_.frames * 23 // 4 > 24576
    a = alone(ex, "w2", "tail_odd")
    alone(ex, "w2", "long_odd")
    outs = run(ex, ["tail_odd", "tail_odd"])
    buf, starts, _ = run.last
    assert (buf.data_ptr() + 4 * int(starts[0]) * 23) % 16 == 0 and (buf.data_ptr() + 4 * int(starts[1]) * 23) % 16 != 0
    for o in outs:
        assert np.array_equal(o.cpu().numpy(), a)


# ---- semantics, on every route ---------------------------------------------------------------------------------------------------------------
SEM = [("w3", 80), ("w3", 128), ("w3", 81), ("w2", 80), ("generic", 80)]


@pytest.mark.parametrize("route,n_mels", SEM)
def test_dropped_last_column_does_not_count_for_the_maximum(route, n_mels):
    """The burst behind the last kept frame raises the dropped column 6 decades over the cut: counted, it would clamp 53 % of the
    elements by up to 1.2; the correct maximum clamps nothing."""
    alone(extractor(n_mels, route), route, "dropped")


@pytest.mark.parametrize("route,n_mels", SEM)
def test_loud_cut_alone_and_collated(route, n_mels):
    """Clamp level c = 1.35 > 0: the padding row stays 0 and the fill rows of a collated batch stay LOG_EPSILON."""
    ex = extractor(n_mels, route)
    a = alone(ex, route, "loud")
    longer = (300 * 160 + 100, 0.5, 21)
    col, lens = ex.extract_collated([WC.signal("loud"), WC.noise(*longer)], 16000)
    T = WC.CASES["loud"].rows
    assert col.shape == (2, 301, n_mels) and lens.tolist() == [T, 301]
    got = col.cpu().numpy()
    assert np.array_equal(got[0, :T], a) and np.all(got[0, T - 1] == 0.0)
    assert np.all(got[0, T:] == np.float32(LA.compat.LOG_EPSILON)), "the fill rows of the collated batch were touched"
    check(got[1], longer, n_mels, ("collated neighbour", route, n_mels), False)


@pytest.mark.parametrize("route,n_mels", [("w3", 80), ("w3", 81), ("w2", 80), ("generic", 80)])
def test_workgroup_that_holds_only_the_padding_row(route, n_mels):
    ex = extractor(n_mels, route)
    c = WC.CASES["pad_only"]
    assert c.frames % 64 == 0 and c.rows == c.frames + 1
    if route == "w3":  # the third workgroup publishes max = -inf, min = +inf
        assert w3_fpw(ex, [c.num_samples]) == 64
    alone(ex, route, "pad_only")


@pytest.mark.parametrize("route,n_mels", [("w3", 80), ("w3", 128), ("w2", 80), ("generic", 80)])
def test_staging_boundary_lengths_between_loud_neighbours(route, n_mels):
    """S = 160 x 4k + 680 is the first length at which the wave that starts at frame 4k stages its span by LDS-DMA; one sample less
    and it reflects at the cut's end.  Neighbours 5 decades louder sit directly in front of and behind every cut in the buffer."""
    ex = extractor(n_mels, route)
    loud = (2000, 3e4, 31)
    keys = [loud]
    for k in (1, 17):
        for j, s in enumerate(WC.boundary_lengths(k)):
            keys += [(s, 0.5, 40 + 3 * k + j), loud]
    outs = run(ex, keys)
    for key, o in zip(keys, outs):
        if key is not loud:
            check(o, key, n_mels, ("boundary", route, n_mels, key[0]), False)
        assert np.array_equal(o.cpu().numpy(), alone(ex, route, key)), key


# ---- repeats ---------------------------------------------------------------------------------------------------------------------------
def test_w3_repeated_launches_of_a_layout_in_which_the_clamp_acts():
    """9 launches (the layout has kNormSlots = 4 scratch copies) alternately on two streams, every output NaN-filled before."""
    ex = extractor(80)
    plan, L = ex.plan, ex.plan.lib
    keys = ["mid", "loud", "pad_only", "head"]
    xs = [WC.signal(k) for k in keys]
    lens = _lib.i64([len(x) for x in xs])
    assert w3_fpw(ex, lens) == 64  # 2 rounds: `mid` alone spans 18 workgroups, 9 of them listed
    offs = _lib.i64(np.concatenate([[0], np.cumsum(lens)[:-1]]))
    rows = (lens + 80) // 160
    d_wave = torch.from_numpy(np.concatenate(xs)).cuda()
    h = np.zeros(1, dtype=np.uint64)
    L.check("hipfeat_layout_create", plan.handle, len(lens), _lib.addr(offs), _lib.addr(lens), None, None, 80, None, _lib.addr(h))
    outs = [torch.full((int(rows.sum()), 80), float("nan"), device="cuda") for _ in range(9)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        L.check("hipfeat_extract_layout", plan.handle, int(h[0]), d_wave.data_ptr(), o.data_ptr(), (s1 if i % 2 == 0 else s2).cuda_stream)
    torch.cuda.synchronize()
    L.check("hipfeat_layout_destroy", int(h[0]))
    first = outs[0].cpu().numpy()
    assert np.array_equal(first, np.concatenate([alone(ex, "w3", k) for k in keys]))
    for i, o in enumerate(outs[1:]):
        np.testing.assert_array_equal(o.cpu().numpy(), first, err_msg=f"launch {i + 1}")
