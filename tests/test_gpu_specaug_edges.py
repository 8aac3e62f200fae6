"""GPU: specaug_warp_kernel<1|4>, specaug_mask_kernel and global_mvn_kernel at their edge shapes (cases: tests/_specaug_cases.py, whose
geometry and reference are pinned on the CPU by tests/test_specaug_edges_reference.py).

The specaug cases go through hipfeat_specaug itself, so that base offsets, guard bands and out-of-range masks are possible: ``out`` is a
slice of a buffer filled with the bit pattern 0x5A5A5A5A, at least 64 floats of it on either side, and after every run both guards still
hold the pattern and the input its bits.  Against oracle.specaug_ref.apply (the float32 restatement of the reference's arithmetic):

  * elements in no segment and no mask are the input's bits;
  * elements in a segment and no mask are within 2e-5 (the bar of tests/test_gpu_specaug.py: the data has the goldens' scale);
  * the masked elements of one sequence all hold the same bits, within 2e-5 of the oracle's mean of the warped sequence;
  * a second run of the same call returns the same bits.

Where a case's data is at another level than the goldens' (|x| up to ~20) the bar is 2e-5 * max|x| / 10; those cases say so.
GlobalMVN is held to torch's two CPU ops bit for bit, NaNs position for position."""
import numpy as np
import pytest
import torch

import _specaug_cases as C
import lhotse_amd as LA
from lhotse_amd import _lib
from lhotse_amd.signal_transforms import apply_specaug
from oracle import specaug_ref as R
from oracle.make_golden_specaug import seed_all

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A
GUARD = 64
BAR = 2e-5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _upload(x, off):
    """x on the device, ``off`` floats behind a 16-byte boundary."""
    base = torch.empty(x.size + 8, dtype=torch.float32, device="cuda")
    assert base.data_ptr() % 16 == 0
    view = base[off : off + x.size]
    view.copy_(torch.from_numpy(x.reshape(-1)))
    return view


def _poisoned(n, off):
    buf = torch.full((GUARD + off + n + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    lo = GUARD + off
    return buf, buf[lo : lo + n], lo


def _call(lib, xin, out, shape, segs, masks, stream):
    B, T, F = shape
    segs, masks = np.ascontiguousarray(segs), np.ascontiguousarray(masks)
    lib.check("hipfeat_specaug", xin.data_ptr(), out.data_ptr(), B, T, F, _lib.addr(segs) if len(segs) else None, len(segs),
              _lib.addr(masks) if len(masks) else None, len(masks), stream)


def _collect(x, xin, buf, lo):
    """After the stream is idle: the output, once the guards and the input are seen to be intact."""
    host = buf.cpu().numpy()
    n = x.size
    assert (host[:lo] == PATTERN).all(), "a store in front of out"
    assert (host[lo + n :] == PATTERN).all(), "a store behind out"
    assert np.array_equal(bits(xin.cpu().numpy()), bits(x).reshape(-1)), "the input changed"
    return host[lo : lo + n].view(np.float32).reshape(x.shape)


def run(x, segs, masks, in_off=0, out_off=0):
    xin = _upload(x, in_off)
    buf, out, lo = _poisoned(x.size, out_off)
    assert xin.data_ptr() % 16 == 4 * in_off and out.data_ptr() % 16 == 4 * out_off
    _call(_lib.load(), xin, out, x.shape, segs, masks, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return _collect(x, xin, buf, lo)


def judge(name, x, seg_rounds, masks, got, bar=BAR):
    want = R.apply(x, seg_rounds, masks)
    in_seg, masked = C.regions(x, seg_rounds, masks)
    in_seg = np.broadcast_to(in_seg[:, :, None], x.shape)
    copied = ~in_seg & ~masked
    assert np.array_equal(bits(got)[copied], bits(x)[copied]), (name, "a copied element changed", int((bits(got) != bits(x))[copied].sum()))
    warped = in_seg & ~masked
    if warped.any():
        err = float(np.abs(got - want)[warped].max())
        print(f"{name}: warp max abs error {err:.3e} (bar {bar:.1e})")
        assert err <= bar, (name, err)
    for b in range(x.shape[0]):
        if masked[b].any():
            fill = got[b][masked[b]]
            assert (bits(fill) == bits(fill)[0]).all(), (name, b, "the masked elements differ among themselves")
            mean = want[b][masked[b]][0]
            print(f"{name}: sequence {b} mean {fill[0]!r} oracle {mean!r} (bar {bar:.1e})")
            assert abs(float(fill[0]) - float(mean)) <= bar, (name, b, float(fill[0]), float(mean))
    return want


def check_case(case, bar=BAR, in_off=0, out_off=0):
    name, x, seg_rounds, masks, claims = case
    assert len(seg_rounds) == 1
    got = run(x, seg_rounds[0], masks, in_off, out_off)
    judge(name, x, seg_rounds, masks, got, bar)
    again = run(x, seg_rounds[0], masks, in_off, out_off)
    assert np.array_equal(bits(got), bits(again)), (name, "two runs differ")
    return got


# ---- 1. walk regimes ----------------------------------------------------------------------------------------------------------------
WALK = C.walk_cases()


@pytest.mark.parametrize("case", WALK, ids=[c[0] for c in WALK])
def test_walk_regimes(case):
    check_case(case)


# ---- 2. base alignment --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [80, 1028])
def test_base_alignment_selects_the_route_and_nothing_else(F):
    """A multiple-of-4 feature dimension in buffers off a 16-byte boundary takes the scalar route: the same bits outside the masks (the
    mean's partial sums are grouped differently on the two routes, so the fill is held to the oracle on each, not to the other route)."""
    outs = {}
    for in_off, out_off in C.ALIGN_OFFSETS:
        case = C.alignment_case(F, in_off, out_off)
        assert case[4]["route"] == ("float4" if (in_off, out_off) == (0, 0) else "scalar")
        outs[in_off, out_off] = check_case(case, in_off=in_off, out_off=out_off)
    _, x, seg_rounds, masks, _ = case
    _, masked = C.regions(x, seg_rounds, masks)
    for key, got in outs.items():
        assert np.array_equal(bits(got)[~masked], bits(outs[0, 0])[~masked]), key


# ---- 3. extreme segments ------------------------------------------------------------------------------------------------------------
EXTREME = C.extreme_cases()


@pytest.mark.parametrize("case", EXTREME, ids=[c[0] for c in EXTREME])
def test_extreme_segments(case):
    name, x, seg_rounds, _, _ = case
    got = check_case(case)
    if name == "seg-forty-in-one-sequence":
        assert np.array_equal(bits(got[1]), bits(x[1]))
    if name != "seg-two-rows":  # (two rows leave center == warped == 1: the identity)
        assert not np.array_equal(got, x)


@pytest.mark.parametrize("n", C.IDENTITY_LENGTHS)
def test_a_segment_with_warped_equal_to_center_returns_its_input_bits(n):
    case = C.identity_case(n)
    got = check_case(case)
    assert np.array_equal(bits(got), bits(case[1]))


# ---- 4. three rounds ----------------------------------------------------------------------------------------------------------------
def test_three_rounds_of_overlapping_segments():
    name, x, seg_rounds, masks, _ = C.rounds_case()
    assert len(seg_rounds) == 3
    xd = torch.from_numpy(x).cuda()
    got = apply_specaug(xd, seg_rounds, masks).cpu().numpy()
    judge(name, x, seg_rounds, masks, got)
    assert np.array_equal(bits(xd.cpu().numpy()), bits(x))
    assert np.array_equal(bits(got), bits(apply_specaug(xd, seg_rounds, masks).cpu().numpy()))
    # masks in the last round only: the first two rounds alone are the oracle's two rounds
    two = apply_specaug(xd, seg_rounds[:2], masks[:0]).cpu().numpy()
    judge(name + "/two", x, seg_rounds[:2], masks[:0], two)


# ---- 5. masks -----------------------------------------------------------------------------------------------------------------------
MASKS = C.mask_cases()


@pytest.mark.parametrize("case", MASKS, ids=[c[0] for c in MASKS])
def test_masks(case):
    name, x, seg_rounds, masks, _ = case
    got = check_case(case)
    warp_only = run(x, seg_rounds[0], masks[:0])
    _, masked = C.regions(x, seg_rounds, masks)
    assert np.array_equal(bits(got)[~masked], bits(warp_only)[~masked])  # the mask pass stores masked elements and nothing else
    if name in ("mask-begin-at-size", "mask-empty"):
        assert not masked.any()
    if name == "mask-all-rows":
        assert masked.all() and all(len(np.unique(bits(got[b]))) == 1 for b in range(x.shape[0]))


def test_a_sequence_without_masks_between_two_that_have_them():
    name, x, seg_rounds, masks, _ = C.between_case()
    got = check_case((name, x, seg_rounds, masks, None))
    warp_only = run(x, seg_rounds[0], masks[:0])
    assert np.array_equal(bits(got[1]), bits(warp_only[1]))
    _, masked = C.regions(x, seg_rounds, masks)
    assert masked[0].any() and masked[2].any() and not masked[1].any()
    assert np.array_equal(bits(got)[~masked], bits(warp_only)[~masked])


# ---- 6. which mean ------------------------------------------------------------------------------------------------------------------
MEANS = C.mean_cases()


@pytest.mark.parametrize("case", MEANS, ids=[c[0] for c in MEANS])
def test_the_fill_is_the_mean_of_the_warped_sequence(case):
    """Data at other levels than the goldens': the bar is 2e-5 * max|x| / 10 (float32 rounding scales with the values)."""
    name, x, seg_rounds, masks, _ = case
    scale = float(np.abs(x).max()) / 10.0
    assert scale > 4.0  # (the goldens' data stays below |x| = 30)
    got = check_case(case, bar=BAR * scale)
    _, masked = C.regions(x, seg_rounds, masks)
    fills = [float(got[b][masked[b]][0]) for b in range(x.shape[0])]
    warped = R.apply(x, seg_rounds, masks[:0]).astype(np.float64)
    # the candidates a wrong kernel could have taken lie far outside the bar
    for b, fill in enumerate(fills):
        of_input = float(x[b].astype(np.float64).mean())
        of_unmasked = float(warped[b][~masked[b]].mean())
        of_batch = float(warped.mean())
        print(f"{name}: sequence {b} fill {fill:.6f}; means: input {of_input:.6f}, unmasked part {of_unmasked:.6f}, batch {of_batch:.6f}")
        if name == "mean-three-levels":
            assert abs(fill - of_batch) > 10
        if name == "mean-moves-with-the-warp":
            assert abs(fill - of_input) > 30
        if name == "mean-counts-the-masked-rows":
            assert abs(fill - of_unmasked) > 5


# ---- 7. the staging ring ------------------------------------------------------------------------------------------------------------
def _ring_call(i):
    """Calls 0, 2, 4, ... are (2, 50, 16); calls 1, 3, 5, 7 have B * tiles = 24, 48, 96, 192 partial sums and 3000, 6000, 12000, 24000 masks
    (12 bytes each on the device: 36, 72, 144, 288 KB).  A slot of the four-slot ring is used every fourth call, so it sees a descriptor
    block four times the one it was sized for and holds twice that one (36 -> 144 KB on slot 1, 72 -> 288 KB on slot 3): it has to be
    released and allocated again."""
    name = f"ring-{i}"
    if i % 2 == 0:
        x = C.data(name, (2, 50, 16))
        return name, x, C.segs((0, 5, 40, 20, 10 + i), (1, 0, 50, 25, 30 - i)), C.masks_of((0, 1, i, i + 6), (1, 2, 3, 7), (0, 2, 15, 21))
    k = i // 2
    T, F = 32 << k, 2048
    x = C.data(name, (3, T, F))
    count = 3000 << k
    idx = np.arange(count)
    axis = 1 + idx % 2
    begin = np.where(axis == 1, (idx * 7) % T, (idx * 13) % F)
    masks = np.zeros(count, dtype=_lib.MASK_DTYPE)
    masks["sequence"], masks["axis"], masks["begin"], masks["end"] = idx % 3, axis, begin, begin + (idx % 100 < 2)  # one in fifty is one wide
    return name, x, C.segs((0, 1, T - 2, T // 2, T // 2 - 3), (2, 0, T, T // 3, T // 3 + 2)), masks


def test_nine_calls_on_two_streams_with_growing_descriptor_blocks():
    lib = _lib.load()
    calls = [_ring_call(i) for i in range(9)]
    assert [c[1].shape[1] * 3 // 4 for c in calls[1::2]] == [24, 48, 96, 192] and [len(c[3]) for c in calls[1::2]] == [3000, 6000, 12000, 24000]
    staged = [(_upload(x, 0),) + _poisoned(x.size, 0) for _, x, _, _ in calls]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i, ((_, x, segs, masks), (xin, _, out, _)) in enumerate(zip(calls, staged)):
        with torch.cuda.stream(streams[i % 2]):
            _call(lib, xin, out, x.shape, segs, masks, streams[i % 2].cuda_stream)
    for s in streams:
        s.synchronize()
    for (name, x, segs, masks), (xin, buf, _, lo) in zip(calls, staged):
        judge(name, x, [segs], masks, _collect(x, xin, buf, lo))


def test_a_non_contiguous_batch_is_its_contiguous_copy():
    base = (torch.randn(200, 3, 40, device="cuda") * 3 - 8)
    view = base.transpose(0, 1)  # (B, T, F) with the batch as the middle stride
    assert view.shape == (3, 200, 40) and not view.is_contiguous()
    tfm = LA.HipSpecAugment(time_warp_factor=10, p=1.0)
    seed_all(7)
    a = tfm(view)
    seed_all(7)
    b = tfm(view.contiguous())
    assert torch.equal(a, b) and a.is_contiguous() and not torch.equal(a, view)
    assert torch.equal(base.transpose(0, 1), view)


# ---- 8. GlobalMVN -------------------------------------------------------------------------------------------------------------------
MVN = C.mvn_cases()


def _mvn(means, stds):
    mvn = LA.HipGlobalMVN(len(means))
    mvn.load_state_dict({"norm_means": torch.from_numpy(means), "norm_stds": torch.from_numpy(stds)})
    return mvn


def _torch_cpu(x, means, stds):
    tx, tm, ts = (torch.from_numpy(a) for a in (x, means, stds))
    return ((tx - tm) / ts).numpy(), (tx * ts + tm).numpy()


@pytest.mark.parametrize("case", MVN, ids=[c[0] for c in MVN])
def test_global_mvn_is_torch_bit_for_bit(case):
    name, x, means, stds = case
    want_fwd, want_inv = _torch_cpu(x, means, stds)
    mvn = _mvn(means, stds)
    xd = torch.from_numpy(x).cuda()  # a (T, F) input
    assert C.same_bits_nan_by_position(mvn(xd).cpu().numpy(), want_fwd)
    assert C.same_bits_nan_by_position(mvn.inverse(xd).cpu().numpy(), want_inv)
    assert C.same_bits_nan_by_position(xd.cpu().numpy(), x)


@pytest.mark.parametrize("F", [1, 3, 80, 257])
def test_global_mvn_layouts(F):
    """A transposed (B, T, F) input and a view four bytes into its storage give what the contiguous batch gives."""
    name, x, means, stds = next(c for c in MVN if c[1].shape[1] == F and c[1].shape[0] in (37, 50, 64, 8161))
    rows = 36
    x = x[:rows]
    want_fwd, want_inv = (w.reshape(4, 9, F) for w in _torch_cpu(x, means, stds))
    mvn = _mvn(means, stds).cuda()
    xd = torch.from_numpy(x).cuda().view(4, 9, F)
    transposed = xd.transpose(0, 1).contiguous().transpose(0, 1)
    assert not transposed.is_contiguous() and torch.equal(transposed.isnan(), xd.isnan())
    base = torch.zeros(rows * F + 4, dtype=torch.float32, device="cuda")
    shifted = base[1 : 1 + rows * F].view(4, 9, F)
    shifted.copy_(xd)
    assert shifted.data_ptr() % 16 == 4
    for src in (xd, transposed, shifted):
        assert C.same_bits_nan_by_position(mvn(src).cpu().numpy(), want_fwd)
        assert C.same_bits_nan_by_position(mvn.inverse(src).cpu().numpy(), want_inv)
    assert bool((base[0] == 0) and (base[1 + rows * F :] == 0).all())
