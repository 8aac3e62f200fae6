"""GPU: the collate launch (lhotse_amd/csrc/kernel_collate.hpp through ``lhotse_amd.augmentation.collate_in_arena``) against its numpy
statement ``collate_ref`` (tests/_collate_ref.py), bit for bit, for float32, float16 and bfloat16 output.

Shapes: the lengths that put a cut's first and last sample on every side of a 16-byte group and of a tile (T = COLLATE_TILE) in ONE
batch; rows of max(len) + 0 ... 3 elements, so that the row starts take every alignment; sources at every residue modulo 4; right
padding, left padding and the destination offsets 1, 2, 3, 5, 9.  ``out`` is a slice of a poisoned tensor whose 64 elements on either side
must stay what they were, and the arena must come back unchanged."""
import numpy as np
import pytest
import torch

from _collate_ref import bits_of, collate_ref

from lhotse_amd import _lib
from lhotse_amd import augmentation as A

pytestmark = pytest.mark.gpu
T = A.COLLATE_TILE
LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, T - 1, T, T + 1, 2 * T + 7]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
GUARD = 64
POISON = {4: 0x5A5A5A5A, 2: 0x5A5A}  # non-zero, and no NaN: 0x5a5a5a5a is 1.5e16 as float32, 0x5a5a is 203.25 as binary16, 1.5e16 as bfloat16
F32_MAX = np.finfo(np.float32).max

# what the 2-byte conversions can get wrong: signed zeros, infinities, the largest float32 (-> inf), binary16 subnormals and the ties
# around them (2^-25 is half the smallest subnormal: to even = 0; 3 * 2^-25: to even = 2^-23), the largest binary16 (65504) and the
# values around the tie to infinity (65520), ties of the 10-bit and of the 7-bit significand in both directions, and their neighbours
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, F32_MAX, -F32_MAX, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)),
                     -(2.0 ** -25), 5.9e-8, 6e-5, 6.1e-5, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 65504.0, 65519.0, 65519.996, 65520.0, -65520.0, 65536.0,
                     1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, np.nextafter(np.float32(1 + 2.0 ** -11), np.float32(2)), np.nextafter(np.float32(1 + 2.0 ** -11), np.float32(0)),
                     1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, np.nextafter(np.float32(1 + 2.0 ** -8), np.float32(2)), np.nextafter(np.float32(1 + 2.0 ** -8), np.float32(0)),
                     -(1 + 2.0 ** -8), 3.3895314e38, 3.3961775e38, 1e-40, -1e-40, 2.0 ** -133, 3 * 2.0 ** -134], dtype=np.float32)


def _pack(lengths, seed=0):
    """An arena packed by hand with gaps of 0 ... 3 floats between the items -> (host arena, offsets); the specials lead every item that
    has room for them."""
    rs = np.random.RandomState(seed)
    offs, pos = [], 4  # (a few floats in front of the first item too)
    for i, n in enumerate(lengths):
        pos += i % 4
        offs.append(pos)
        pos += n
    arena = (rs.randn(pos + 5) * 10.0 ** rs.uniform(-6, 3, pos + 5)).astype(np.float32)
    for o, n in zip(offs, lengths):
        k = min(n, len(SPECIALS))
        arena[o : o + k] = np.roll(SPECIALS, o)[:k]
    return arena, np.asarray(offs, dtype=np.int64)


@pytest.fixture(scope="module")
def batch():
    arena, offs = _pack(LENGTHS)
    assert sorted({int(o) % 4 for o in offs}) == [0, 1, 2, 3]  # sources at every residue modulo 4
    return arena, offs, torch.from_numpy(arena).cuda()


def _dst(mode, lengths, row_len):
    lens = np.asarray(lengths, dtype=np.int64)
    if mode == "right":
        return None
    if mode == "left":
        return A.left_pad_offsets(lens, row_len)
    return np.minimum(np.resize([1, 2, 3, 5, 9], len(lens)), row_len - lens)  # (a row that is full, or nearly, has no room for more)


def _run(d_arena, offs, lengths, row_len, dst, dtype, guard_front=GUARD):
    """collate_in_arena into a slice of a poisoned tensor -> (result, the whole poisoned tensor's bits, the poison)"""
    size = torch.empty((), dtype=dtype).element_size()
    n = len(lengths) * row_len
    big = torch.empty(guard_front + n + GUARD, dtype=torch.int32 if size == 4 else torch.int16, device="cuda")
    big.fill_(POISON[size] if size == 4 else np.int16(POISON[size]).item())
    out = big.view(dtype)[guard_front : guard_front + n]
    res, lens = A.collate_in_arena(d_arena, offs, lengths, row_len=row_len, dst_offsets=dst, dtype=dtype, out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr() and tuple(res.shape) == (len(lengths), row_len) and lens.tolist() == list(lengths)
    whole = bits_of(big.view(dtype))
    assert (whole[:guard_front] == POISON[size]).all() and (whole[guard_front + n :] == POISON[size]).all(), "a guard element changed"
    return res


@pytest.mark.parametrize("mode", ["right", "left", "offsets"])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_one_ragged_batch_bit_for_bit(batch, dtype, k, mode):
    arena, offs, d_arena = batch
    row_len = max(LENGTHS) + k
    dst = _dst(mode, LENGTHS, row_len)
    if mode == "offsets":  # source and destination alignments differ in every way
        assert {int(o - d) % 4 for o, d, n in zip(offs, dst, LENGTHS) if n >= 8} == {0, 1, 2, 3}
    res = _run(d_arena, offs, LENGTHS, row_len, dst, dtype)
    want = collate_ref(arena, offs, LENGTHS, row_len, dst, dtype)
    got_b, want_b = bits_of(res), bits_of(want)
    bad = np.argwhere(got_b != want_b)
    assert not len(bad), (str(dtype), k, mode, bad[:5].tolist(), [hex(int(got_b[tuple(b)])) for b in bad[:5]], [hex(int(want_b[tuple(b)])) for b in bad[:5]])
    assert np.array_equal(d_arena.cpu().numpy().view(np.uint32), arena.view(np.uint32))  # the arena is only read


def test_the_row_alignments_of_the_sweep_cover_every_residue():
    """Rows start at r * row_len: with row_len = max(len) + 0 ... 3 the rows of the sweep start at every element of a 16-byte group."""
    for vec in (4, 8):
        seen = {(r * (max(LENGTHS) + k)) % vec for k in range(4) for r in range(len(LENGTHS))}
        assert seen == set(range(vec))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_the_special_values_convert_as_torch_converts_them(dtype):
    """The expected values are torch's CPU ``.to(dtype)`` of the same float32 values (``collate_ref`` is that), NaNs apart."""
    x = np.concatenate([SPECIALS, -SPECIALS[::-1]]).astype(np.float32)
    res = _run(torch.from_numpy(x).cuda(), [0], [len(x)], len(x) + 3, [2], dtype)
    want = torch.zeros(len(x) + 3, dtype=dtype)
    want[2 : 2 + len(x)] = torch.from_numpy(x).to(dtype)
    assert np.array_equal(bits_of(res[0]), bits_of(want))
    if dtype == torch.float16:  # (the cases are what their names say)
        h = torch.from_numpy(SPECIALS).to(dtype)
        assert float(h[7]) == 0.0 and float(h[8]) == 2.0 ** -23 and float(h[16]) == 65504.0 and float(h[18]) == 65504.0 and float(h[19]) == float("inf")
        assert float(h[22]) == 1.0 and float(h[23]) == 1 + 2.0 ** -9 and float(h[4]) == float("inf")
    if dtype == torch.bfloat16:
        b = torch.from_numpy(SPECIALS).to(dtype)
        assert float(b[26]) == 1.0 and float(b[27]) == 1 + 2.0 ** -6 and float(b[4]) == float("inf") and float(b[31]) < float("inf") and float(b[32]) == float("inf")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_one_row_and_a_batch_of_full_rows(dtype):
    arena, offs = _pack([T + 1], seed=1)
    d = torch.from_numpy(arena).cuda()
    res = _run(d, offs, [T + 1], T + 1, None, dtype)  # B = 1, and the row is full
    assert np.array_equal(bits_of(res), bits_of(collate_ref(arena, offs, [T + 1], T + 1, None, dtype)))
    lens = [T + 5] * 5  # every row is full: no padding is written anywhere; rows start at 0, 1, 2, 3, 4 modulo 4
    arena, offs = _pack(lens, seed=2)
    res = _run(torch.from_numpy(arena).cuda(), offs, lens, T + 5, None, dtype)
    assert np.array_equal(bits_of(res), bits_of(collate_ref(arena, offs, lens, T + 5, None, dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_an_out_that_starts_off_a_16_byte_boundary(dtype):
    """``out`` is aligned to its element size, no more: the row alignment is taken from the address, not from the row index."""
    lens = [9, 0, T + 1, 33]
    arena, offs = _pack(lens, seed=3)
    d = torch.from_numpy(arena).cuda()
    for front in (GUARD + 1, GUARD + 3):
        res = _run(d, offs, lens, T + 2, [1, 0, 1, 5], dtype, guard_front=front)
        assert res.data_ptr() % 16 != 0
        assert np.array_equal(bits_of(res), bits_of(collate_ref(arena, offs, lens, T + 2, [1, 0, 1, 5], dtype)))


def test_the_launch_is_ordered_behind_a_copy_on_the_same_stream(batch):
    """On a stream of its own: a ``copy_`` fills the arena, the collate launch follows with no synchronisation in between."""
    arena, offs, _ = batch
    host = torch.from_numpy(arena).pin_memory()
    big = torch.from_numpy(np.random.RandomState(5).randn(1 << 24).astype(np.float32)).pin_memory()  # 64 MiB in front: the copies take a while
    d_big = torch.empty(1 << 24, device="cuda")
    d_arena = torch.full((len(arena),), float("nan"), device="cuda")
    row_len = max(LENGTHS) + 1
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_big.copy_(big, non_blocking=True)
        d_arena.copy_(host, non_blocking=True)
        res, _ = A.collate_in_arena(d_arena, offs, LENGTHS, row_len=row_len, dtype=torch.float32)
    s.synchronize()
    assert np.array_equal(bits_of(res), bits_of(collate_ref(arena, offs, LENGTHS, row_len)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_two_runs_give_equal_bits(batch, dtype):
    arena, offs, d_arena = batch
    row_len = max(LENGTHS) + 3
    dst = _dst("offsets", LENGTHS, row_len)
    a = _run(d_arena, offs, LENGTHS, row_len, dst, dtype)
    b = _run(d_arena, offs, LENGTHS, row_len, dst, dtype)
    assert np.array_equal(bits_of(a), bits_of(b))


def test_defaults_and_the_result_of_no_rows(batch):
    arena, offs, d_arena = batch
    res, lens = A.collate_in_arena(d_arena, offs, LENGTHS)  # row_len: the longest cut; right padding; float32; a tensor of its own
    torch.cuda.synchronize()
    assert tuple(res.shape) == (len(LENGTHS), max(LENGTHS)) and res.dtype == torch.float32 and res.is_cuda and lens.dtype == np.int64
    assert np.array_equal(bits_of(res), bits_of(collate_ref(arena, offs, LENGTHS)))
    res, lens = A.collate_in_arena(d_arena, [], [])
    assert tuple(res.shape) == (0, 0) and res.is_cuda and len(lens) == 0


def test_what_the_host_refuses_launches_nothing(batch):
    """All of this is decided on the host: nothing is enqueued, so nothing can go wrong on the device."""
    arena, offs, d_arena = batch
    lib = _lib.load()
    co = A.HipCollator("cuda")  # a private one: a refused run leaves its plan outstanding
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.full((64,), 7.0, device="cuda")
    # rows == 0: a valid plan whose run launches nothing
    ticket, info = co.plan([], [], None, 16)
    assert info.tolist() == [ticket, 0, 0, 0]
    co.run(ticket, d_arena, out)
    assert lib.raw("hipfeat_collate_run", co.handle, ticket, d_arena.data_ptr(), d_arena.numel(), out.data_ptr(), out.numel(), stream) == _lib.ERR_INVALID  # it ran once
    # an overlapping out, an arena or an out smaller than planned, an unknown ticket
    with pytest.raises(ValueError, match="overlaps"):
        A.collate_in_arena(d_arena, offs[:2], LENGTHS[:2], row_len=4, out=d_arena[8:16])
    ticket, info = co.plan([0, 8], [8, 8], None, 8)
    assert info.tolist() == [ticket, 16, 16, 2]
    inside = d_arena[32:48]
    assert lib.raw("hipfeat_collate_run", co.handle, ticket, d_arena.data_ptr(), d_arena.numel(), inside.data_ptr(), 16, stream) == _lib.ERR_INVALID
    assert "overlaps" in lib.last_error()
    assert lib.raw("hipfeat_collate_run", co.handle, ticket, d_arena.data_ptr(), 15, out.data_ptr(), out.numel(), stream) == _lib.ERR_INVALID
    assert "arena holds" in lib.last_error()
    assert lib.raw("hipfeat_collate_run", co.handle, ticket, d_arena.data_ptr(), d_arena.numel(), out.data_ptr(), 15, stream) == _lib.ERR_INVALID
    assert "out holds" in lib.last_error()
    assert lib.raw("hipfeat_collate_run", co.handle, ticket + 1, d_arena.data_ptr(), d_arena.numel(), out.data_ptr(), out.numel(), stream) == _lib.ERR_INVALID
    with pytest.raises(_lib.HipFeatError) as e:
        co.plan([0], [8], [1], 8)
    assert e.value.status == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and np.array_equal(d_arena.cpu().numpy().view(np.uint32), arena.view(np.uint32))
    co.run(ticket, d_arena, out)  # the refused runs left the ticket planned: it still runs, once
    torch.cuda.synchronize()
    assert np.array_equal(out[:16].cpu().numpy(), arena[:16]) and bool((out[16:] == 7.0).all())
    co.close()
