"""CPU: the LDS exchange between the two FFT passes of fft512c_kernel (kernel_fft512c.hpp::exchange_halves) modelled instruction by
instruction from the constants the kernel is compiled with (lhotse_amd/csrc/fft512c_geom.hpp through tests/native/fft512c_geom_capi.cpp),
and the filterbank instance plan creation picks for a schedule.

The exchange, per wave (lane = 16 g + q: frame g, FFT lane q), for the halves h = 0, 1 of the pass-1 rows k1 = 8 h + rr:
  four ds_write2_b64   lane (g, q) stores its value of row rr at  g * frame_stride + rr * row_stride + 2 q  (dwords; two rows per instruction)
  eight ds_read_b128   lane (g, q) loads the dwords  g * frame_stride + (q % 8) * row_stride + 4 j .. + 3,  j = 0 .. 7: the columns 2 j and
                       2 j + 1 of "its" row; half 0 under the full exec mask, half 1 under q >= 8, over half 0's registers
so that afterwards lane (g, q) holds row k1 = q of frame g, column n2 in register pair n2.

Banking (LDS of CDNA4, 64 banks of 4 bytes): a ds_read_b128 is served in the four 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19,
28-31} and the same + 32, bank = dword address mod 64, so a conflict-free group touches 64 distinct banks.  A 64-bit store is served in
four groups of 16 consecutive lanes, one access per element of a ds_write2_b64: such a group stores 16 x 8 bytes = 32 dwords per element,
so "conflict-free" is 32 distinct banks per element (its 128 bytes are contiguous: true for any row stride) -- the 64 dwords of the two
elements of a group cannot lie on 64 distinct banks for any row stride below 64 dwords, and are not served in one cycle either.  The
test asserts the 32 per element and that the two elements of a group never share a dword.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from lhotse_amd import constants as C
from test_mel4_schedule import build as build_schedule
from test_mel4_schedule import emulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ_GROUPS = [sorted(list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28))), sorted(list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)))]
READ_GROUPS += [[l + 32 for l in grp] for grp in READ_GROUPS]
WRITE_GROUPS = [list(range(16 * i, 16 * i + 16)) for i in range(4)]


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(tempfile.mkdtemp(prefix="f5g_"), "libf5g.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "fft512c_geom_capi.cpp"), "-o", out])
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def mel4_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="f5g_mel4_"), "libmel4.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "mel4_schedule_capi.cpp"), "-o", out])
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def geom(lib):
    v = (ctypes.c_int * 6)()
    lib.f5g_constants(v)
    return dict(zip(["row", "frame", "prow", "region", "max_sets", "max_steps"], list(v)))


LANES = np.arange(64)
Q, G = LANES & 15, LANES >> 4


def write_addresses(geom, j):
    """dword addresses of the two elements of the j-th ds_write2_b64 of a half, per lane: (2, 64); element e is row 2 j + e"""
    unit = geom["row"] // 2  # the instruction's offsets count 8-byte units: 18 rr
    assert 2 * unit == geom["row"] and (2 * j + 1) * unit < 256, "offset0 / offset1 have 8 bits"
    base = G * geom["frame"] + 2 * Q
    return np.stack([base + 2 * unit * (2 * j + e) for e in (0, 1)])


def read_addresses(geom, j):
    """first dword address of the j-th ds_read_b128 of a half, per lane"""
    return G * geom["frame"] + (Q % 8) * geom["row"] + 4 * j


def test_every_value_reaches_the_lane_that_owns_its_row(geom):
    lds = np.full(geom["region"], -1, dtype=np.int64)  # tag of (half, frame, row rr, column) = ((h * 4 + g) * 8 + rr) * 16 + column
    regs = np.full((64, 16, 2), -1, dtype=np.int64)  # per lane: 16 columns x (re, im) as (tag, dword of the pair)
    written = np.zeros(geom["region"], dtype=bool)
    read = np.zeros(geom["region"], dtype=bool)
    for h in (0, 1):
        for j in range(4):
            for e, addr in enumerate(write_addresses(geom, j)):
                tag = ((h * 4 + G) * 8 + 2 * j + e) * 16 + Q
                for d in (0, 1):
                    lds[addr + d] = 2 * tag + d
                    written[addr + d] = True
        active = np.ones(64, dtype=bool) if h == 0 else Q >= 8
        for j in range(8):
            addr = read_addresses(geom, j)
            for d in range(4):
                regs[active, 2 * j + d // 2, d % 2] = lds[addr[active] + d]
                read[addr[active] + d] = True
    # lane (g, q) holds row k1 = q of its frame -- half q // 8, row q % 8 of the block -- column n2 in register pair n2
    n2 = np.arange(16)
    want = ((((Q >> 3) * 4 + G) * 8 + Q % 8)[:, None] * 16 + n2[None, :])
    assert np.array_equal(regs[:, :, 0], 2 * want) and np.array_equal(regs[:, :, 1], 2 * want + 1)
    # each (half, frame, row, column) that was written ends up in exactly one lane's registers: the owner's
    tags, counts = np.unique(regs[:, :, 0] // 2, return_counts=True)
    assert len(tags) == 64 * 16 and (counts == 1).all()
    # nothing is read that was not written (the 4 padding dwords of a row in particular), nothing lies outside the region
    assert not (read & ~written).any()
    pad = np.zeros(geom["region"], dtype=bool)
    for g in range(4):
        for r in range(8):
            pad[g * geom["frame"] + r * geom["row"] + 32 : g * geom["frame"] + (r + 1) * geom["row"]] = True
    pad[4 * geom["frame"] :] = True
    assert not (pad & (read | written)).any() and (written | pad).all()


def test_addresses_are_aligned_and_inside_the_region(geom):
    assert geom["row"] % 4 == 0 and geom["frame"] % 4 == 0 and geom["region"] % 4 == 0
    assert geom["frame"] == 8 * geom["row"] and 4 * geom["frame"] <= geom["region"] and 4 * geom["prow"] <= geom["region"]
    for j in range(8):
        a = read_addresses(geom, j)
        assert (a % 4 == 0).all(), "ds_read_b128: 16-byte aligned"
        assert (a >= 0).all() and (a + 4 <= geom["region"]).all()
        assert 16 * j < 65536
    for j in range(4):
        a = write_addresses(geom, j)
        assert (a % 2 == 0).all(), "ds_write2_b64: 8-byte aligned"
        assert (a >= 0).all() and (a + 2 <= geom["region"]).all()


@pytest.mark.parametrize("half", [0, 1])
def test_reads_are_conflict_free(geom, half):
    active = np.ones(64, dtype=bool) if half == 0 else Q >= 8
    for j in range(8):
        a = read_addresses(geom, j)
        for grp in READ_GROUPS:
            lanes = [l for l in grp if active[l]]
            banks = np.concatenate([(a[lanes] + d) % 64 for d in range(4)])
            assert len(set(banks.tolist())) == 4 * len(lanes), (half, j, grp)
            if half == 0:
                assert len(lanes) == 16 and len(set(banks.tolist())) == 64


def test_writes_are_conflict_free(geom):
    for j in range(4):
        a = write_addresses(geom, j)
        for grp in WRITE_GROUPS:
            both = []
            for e in (0, 1):
                dwords = np.concatenate([a[e][grp], a[e][grp] + 1])
                assert len(set((dwords % 32).tolist())) == 32, (j, e, grp)  # one element: 128 contiguous bytes of one frame's row
                assert dwords.max() - dwords.min() == 31
                both += dwords.tolist()
            assert len(set(both)) == 64, (j, grp)


# ---- the filterbank instance and its trimmed accumulator sets -----------------------------------------------------------------------


def _instance(lib, mel):
    K, M = mel.shape
    mel = np.ascontiguousarray(mel, dtype=np.float32)
    sched, inst = (ctypes.c_int * 4)(), (ctypes.c_int * 2)()
    nsets = lib.f5g_instance(mel.ctypes.data_as(ctypes.c_void_p), M, K, sched, inst)
    return nsets, list(sched)[:nsets], list(inst)


@pytest.mark.parametrize("M,steps", [(80, [16, 12]), (72, [16, 12]), (64, [16, 8])])
def test_instance_carries_the_schedules_step_counts(lib, M, steps):
    mel = np.asarray(C.make_kaldi_mel(M, 512, 16000, 20.0, -400.0), dtype=np.float32)
    nsets, sched, inst = _instance(lib, mel)
    assert nsets == 2 and sched == steps, (M, sched)
    assert inst == sched, "the instance runs exactly the schedule's steps"


def test_other_schedules_keep_the_padded_instance(lib, geom):
    inst = (ctypes.c_int * 2)()
    full = [geom["max_steps"]] * 2
    for nsets, steps in [(1, [16, 0]), (2, [16, 16]), (2, [16, 4]), (2, [12, 12]), (2, [12, 8]), (2, [8, 8]), (1, [12, 0])]:
        lib.f5g_mel_steps(nsets, (ctypes.c_int * 4)(*steps, 0, 0), inst)
        assert list(inst) == full, (nsets, steps)
    for steps in ([16, 12], [16, 8]):
        lib.f5g_mel_steps(2, (ctypes.c_int * 4)(*steps, 0, 0), inst)
        assert list(inst) == steps


@pytest.mark.parametrize("M", [80, 72, 64])
def test_trimmed_sets_equal_the_16_step_run_bit_for_bit(lib, mel4_lib, geom, M):
    """The kernel's weight table keeps 16 steps per set, zero past a set's own; an instance with the schedule's counts leaves the zero
    steps out.  Emulation of test_mel4_schedule.py on that padded table, run over 16 steps per set and over the instance's counts."""
    mel = np.asarray(C.make_kaldi_mel(M, 512, 16000, 20.0, -400.0), dtype=np.float32)
    nsets, steps, step0, wtab, ltab = build_schedule(mel4_lib, mel, geom["max_sets"], geom["max_steps"])
    _, sched, inst = _instance(lib, mel)
    assert steps == sched
    T = geom["max_steps"]
    padded = np.zeros((nsets * T // 4, 64, 4), dtype=np.float32)
    for s in range(nsets):
        padded[s * T // 4 : s * T // 4 + steps[s] // 4] = wtab[step0[s] // 4 : (step0[s] + steps[s]) // 4]
    poff = ltab[:, :, 0].view(np.int32)
    assert (poff + T <= 4 * geom["prow"]).all(), "the 16-step run stays inside the wave's power rows"
    rs = np.random.RandomState(M)
    P = np.zeros((4, geom["prow"]), dtype=np.float32)  # (the padding past bin 256 is zeroed every round)
    P[:, :257] = rs.rand(4, 257).astype(np.float32) ** 4 * 50.0
    P[:, rs.randint(0, 257, 20)] = 0.0
    pad_step0 = [s * T for s in range(nsets)]
    full, seen = emulate((nsets, [T] * nsets, pad_step0, padded, ltab), P, M)
    trim, seen_t = emulate((nsets, inst[:nsets], pad_step0, padded, ltab), P, M)
    assert (seen == 1).all() and (seen_t == 1).all()
    assert np.array_equal(full, trim)
    assert np.array_equal(full, emulate((nsets, steps, step0, wtab, ltab), P, M)[0])
