"""CPU: the collate entry points (additive to ABI v8) are declared in the header with their own export macro, mirrored in
``_lib._COLLATE_SIGNATURES`` and exported by the built library (its symbol table; no device is touched); the plan -- the row table, every
plan-time error and the 16 ticket slots -- is what csrc/collate_tables.hpp decides, checked here through
tests/native/collate_tables_capi.cpp without a device."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from lhotse_amd import _lib, build
from lhotse_amd.augmentation import COLLATE_TILE

from test_abi import HEADER, declared_functions

COLLATE_API = {"hipfeat_collate_create", "hipfeat_collate_destroy", "hipfeat_collate_plan", "hipfeat_collate_run"}
SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "collate_tables_capi.cpp")
OK, INVALID = 0, 1
F32, F16, BF16 = 0, 1, 2
ROW_DTYPE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("len", "<i8"), ("pad", "<i8")])
I64_MAX = 2 ** 63 - 1


def test_collate_entry_points_are_declared_mirrored_and_exported():
    declared = set(re.findall(r"HIPFEAT_COLLATE_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\(", open(HEADER).read()))
    assert declared == COLLATE_API == set(_lib._COLLATE_SIGNATURES)
    # ... and absent from the v8 set and from the level set, which older tests count
    assert set(declared_functions()) == set(_lib._SIGNATURES)
    assert not COLLATE_API & set(_lib._SIGNATURES) and not COLLATE_API & set(_lib._LEVEL_SIGNATURES)
    assert all(callable(_lib.load().fn(name)) for name in COLLATE_API)  # the loaded library binds them
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    assert COLLATE_API <= set(re.findall(r" T (hipfeat_\w+)", out))


def test_the_abi_version_is_still_8():
    text = open(HEADER).read()
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", text).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version") == 8
    assert "v8 libraries built from this commit on also carry hipfeat_collate_*" in text


def test_prototypes_match_the_signature_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(COLLATE_API):
        proto = re.search(r"HIPFEAT_COLLATE_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert _lib._COLLATE_SIGNATURES[name] == ("int", args), (name, args)


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(tempfile.mkdtemp(prefix="cotab_"), "libcotab.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", out])
    lib = ctypes.CDLL(out)
    lib.ct_plan.restype = ctypes.c_int
    lib.ct_plan.argtypes = [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p,
                            ctypes.c_void_p, ctypes.c_void_p]
    lib.ct_slots_plan.restype = ctypes.c_longlong
    lib.ct_slots_run.argtypes = [ctypes.c_longlong]
    lib.ct_tiles.restype = ctypes.c_longlong
    lib.ct_tiles.argtypes = [ctypes.c_longlong, ctypes.c_int]
    return lib


POISON = -12345


def plan(shim, src, lens, dst, row_len, out_type=F32, rows=None):
    """-> (status, info, row table, message); ``info`` is pre-filled with POISON so that "plans nothing" can be seen."""
    so, sl = _lib.i64(src), _lib.i64(lens)
    do = None if dst is None else _lib.i64(dst)
    n = len(so) if rows is None else rows
    info, table, msg = np.full(4, POISON, np.int64), np.zeros(max(n, 0), ROW_DTYPE), ctypes.create_string_buffer(256)
    st = shim.ct_plan(n, so.ctypes.data, sl.ctypes.data, None if do is None else do.ctypes.data, row_len, out_type, info.ctypes.data, table.ctypes.data,
                      ctypes.addressof(msg))
    return st, info, table, msg.value.decode()


def test_the_table_is_what_the_kernel_reads(shim):
    assert ROW_DTYPE.itemsize == 32 and shim.ct_tile() == COLLATE_TILE == 4096 and shim.ct_slots() == 16
    src, lens, dst = [0, 4099, 9001, 2 ** 40], [4096, 4094, 70001, 0], [0, 7, 3, 70004]
    st, info, table, msg = plan(shim, src, lens, dst, 70004, F16)
    assert st == OK, msg
    assert table["src_off"].tolist() == src and table["len"].tolist() == lens and table["dst_off"].tolist() == dst
    tiles = (70004 - 1 + 7) // COLLATE_TILE + 1  # 8 two-byte elements per 16 bytes: a row starts at most 7 elements behind a boundary
    assert shim.ct_tiles(70004, F16) == tiles == 18 and shim.ct_tiles(70004, F32) == 18 and shim.ct_tiles(0, F32) == 0
    assert shim.ct_tiles(4096, F32) == 2 and shim.ct_tiles(4093, F32) == 1 and shim.ct_tiles(4089, BF16) == 1 and shim.ct_tiles(4090, BF16) == 2
    # {ticket, floats the arena must hold (the row of padding at 2^40 reads nothing), elements of out, work items}
    assert info.tolist() == [0, 9001 + 70001, 4 * 70004, 4 * tiles]
    st, info, table, _ = plan(shim, src[:3], lens[:3], None, 70001)  # NULL destination offsets: 0 for every row
    assert st == OK and table["dst_off"].tolist() == [0, 0, 0] and info.tolist() == [0, 79002, 3 * 70001, 3 * 18]


def test_plan_time_errors_are_decided_on_the_host(shim):
    def refused(*a, **k):
        st, info, _, msg = plan(shim, *a, **k)
        assert (st == INVALID and msg and info.tolist() == [POISON] * 4) or st == OK, (st, msg)  # a refusal plans nothing
        return st == INVALID

    assert not refused([0], [8], [0], 8)
    assert refused([-1], [8], [0], 8) and refused([0], [8], [-1], 16)  # a negative source / destination offset
    assert refused([0], [-1], [0], 8)  # src_len < 0
    assert refused([0], [0], [0], -1) and refused([], [], [], -1)  # row_len < 0
    assert refused([0], [8], [1], 8) and refused([0], [9], [0], 8) and refused([0, 0], [8, 4], [0, 5], 8)  # dst_off + src_len > row_len
    assert not refused([0, 0], [8, 4], [0, 4], 8)  # ... == row_len is a full row
    assert refused([0], [1], [I64_MAX], I64_MAX)  # (the comparison itself must not overflow)
    assert refused([0, 0, 0], [0, 0, 0], None, 2 ** 62)  # rows * row_len beyond INT64_MAX
    assert not refused([0], [0], None, I64_MAX)
    assert refused([I64_MAX - 3], [4], [0], 8) and not refused([I64_MAX - 4], [4], [0], 8)  # src_off + src_len beyond INT64_MAX
    for bad in (-1, 3, 7):
        assert refused([0], [8], [0], 8, out_type=bad)  # an unknown output type
    for ok in (F32, F16, BF16):
        assert not refused([0], [8], [0], 8, out_type=ok)
    assert refused([], [], [], 8, rows=-1)
    st, _, _, msg = plan(shim, [0, 5], [8, 9], [0, 0], 8)
    assert st == INVALID and "row 1" in msg and "do not fit" in msg


def test_a_17th_plan_while_16_are_outstanding_is_refused(shim):
    shim.ct_slots_reset()
    assert [shim.ct_slots_plan() for _ in range(16)] == list(range(16))
    assert shim.ct_slots_plan() == -1 and shim.ct_slots_plan() == -1  # refused, and nothing planned: the 16 stay what they were
    assert shim.ct_slots_run(16) == INVALID and shim.ct_slots_run(-1) == INVALID  # unknown tickets
    assert shim.ct_slots_run(5) == OK and shim.ct_slots_plan() == -1  # the slot ticket 16 would take (0) is still planned
    assert shim.ct_slots_run(0) == OK and shim.ct_slots_run(0) == INVALID  # a ticket runs once
    assert shim.ct_slots_plan() == 16 and shim.ct_slots_run(16) == OK
    for t in (1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15):
        assert shim.ct_slots_run(t) == OK
    assert shim.ct_slots_plan() == 17


def test_valid_edge_plans(shim):
    st, info, _, msg = plan(shim, [], [], [], 100)  # no rows: a plan whose run launches nothing
    assert st == OK and info.tolist() == [0, 0, 0, 0], msg
    st, info, _, msg = plan(shim, [], [], None, 0, BF16)
    assert st == OK and info.tolist() == [0, 0, 0, 0], msg
    st, info, table, msg = plan(shim, [123456], [0], [5], 10)  # a row of padding only: nothing of the arena is needed
    assert st == OK and info.tolist() == [0, 0, 10, 1] and table["len"].tolist() == [0], msg
    st, info, _, msg = plan(shim, [0, 0], [0, 0], None, 0)  # rows of no elements: nothing to launch either
    assert st == OK and info.tolist() == [0, 0, 0, 0], msg
    st, info, table, msg = plan(shim, [4], [6], [4], 10)  # dst_off + src_len == row_len
    assert st == OK and info.tolist() == [0, 10, 10, 1] and table["dst_off"].tolist() == [4], msg


def test_offsets_past_2_31_travel_unchanged(shim):
    far, farther = 2 ** 31 + 1, 2 ** 40
    st, info, table, msg = plan(shim, [far, farther, 5], [4099, 70001, 8], [2 ** 33, 0, 1], 2 ** 33 + 4099, F16)
    assert st == OK, msg
    assert table["src_off"].tolist() == [far, farther, 5] and table["dst_off"].tolist() == [2 ** 33, 0, 1] and table["len"].tolist() == [4099, 70001, 8]
    tiles = (2 ** 33 + 4099 - 1 + 7) // COLLATE_TILE + 1
    assert info.tolist() == [0, farther + 70001, 3 * (2 ** 33 + 4099), 3 * tiles]


def test_stand_alone_program_of_the_shim(tmp_path):
    exe = str(tmp_path / "cotab")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DCOLLATE_TABLES_MAIN", SHIM, "-o", exe])
    # (bounds and overflow are what is looked for; the leak check at exit needs ptrace, which not every container grants)
    res = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
