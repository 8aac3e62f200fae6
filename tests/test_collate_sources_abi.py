"""CPU: ``hipfeat_collate_plan_sources`` (additive to ABI v8) is declared in the header with its own export macro, mirrored in
``_lib._CHANNELS_SIGNATURES`` and exported by the built library (its symbol table; no device is touched); the plan of the sources form --
the row table with the first-source index and count in ``CoRow.pad``, the staged source offsets, every plan-time refusal, the arena need,
the work items and the 16 ticket slots it shares with ``hipfeat_collate_plan`` -- is what csrc/collate_tables.hpp decides, checked here
through tests/native/collate_sources_capi.cpp without a device."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from lhotse_amd import _lib, build
from lhotse_amd.augmentation import COLLATE_MAX_SOURCES, COLLATE_TILE, collate_sources_layout

from test_abi import HEADER, declared_functions

CHANNELS_API = {"hipfeat_collate_plan_sources"}
SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "collate_sources_capi.cpp")
OK, INVALID, UNSUPPORTED = 0, 1, 3
F32, F16, BF16 = 0, 1, 2
ROW_DTYPE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("len", "<i8"), ("pad", "<i8")])
I64_MAX = 2 ** 63 - 1
POISON = -12345


def test_the_entry_point_is_declared_mirrored_and_exported():
    text = open(HEADER).read()
    declared = set(re.findall(r"HIPFEAT_CHANNELS_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\(", text))
    assert declared == CHANNELS_API == set(_lib._CHANNELS_SIGNATURES)
    assert re.search(r"#define\s+HIPFEAT_CHANNELS_API\s+HIPFEAT_API\b", text)
    assert CHANNELS_API <= set(_lib._ADDED_SIGNATURES)
    # ... and absent from the v8 set and from the collate set, which older tests count
    assert set(declared_functions()) == set(_lib._SIGNATURES)
    assert not CHANNELS_API & set(_lib._SIGNATURES) and not CHANNELS_API & set(_lib._COLLATE_SIGNATURES)
    assert all(callable(_lib.load().fn(name)) for name in CHANNELS_API)  # the loaded library binds it
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    assert CHANNELS_API <= set(re.findall(r" T (hipfeat_\w+)", out))


def test_the_abi_version_is_still_8_and_the_block_cites_the_reference():
    text = open(HEADER).read()
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", text).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version") == 8
    start = text.index("v8 libraries built from this commit on also carry hipfeat_collate_plan_sources")
    doc = text[start: text.index("HIPFEAT_CHANNELS_API hipfeat_status hipfeat_collate_plan_sources")]
    for cited in ("collation.py:215-241", "did not change because nothing that existed changed", "k = 0", "k = 1", "k >= 2", "ascending source order", "one\n *           float64 division",
                  "HIPFEAT_ERR_UNSUPPORTED", "HIPFEAT_ERR_INVALID", "more than 32 sources"):
        assert cited in doc, cited


def test_the_prototype_matches_the_signature_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(CHANNELS_API):
        proto = re.search(r"HIPFEAT_CHANNELS_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert _lib._CHANNELS_SIGNATURES[name] == ("int", args), (name, args)


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(tempfile.mkdtemp(prefix="cosrc_"), "libcosrc.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", out])
    lib = ctypes.CDLL(out)
    lib.cs_plan.restype = ctypes.c_int
    lib.cs_plan.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 4 + [ctypes.c_longlong, ctypes.c_int] + [ctypes.c_void_p] * 4
    lib.cs_slots_plan.restype = ctypes.c_longlong
    lib.cs_slots_run.argtypes = [ctypes.c_longlong]
    lib.cs_first_source.restype = ctypes.c_longlong
    lib.cs_first_source.argtypes = [ctypes.c_longlong]
    lib.cs_num_sources.argtypes = [ctypes.c_longlong]
    lib.cs_tiles.restype = ctypes.c_longlong
    lib.cs_tiles.argtypes = [ctypes.c_longlong, ctypes.c_int]
    return lib


def plan(shim, first, src, lens, dst, row_len, out_type=F32, rows=None):
    """-> (status, info, row table, staged source offsets, message); ``info`` is pre-filled with POISON so that "plans nothing" shows."""
    fi, so, sl = _lib.i64(first), _lib.i64(src), _lib.i64(lens)
    do = None if dst is None else _lib.i64(dst)
    n = len(sl) if rows is None else rows
    info, table, srcs, msg = np.full(4, POISON, np.int64), np.zeros(max(n, 0), ROW_DTYPE), np.full(len(so), POISON, np.int64), ctypes.create_string_buffer(256)
    st = shim.cs_plan(n, fi.ctypes.data, so.ctypes.data, sl.ctypes.data, None if do is None else do.ctypes.data, row_len, out_type, info.ctypes.data,
                      table.ctypes.data, srcs.ctypes.data, ctypes.addressof(msg))
    return st, info, table, srcs, msg.value.decode()


def test_the_tables_are_what_the_kernel_reads(shim):
    assert ROW_DTYPE.itemsize == 32 and shim.cs_max_sources() == COLLATE_MAX_SOURCES == 32 and shim.cs_slots() == 16
    # rows of 2, 0, 1 and 3 sources; the last row has no samples
    first, src = [0, 2, 2, 3, 6], [100, 9000, 20000, 2 ** 40, 2 ** 41, 2 ** 42]
    lens, dst = [4097, 4000, 70001, 0], [3, 0, 0, 70001]
    st, info, table, srcs, msg = plan(shim, first, src, lens, dst, 70001, F16)
    assert st == OK, msg
    assert srcs.tolist() == src
    assert [shim.cs_first_source(int(p)) for p in table["pad"]] == first[:-1]
    assert [shim.cs_num_sources(int(p)) for p in table["pad"]] == [2, 0, 1, 3]
    assert table["src_off"].tolist() == [100, 0, 20000, 2 ** 40]  # the first source (what a row of one source reads); 0 without sources
    assert table["len"].tolist() == [4097, 0, 70001, 0]  # k = 0: a row of padding only, whatever its length says
    assert table["dst_off"].tolist() == dst
    tiles = (70001 - 1 + 7) // COLLATE_TILE + 1
    assert shim.cs_tiles(70001, F16) == tiles
    # {ticket, floats the arena must hold, elements of out, work items}: the sources of the row of no samples (at 2^40 ...) do not count,
    # nor does a row without sources
    assert info.tolist() == [0, 20000 + 70001, 4 * 70001, 4 * tiles]
    st, info, table, _, msg = plan(shim, [0, 1, 3], [5, 6, 7], [8, 9], None, 9)  # NULL destination offsets: 0 for every row
    assert st == OK and table["dst_off"].tolist() == [0, 0] and info.tolist() == [0, 16, 18, 2], msg


def test_the_arena_need_counts_only_sources_that_are_read(shim):
    st, info, _, _, msg = plan(shim, [0, 0, 0], [], [100, 5], None, 100)  # k = 0 everywhere: nothing of the arena is needed
    assert st == OK and info.tolist() == [0, 0, 200, 2], msg
    st, info, _, _, msg = plan(shim, [0, 2, 4], [2 ** 50, 2 ** 51, 10, 30], [0, 7], [5, 0], 8)  # len = 0: its sources do not count
    assert st == OK and info.tolist() == [0, 37, 16, 2], msg
    st, info, _, _, msg = plan(shim, [0], [], [], None, 100)  # no rows: a plan whose run launches nothing
    assert st == OK and info.tolist() == [0, 0, 0, 0], msg
    st, info, _, _, msg = plan(shim, [0, 1, 2], [0, 0], [0, 0], None, 0)  # rows of no elements: nothing to launch either
    assert st == OK and info.tolist() == [0, 0, 0, 0], msg
    st, info, _, _, msg = plan(shim, [0, 2], [2 ** 31 + 1, 2 ** 40], [4099], [2 ** 33], 2 ** 33 + 4099, BF16)  # offsets past 2^31 travel unchanged
    assert st == OK and info.tolist() == [0, 2 ** 40 + 4099, 2 ** 33 + 4099, (2 ** 33 + 4099 - 1 + 7) // COLLATE_TILE + 1], msg


def test_plan_time_errors_are_decided_on_the_host(shim):
    def refused(*a, **k):
        st, info, _, _, msg = plan(shim, *a, **k)
        assert (st == INVALID and msg and info.tolist() == [POISON] * 4) or st == OK, (st, msg)  # a refusal plans nothing
        return st == INVALID

    assert not refused([0, 2], [0, 8], [8], [0], 8)
    assert refused([1, 2], [0, 8], [8], [0], 8)  # h_first does not start at 0
    assert refused([0, 2, 1], [0, 8], [4, 4], None, 8)  # h_first decreases
    assert refused([0, 2], [0, -1], [8], [0], 8) and refused([0, 2], [-1, 0], [8], [0], 8)  # a negative source offset
    assert refused([0, 2], [-1, 0], [0], [0], 8)  # ... also where the row has no samples
    assert refused([0, 2], [0, 8], [8], [-1], 16)  # a negative destination offset
    assert refused([0, 2], [0, 8], [-1], [0], 8)  # a negative length
    assert refused([0, 1], [0], [0], [0], -1) and refused([0], [], [], [], -1)  # row_len < 0
    assert refused([0, 2], [0, 8], [8], [1], 8) and refused([0, 2], [0, 9], [9], [0], 8)  # the row does not fit row_len
    assert refused([0, 0], [], [9], [0], 8)  # ... also a row without sources
    assert not refused([0, 1, 3], [0, 0, 4], [8, 4], [0, 4], 8)  # dst_off + len == row_len is a full row
    assert refused([0, 1], [0], [1], [I64_MAX], I64_MAX)  # (the comparison itself must not overflow)
    assert refused([0, 0, 0, 0], [], [0, 0, 0], None, 2 ** 62)  # rows * row_len beyond INT64_MAX
    assert not refused([0, 1], [0], [0], None, I64_MAX)
    assert refused([0, 2], [0, I64_MAX - 3], [4], [0], 8) and not refused([0, 2], [0, I64_MAX - 4], [4], [0], 8)  # src_off + len beyond INT64_MAX
    for bad in (-1, 3, 7):
        assert refused([0, 1], [0], [8], [0], 8, out_type=bad)  # an unknown output type
    for ok in (F32, F16, BF16):
        assert not refused([0, 1], [0], [8], [0], 8, out_type=ok)
    assert refused([0], [], [], [], 8, rows=-1)
    st, _, _, _, msg = plan(shim, [0, 1, 3], [0, 5, 6], [8, 9], [0, 0], 8)
    assert st == INVALID and "row 1" in msg and "do not fit" in msg


def test_a_row_of_33_sources_is_unsupported(shim):
    for k, want in ((32, OK), (33, UNSUPPORTED), (64, UNSUPPORTED), (65, UNSUPPORTED)):
        st, info, table, _, msg = plan(shim, [0, 1, 1 + k], np.arange(1 + k) * 16, [8, 8], None, 8)
        assert st == want, (k, st, msg)
        if want == OK:
            assert shim.cs_num_sources(int(table["pad"][1])) == 32 and shim.cs_first_source(int(table["pad"][1])) == 1
        else:
            assert info.tolist() == [POISON] * 4 and "at most 32" in msg  # nothing is planned


def test_a_17th_plan_while_16_are_outstanding_is_refused(shim):
    """The ring is the one of hipfeat_collate_plan: tickets of either form count towards the 16."""
    shim.cs_slots_reset()
    assert [shim.cs_slots_plan() for _ in range(16)] == list(range(16))
    assert shim.cs_slots_plan() == -1 and shim.cs_slots_plan() == -1  # refused, and nothing planned
    assert shim.cs_slots_run(16) == INVALID and shim.cs_slots_run(-1) == INVALID  # unknown tickets
    assert shim.cs_slots_run(5) == OK and shim.cs_slots_plan() == -1  # the slot ticket 16 would take (0) is still planned
    assert shim.cs_slots_run(0) == OK and shim.cs_slots_run(0) == INVALID  # a ticket runs once
    assert shim.cs_slots_plan() == 16 and shim.cs_slots_run(16) == OK


def test_the_python_layout_refuses_what_the_plan_refuses():
    fi, so, sl, do, row_len = collate_sources_layout(100, [0, 2, 2, 3], [0, 50, 10], [40, 7, 0])
    assert (fi.tolist(), so.tolist(), sl.tolist(), do.tolist(), row_len) == ([0, 2, 2, 3], [0, 50, 10], [40, 7, 0], [0, 0, 0], 40)
    assert collate_sources_layout(0, [0], [], [])[4] == 0  # no rows
    collate_sources_layout(10, [0, 1], [2 ** 40], [0], 8)  # a row of no samples reads nothing
    for bad in (dict(first=[1, 2], src_offsets=[0, 0], lengths=[4]), dict(first=[0, 2, 1], src_offsets=[0, 0], lengths=[4, 4]),
                dict(first=[0, 1], src_offsets=[0, 0], lengths=[4]), dict(first=[0, 1], src_offsets=[-1], lengths=[4]),
                dict(first=[0, 1], src_offsets=[0], lengths=[-4]), dict(first=[0, 1], src_offsets=[0], lengths=[4], row_len=3),
                dict(first=[0, 1], src_offsets=[0], lengths=[4], dst_offsets=[1], row_len=4), dict(first=[0, 1], src_offsets=[97], lengths=[4]),
                dict(first=[0, 33], src_offsets=[0] * 33, lengths=[4]), dict(first=[0, 1], src_offsets=[0], lengths=[4, 4])):
        with pytest.raises(ValueError):
            collate_sources_layout(100, **bad)


def test_stand_alone_program_of_the_shim(tmp_path):
    exe = str(tmp_path / "cosrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DCOLLATE_SOURCES_MAIN", SHIM, "-o", exe])
    # (bounds and overflow are what is looked for; the leak check at exit needs ptrace, which not every container grants)
    res = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
