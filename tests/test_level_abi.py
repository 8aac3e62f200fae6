"""CPU: the level entry points (additive to ABI v8) are declared in the header, mirrored in ``_lib._LEVEL_SIGNATURES`` and exported by the built
library (its symbol table; no device is touched); the plan -- the table and every plan-time error -- is what csrc/level_tables.hpp
decides, checked here through tests/native/level_tables_capi.cpp without a device; the host-only parts of the Python layer agree with
the rule of tests/_level_ref.py."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from lhotse_amd import _lib, build, constants
from lhotse_amd.augmentation import LEVEL_MAX_OPS, level_op_tables

import _level_ref
from test_abi import HEADER, declared_functions

LEVEL_API = {"hipfeat_level_create", "hipfeat_level_destroy", "hipfeat_level_plan", "hipfeat_level_run"}
SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "level_tables_capi.cpp")
OK, INVALID, UNSUPPORTED = 0, 1, 3
ITEM_DTYPE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("len", "<i4"), ("item_first", "<i4"), ("nops", "<i4"), ("clip_at", "<i4"),
                       ("op", "<i4", 4), ("value", "<f4", 4)])
BLOCK = 4096


def test_level_entry_points_are_declared_mirrored_and_exported():
    """Additive to v8: they carry their own export macro in the header and their own table in ``_lib``, so that the v8 set -- which older
    tests count -- stays what it was."""
    declared = set(re.findall(r"HIPFEAT_LEVEL_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\(", open(HEADER).read()))
    assert declared == LEVEL_API == set(_lib._LEVEL_SIGNATURES)
    assert set(declared_functions()) == set(_lib._SIGNATURES) and not LEVEL_API & set(_lib._SIGNATURES)
    assert all(callable(_lib.load().fn(name)) for name in LEVEL_API)  # ... and the loaded library binds them
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    assert LEVEL_API <= set(re.findall(r" T (hipfeat_\w+)", out))


def test_the_abi_version_is_still_8():
    text = open(HEADER).read()
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", text).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version") == 8
    assert "v8 libraries built from this commit on also carry hipfeat_level_*" in text


def test_prototypes_match_the_signature_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(LEVEL_API):
        proto = re.search(r"HIPFEAT_LEVEL_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert _lib._LEVEL_SIGNATURES[name] == ("int", args), (name, args)


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(tempfile.mkdtemp(prefix="lvtab_"), "liblvtab.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", out])
    lib = ctypes.CDLL(out)
    lib.lt_plan.restype = ctypes.c_int
    lib.lt_plan.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 10
    lib.lt_silence_peak.restype = ctypes.c_float
    lib.lt_block.restype = ctypes.c_int
    return lib


def plan(shim, src, lens, programs, dst=None, raw_ops=None):
    """-> (status, info, items, message); raw_ops = (first, kind, value, flags) overrides the programs."""
    so, sl = _lib.i64(src), _lib.i64(lens)
    do = so if dst is None else _lib.i64(dst)
    first, kind, value, flags = raw_ops if raw_ops is not None else level_op_tables(programs)
    first, kind = _lib.i64(first), np.ascontiguousarray(kind, np.int32)
    value, flags = np.ascontiguousarray(value, np.float32), np.ascontiguousarray(flags, np.int32)
    info, items, msg = np.zeros(4, np.int64), np.zeros(len(so), ITEM_DTYPE), ctypes.create_string_buffer(256)
    st = shim.lt_plan(len(so), *(a.ctypes.data for a in (so, sl, do, first, kind, value, flags, info)), items.ctypes.data, ctypes.addressof(msg))
    return st, info, items, msg.value.decode()


VOL, CLIP = ("volume", 0.5), ("clip", True, 0.0, True)


def test_the_table_is_what_the_kernels_read(shim):
    assert ITEM_DTYPE.itemsize == 64 and shim.lt_block() == BLOCK
    src, lens = [0, 4099, 9001, 100000], [4096, 4094, 70001, 1]
    programs = [[VOL], [CLIP], [("volume", -1.5), ("clip", False, 20.0, False), ("volume", 2.0)], [("clip", False, 0.05, True)]]
    st, info, items, msg = plan(shim, src, lens, programs, dst=[0, 4099, 200000, 100000])
    assert st == OK, msg
    blocks = [((s & 3) + n + BLOCK - 1) // BLOCK for s, n in zip(src, lens)]
    assert blocks == [1, 2, 18, 1]  # (4099 & 3 = 3: 3 + 4094 = 4097 samples from the boundary: 2 tiles)
    assert items["item_first"].tolist() == [0, 1, 3, 21] and items["nops"].tolist() == [1, 1, 3, 1] and items["clip_at"].tolist() == [-1, 0, 1, 0]
    assert items["src_off"].tolist() == src and items["dst_off"].tolist() == [0, 4099, 200000, 100000] and items["len"].tolist() == lens
    assert info.tolist() == [0, 270001, 2 + 18 + 1, 22]
    # kind | flags << 8: hard 1, normalize 2, use-gain 4 (|gain_db| >= 0.1); g = (float)10**(gain_db / 20)
    assert items["op"][2].tolist() == [0, 1 | (4 << 8), 0, 0] and items["op"][1][0] == 1 | (3 << 8) and items["op"][3][0] == 1 | (2 << 8)
    assert items["value"][2].tolist() == [np.float32(-1.5), np.float32(10.0), np.float32(2.0), 0.0]
    assert items["value"][3][0] == np.float32(10 ** (0.05 / 20.0))


def test_plan_time_errors_are_decided_on_the_host(shim):
    def status(*a, **k):
        return plan(shim, *a, **k)[0]

    assert status([0], [1], [[VOL]]) == OK
    assert status([0], [0], [[VOL]]) == INVALID and status([0], [-3], [[CLIP]]) == INVALID  # np.max of nothing raises in the reference
    assert status([0], [8], [[]]) == INVALID  # a program of 0 ops
    assert status([0], [8], [[VOL] * LEVEL_MAX_OPS]) == OK and status([0], [8], [[VOL] * (LEVEL_MAX_OPS + 1)]) == INVALID
    assert status([0], [8], [[CLIP, VOL, CLIP]]) == UNSUPPORTED  # two CLIPs in a program
    assert status([-1], [8], [[VOL]]) == INVALID and status([0], [8], [[VOL]], dst=[-4]) == INVALID
    # a destination: its source (in place) or away from it, never across it
    assert status([16], [8], [[VOL]], dst=[16]) == OK and status([16], [8], [[VOL]], dst=[24]) == OK and status([16], [8], [[VOL]], dst=[8]) == OK
    assert status([16], [8], [[VOL]], dst=[23]) == INVALID and status([16], [8], [[VOL]], dst=[9]) == INVALID
    # ... nor across another item's source or destination
    assert status([0, 8], [8, 8], [[VOL], [VOL]]) == OK
    assert status([0, 7], [8, 8], [[VOL], [VOL]]) == INVALID
    assert status([0, 100], [8, 8], [[VOL], [VOL]], dst=[50, 57]) == INVALID
    assert status([0, 100], [8, 8], [[VOL], [VOL]], dst=[50, 58]) == OK
    assert status([0, 100], [8, 8], [[VOL], [VOL]], dst=[104, 200]) == INVALID  # item 0 writes what item 1 reads
    assert status([0, 0], [8, 8], [[VOL], [VOL]], dst=[100, 200]) == OK  # two readers of one source
    # op tables
    assert status([0], [8], None, raw_ops=([0, 1], [2], [1.0], [0])) == INVALID  # unknown kind
    assert status([0], [8], None, raw_ops=([0, 1], [0], [1.0], [1])) == INVALID  # SCALE takes no flags
    assert status([0], [8], None, raw_ops=([0, 1], [1], [1.0], [8])) == INVALID  # unknown CLIP flag
    assert status([0], [8], None, raw_ops=([0, 1], [1], [0.0], [4])) == INVALID and status([0], [8], None, raw_ops=([0, 1], [1], [np.inf], [4])) == INVALID
    assert status([0], [8], None, raw_ops=([1, 2], [0, 0], [1.0, 1.0], [0, 0])) == INVALID  # op_first[0] != 0
    st, info, _, msg = plan(shim, [0], [0], [[VOL]])
    assert "item 0" in msg and "1 ..." in msg


def test_offsets_past_2_31_travel_unchanged_and_overlaps_up_there_are_seen(shim):
    """64-bit offsets: nothing of the table or of the overlap checks may pass through an int (tests/test_gpu_large_offsets.py runs the
    kernels on such tables)."""
    far, farther = 2 ** 31 + 1, 2 ** 40
    st, info, items, msg = plan(shim, [far, farther, 5], [4099, 70001, 8], [[VOL], [CLIP], [VOL]], dst=[far, farther + 70001, far + 4099])
    assert st == OK, msg
    assert items["src_off"].tolist() == [far, farther, 5] and items["dst_off"].tolist() == [far, farther + 70001, far + 4099]
    assert items["len"].tolist() == [4099, 70001, 8] and items["item_first"].tolist() == [0, 2, 20]  # (far & 3 = 1: 1 + 4099 samples: 2 tiles)
    assert info.tolist() == [0, farther + 2 * 70001, 18, 21]
    # the same refusals as for small offsets (test_plan_time_errors_are_decided_on_the_host), with every range behind 2^31 / 2^40
    for base in (far, farther):
        assert plan(shim, [base, base + 8], [8, 8], [[VOL], [VOL]])[0] == OK
        st, _, _, msg = plan(shim, [base, base + 7], [8, 8], [[VOL], [VOL]])
        assert st == INVALID and "overlap" in msg, msg
        assert plan(shim, [base], [8], [[VOL]], dst=[base + 7])[0] == INVALID and plan(shim, [base], [8], [[VOL]], dst=[base + 8])[0] == OK
        assert plan(shim, [0, base], [8, 8], [[VOL], [VOL]], dst=[base + 4, 2 * base])[0] == INVALID  # item 0 writes what item 1 reads
        assert plan(shim, [base, base + 2 ** 32], [8, 8], [[VOL], [VOL]])[0] == OK  # equal lower dwords are not an overlap
    assert plan(shim, [0], [2 ** 30], [[VOL]])[0] == INVALID and plan(shim, [farther], [2 ** 30 - 1], [[VOL]])[0] == OK  # INT32_MAX / 2 samples


def test_zero_items_plan_nothing_to_launch(shim):
    st, info, items, msg = plan(shim, [], [], [])
    assert st == OK and info.tolist() == [0, 0, 0, 0]


def test_stand_alone_program_of_the_shim(tmp_path):
    exe = str(tmp_path / "lvtab")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DLEVEL_TABLES_MAIN", SHIM, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr


def test_the_silence_threshold_is_one_number_everywhere(shim):
    assert constants.SILENCE_PEAK.dtype == np.float32
    assert np.float32(shim.lt_silence_peak()) == constants.SILENCE_PEAK == _level_ref.SILENCE_PEAK
    assert "p < 0x1.09e69ep-16" in open(HEADER).read()


def test_op_tables_follow_the_rule():
    first, kind, value, flags = level_op_tables([[("volume", 1.25)], [("clip", True, -6.0, False), ("volume", -3)], []])
    assert first.tolist() == [0, 1, 3, 3] and kind.tolist() == [0, 1, 0] and flags.tolist() == [0, 1 | 4, 0]
    g, use = _level_ref.gain_of(-6.0)
    assert use and value.tolist() == [np.float32(1.25), g, np.float32(-3)] and value.dtype == np.float32
    for gain_db, use in ((0.0, False), (0.05, False), (-0.0999, False), (0.1, True), (-0.1, True), (20.0, True)):
        assert bool(level_op_tables([[("clip", False, gain_db, True)]])[3][0] & 4) is use
    with pytest.raises(ValueError):
        level_op_tables([[("tempo", 1.1)]])
