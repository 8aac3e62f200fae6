"""CPU: what ``hipfeat_stats_update`` decides on the host -- the cut table the kernels read and every refusal with its status -- is
csrc/stats_tables.hpp, checked here through tests/native/stats_tables_capi.cpp (plain g++, ctypes) without a device."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from lhotse_amd import _lib

SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "stats_tables_capi.cpp")
OK, INVALID, UNSUPPORTED = 0, 1, 3
POISON = -12345
CUT_DTYPE = np.dtype([("first_elem", "<i8"), ("frames", "<i4"), ("block_first", "<i4")])
F32, F16 = 0, 1


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(tempfile.mkdtemp(prefix="sttab_"), "libsttab.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", out])
    lib = ctypes.CDLL(out)
    lib.st_plan.restype = ctypes.c_int
    lib.st_plan.argtypes = [ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p,
                            ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    for name in ("st_blocks_of", "st_tiles_of"):
        getattr(lib, name).restype = ctypes.c_longlong
    lib.st_blocks_of.argtypes = [ctypes.c_longlong]
    lib.st_tiles_of.argtypes = [ctypes.c_longlong, ctypes.c_int]
    return lib


def plan(shim, F, frames, first=None, stride=None, elems=None, dtype=F32, base=4096, cuts=None):
    """-> (status, info, cut table, message); ``info`` and the table are pre-filled with POISON so that "plans nothing" can be seen."""
    frames = None if frames is None else _lib.i64(frames)
    first = None if first is None else _lib.i64(first)
    stride = F if stride is None else stride
    n = len(frames) if cuts is None else cuts
    if elems is None:
        rows = int(frames.sum()) if first is None else int((first + frames).max())
        elems = max(rows - 1, 0) * stride + F
    info, msg = np.full(6, POISON, np.int64), ctypes.create_string_buffer(256)
    table = np.zeros(max(n, 1), CUT_DTYPE)
    table["frames"] = POISON
    st = shim.st_plan(F, base, elems, dtype, n, _lib.addr(first), _lib.addr(frames), stride, info.ctypes.data, table.ctypes.data, ctypes.addressof(msg))
    return st, info, table[: max(n, 0)], msg.value.decode()


def test_the_table_is_what_the_kernels_read(shim):
    assert CUT_DTYPE.itemsize == 16
    B = shim.st_block_frames()
    assert B == 256 and shim.st_row_lanes() * shim.st_col_lanes() == 256 and B % shim.st_row_lanes() == 0
    assert shim.st_max_cuts() == 65535 and shim.st_max_dim() == 65535
    # block counts around the block size; a cut of no frames has none
    assert [shim.st_blocks_of(t) for t in (0, 1, B - 1, B, B + 1, 3 * B + 5)] == [0, 1, 1, 1, 2, 4]
    # a lane owns 4 float32 or 8 binary16 bins: tiles of 64 / 128 bins
    assert [shim.st_tiles_of(f, F32) for f in (1, 64, 65, 257)] == [1, 1, 2, 5] and [shim.st_tiles_of(f, F16) for f in (1, 128, 129, 257)] == [1, 1, 2, 3]
    frames = [1, 2, B - 1, 0, B, B + 1, 3 * B + 5]
    st, info, table, msg = plan(shim, 80, frames)
    assert st == OK, msg
    blocks = [1, 1, 1, 0, 1, 2, 4]
    assert info.tolist() == [sum(frames), sum(blocks), 2, 2 * sum(blocks), 1, 80]
    assert table["frames"].tolist() == frames and table["block_first"].tolist() == np.concatenate([[0], np.cumsum(blocks)[:-1]]).tolist()
    assert table["first_elem"].tolist() == (np.concatenate([[0], np.cumsum(frames)[:-1]]) * 80).tolist()  # packed back to back
    # a padded batch: rows in descending order, a stride with a gap; 16-byte loads only where base and stride allow them
    st, info, table, msg = plan(shim, 80, [5, 0, 7], first=[20, 10, 0], stride=84)
    assert st == OK and table["first_elem"].tolist() == [20 * 84, 10 * 84, 0] and info.tolist() == [12, 2, 2, 4, 1, 84], msg
    assert plan(shim, 80, [5], stride=81)[1][4] == 0 and plan(shim, 80, [5], base=4100)[1][4] == 0 and plan(shim, 80, [5], base=4112)[1][4] == 1
    assert plan(shim, 80, [5], stride=88, dtype=F16)[1][4] == 1 and plan(shim, 80, [5], stride=84, dtype=F16)[1][4] == 0
    assert plan(shim, 80, [5], dtype=F16, base=4098)[0] == OK and plan(shim, 80, [5], dtype=F16, base=4098)[1][4] == 0
    # only cuts of no frames: a plan without work
    assert plan(shim, 3, [0, 0])[1].tolist() == [0, 0, 1, 0, 0, 3]


def test_offsets_past_2_40_travel_unchanged(shim):
    far = (2 ** 40) // 80 + 3
    st, info, table, msg = plan(shim, 80, [77, 3], first=[far, 2 ** 31 // 80 + 1], dtype=F16)
    assert st == OK and table["first_elem"].tolist() == [far * 80, (2 ** 31 // 80 + 1) * 80] and table["first_elem"][0] > 2 ** 40, msg


def test_every_refusal_has_its_status_and_plans_nothing(shim):
    def refused(status=INVALID, word="", **kw):
        args = dict(F=4, frames=[8])
        args.update(kw)
        st, info, table, msg = plan(shim, **args)
        assert st == status and msg and word in msg, (st, msg)
        assert info.tolist() == [POISON] * 6 and (table["frames"] == POISON).all()  # the output is as it was
        return True

    assert plan(shim, 4, [8])[0] == OK
    assert refused(frames=[8, -1], elems=1000, word="negative") and refused(frames=[8], first=[-1], elems=1000, word="negative")  # negative frames, negative rows
    assert refused(stride=3, elems=1000, word="shorter than a frame")  # stride < F
    assert refused(elems=8 * 4 - 1, word="reach beyond") and plan(shim, 4, [8], elems=8 * 4)[0] == OK  # the last element
    assert refused(frames=[8], first=[1], stride=6, elems=8 * 6 + 4 - 1, word="reach beyond") and plan(shim, 4, [8], first=[1], stride=6, elems=8 * 6 + 4)[0] == OK
    assert refused(frames=[1], first=[2 ** 62], elems=2 ** 62, word="reach beyond")  # (no overflow on the way)
    assert refused(frames=[0], first=[2 ** 62], stride=7, elems=10, word="out of range")
    assert refused(frames=[2 ** 31], elems=2 ** 40, word="out of range")
    assert refused(dtype=2, word="element type") and refused(dtype=-1, word="element type")
    assert refused(base=4098, word="not aligned") and refused(base=4097, dtype=F16, word="not aligned")  # the base pointer breaks the element alignment
    assert refused(F=0, word="bins") and refused(F=65536, frames=[1], word="bins") and plan(shim, 65535, [1])[0] == OK
    assert refused(frames=[], cuts=0, word="1 ... 65535") and refused(frames=[1] * 65536, word="1 ... 65535") and plan(shim, 4, [1] * 65535)[0] == OK
    assert refused(frames=None, cuts=1, elems=10, word="NULL") and refused(elems=-1, word="elements")
    # too much for one launch: more than 2^24 blocks
    assert refused(status=UNSUPPORTED, frames=[2 ** 29] * 9, elems=2 ** 40, word="split it")


def test_stand_alone_program_of_the_shim(tmp_path):
    exe = str(tmp_path / "sttab")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSTATS_TABLES_MAIN", SHIM, "-o", exe])
    # (bounds and overflow are what is looked for; the leak check at exit needs ptrace, which not every container grants)
    res = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
