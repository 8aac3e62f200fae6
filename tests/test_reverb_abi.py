"""CPU: the reverb entry points (ABI v7 on) are declared in the header, mirrored in ``_lib._SIGNATURES`` and exported by the built library
(its symbol table; no device is touched), and the host-only parts of the Python layer follow their rules; the plan -- the table and every
plan-time error -- is what csrc/reverb_tables.hpp decides, checked here through tests/native/reverb_tables_capi.cpp without a device."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from lhotse_amd import _lib, build

from test_abi import HEADER, declared_functions

REVERB_API = {"hipfeat_reverb_create", "hipfeat_reverb_destroy", "hipfeat_reverb_plan", "hipfeat_reverb_run"}
SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "reverb_tables_capi.cpp")
OK, INVALID = 0, 1
ITEM_DTYPE = np.dtype([("src_off", "<i8"), ("rir_off", "<i8"), ("out_off", "<i8"), ("n", "<i4"), ("taps", "<i4"), ("shift", "<i4"), ("item_first", "<i4"),
                       ("normalize", "<i4"), ("pad", "<i4")])
POISON = -0x5A5A5A5A


def test_reverb_entry_points_are_declared_mirrored_and_exported():
    names = set(declared_functions())
    assert REVERB_API <= names and REVERB_API <= set(_lib._SIGNATURES)
    assert names == set(_lib._SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    assert REVERB_API <= set(re.findall(r" T (hipfeat_\w+)", out))


def test_abi_version_agrees_everywhere_and_knows_the_reverb():
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version")
    assert header >= 7  # the reverb entry points arrived with version 7


def test_prototypes_match_the_signature_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(REVERB_API):
        proto = re.search(r"HIPFEAT_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert args == _lib._SIGNATURES[name][1], (name, args)


def test_the_library_links_the_hip_runtime_only():
    out = subprocess.run(["readelf", "-d", str(build.build())], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", out)
    assert any(n.startswith("libamdhip64") for n in needed)
    assert not [n for n in needed if re.match(r"lib(hipfft|rocfft|rocblas|hipblas|MIOpen)", n)], needed


def test_tail_floats_scaling_and_items_follow_their_rules():
    from lhotse_amd.augmentation import HipReverbWithImpulseResponse, reverb_items, reverb_tail_floats, scaled_rir

    assert reverb_tail_floats([1, 4, 5, 4097]) == 4 + 4 + 8 + 4100 + 3
    assert isinstance(reverb_tail_floats([7]), int) and reverb_tail_floats([]) == 3
    rir = np.array([3, -32768, 32767, 5, 32767], dtype=np.float32) / np.float32(32768.0)
    hs, shift = scaled_rir(rir)
    assert hs.dtype == np.float32 and shift == 2  # the first index of the maximum of the VALUES (np.argmax), not of the magnitudes
    assert np.array_equal(hs.astype(np.float64), rir.astype(np.float64) * 2.0 ** -15)  # the scaling is exact
    # the four cases of the reference (mono / multi-channel input x mono / multi-channel RIR) as (input channel, rir channel) items
    assert reverb_items(1, 1) == [(0, 0)]
    assert reverb_items(1, 3) == [(0, 0), (0, 1), (0, 2)]
    assert reverb_items(2, 1) == [(0, 0), (1, 0)]
    assert reverb_items(2, 2) == [(0, 0), (1, 1)]
    with pytest.raises(ValueError):
        reverb_items(2, 3)
    with pytest.raises(ValueError):
        reverb_items(1, 2, rir_given=False)
    with pytest.raises(_lib.HipFeatError) as e:
        HipReverbWithImpulseResponse(rir=None)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    tf = HipReverbWithImpulseResponse(rir=np.zeros((2, 8), np.float32), rir_channels=[1], early_only=True)
    assert tf.reverse_timestamps(0.25, 1.5, 16000) == (0.25, 1.5) and tf.reverse_timestamps(0.0, None, None) == (0.0, None)
    assert type(tf).__name__ in type(tf).KNOWN_TRANSFORMS or "HipReverbWithImpulseResponse" in tf.KNOWN_TRANSFORMS


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(tempfile.mkdtemp(prefix="rvtab_"), "librvtab.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", out])
    lib = ctypes.CDLL(out)
    lib.rt_plan.restype = ctypes.c_int
    lib.rt_plan.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 6 + [ctypes.c_longlong] + [ctypes.c_void_p] * 4
    return lib


def plan(shim, src_offsets, src_lens, rir_offsets, rir_lens, shifts, normalize=None, tail_start=0):
    """The arguments of ``HipReverb.plan`` -> (status, info, out_offsets, items, message); the outputs start as POISON."""
    so, sl, ro, rl, sh = (_lib.i64(a) for a in (src_offsets, src_lens, rir_offsets, rir_lens, shifts))
    n = len(so)
    nm = np.ascontiguousarray(np.zeros(n) if normalize is None else normalize, dtype=np.int32)
    info, offs, items, msg = np.full(4, POISON, np.int64), np.full(n, POISON, np.int64), np.zeros(n, ITEM_DTYPE), ctypes.create_string_buffer(256)
    st = shim.rt_plan(n, *(a.ctypes.data for a in (so, sl, ro, rl, sh, nm)), int(tail_start), offs.ctypes.data, info.ctypes.data, items.ctypes.data,
                      ctypes.addressof(msg))
    return st, info, offs, items, msg.value.decode()


def test_the_table_is_what_the_kernels_read(shim):
    assert ITEM_DTYPE.itemsize == 48 and (shim.rt_block(), shim.rt_lane()) == (2048, 8)
    src, lens, rir, taps, shifts = [0, 100, 5000], [100, 4097, 2048], [10000, 10020, 10000], [20, 300, 20], [3, 299, 0]
    st, info, offs, items, msg = plan(shim, src, lens, rir, taps, shifts, [1, 0, 7], 10321)
    assert st == OK, msg
    assert items["src_off"].tolist() == src and items["n"].tolist() == lens and items["rir_off"].tolist() == rir and items["taps"].tolist() == taps
    assert items["shift"].tolist() == shifts and items["normalize"].tolist() == [1, 0, 1] and items["pad"].tolist() == [0, 0, 0]
    assert items["item_first"].tolist() == [0, 1, 4]  # 2048 outputs per work item: 1, 3 and 1 of them
    assert offs.tolist() == [10324, 10424, 10424 + 4100] == items["out_off"].tolist()  # (each on a 16-byte boundary behind tail_start)
    assert info.tolist() == [0, 10424 + 4100 + 2048, 5, 10]


def test_plan_time_errors_are_decided_on_the_host(shim):
    """The refusals of tests/test_gpu_reverb.py::test_plan_refuses_bad_tables_and_a_ticket_runs_once, with its table; a refusal writes no
    output."""
    good = dict(src_offsets=[0], src_lens=[100], rir_offsets=[100], rir_lens=[20], shifts=[3], normalize=[1], tail_start=120)

    def refused(**kw):
        st, info, offs, _, msg = plan(shim, **{**good, **kw})
        assert st == INVALID and msg and (info == POISON).all() and (offs == POISON).all(), (kw, st, msg)
        return msg

    assert plan(shim, **good)[0] == OK
    refused(src_offsets=[-1])
    refused(rir_offsets=[-4])
    refused(src_lens=[0])
    refused(rir_lens=[0])
    refused(shifts=[-1])
    assert "shift 20 outside [0, 20)" in refused(shifts=[20])
    assert "reaches into the arena's tail" in refused(tail_start=119)  # the impulse response reaches past tail_start
    refused(src_offsets=[21], rir_offsets=[0])  # the source does
    assert "tail_start -4 is negative" in refused(tail_start=-4)
    # ... and the ones no GPU test reaches
    refused(src_offsets=[], src_lens=[], rir_offsets=[], rir_lens=[], shifts=[], normalize=[])  # no items
    refused(src_lens=[2 ** 30], tail_start=2 ** 31)
    assert plan(shim, [2 ** 33], [2 ** 30 - 1], [0], [20], [3], None, 2 ** 34)[0] == OK  # INT32_MAX / 2 samples, behind 2^31


def test_stand_alone_program_of_the_shim(tmp_path):
    exe = str(tmp_path / "rvtab")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DREVERB_TABLES_MAIN", SHIM, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
