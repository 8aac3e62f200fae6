"""CPU: the FFT route of the reverb (hipfeat_reverb_plan_method, additive to ABI v8) is declared in the header with its contract, mirrored
in ``_lib._SIGNATURES`` and exported by the built library; the plan -- both tables, the workspace and every plan-time error -- is what
csrc/reverb_fft_tables.hpp decides, checked here through tests/native/reverb_fft_tables_capi.cpp without a device; the Python layer's
sizes, keywords and dict round trip follow their rules."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from lhotse_amd import _lib, build
from lhotse_amd import augmentation as A
from lhotse_amd import input_strategies as IS

from test_abi import HEADER, declared_functions
from test_reverb_abi import ITEM_DTYPE as DIRECT_DTYPE
from test_reverb_abi import SHIM as DIRECT_SHIM
from test_reverb_abi import plan as direct_plan

SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "reverb_fft_tables_capi.cpp")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lhotse_amd", "csrc")
OK, INVALID = 0, 1
POISON = -0x5A5A5A5A
FFT_DTYPE = np.dtype([("src_off", "<i8"), ("out_off", "<i8"), ("hspec_off", "<i8"), ("xspec_off", "<i8"), ("n", "<i4"), ("taps", "<i4"), ("shift", "<i4"),
                      ("parts", "<i4"), ("nx", "<i4"), ("j0", "<i4"), ("ny", "<i4"), ("normalize", "<i4"), ("a_first", "<i4"), ("b_first", "<i4"),
                      ("g_first", "<i4"), ("pad", "<i4")])
RIR_DTYPE = np.dtype([("rir_off", "<i8"), ("spec_off", "<i8"), ("taps", "<i4"), ("parts", "<i4"), ("first", "<i4"), ("pad", "<i4")])
DIRECT, FFT, AUTO = 0, 1, 2


def test_the_entry_point_is_declared_mirrored_and_exported():
    name = "hipfeat_reverb_plan_method"
    raw = open(HEADER).read()
    # additive to v8: under an export macro of its own, outside the set the version number stands for
    assert set(re.findall(r"HIPFEAT_REVERB_FFT_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\(", raw)) == {name} == set(_lib._REVERB_FFT_SIGNATURES)
    assert re.search(r"#define\s+HIPFEAT_REVERB_FFT_API\s+HIPFEAT_API\b", raw)
    assert name in _lib._ADDED_SIGNATURES and name not in _lib._SIGNATURES and set(declared_functions()) == set(_lib._SIGNATURES)
    assert callable(_lib.load().fn(name))  # the loaded library binds it
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    proto = re.search(r"HIPFEAT_REVERB_FFT_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
    args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
    assert _lib._REVERB_FFT_SIGNATURES[name] == ("int", args)
    plain = _lib._SIGNATURES["hipfeat_reverb_plan"][1]
    assert args == plain[:9] + ["int32_t", "int64_t"] + plain[9:]  # the arguments of hipfeat_reverb_plan, method and min_fft_taps in front of the outputs
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    assert name in set(re.findall(r" T (hipfeat_\w+)", out))
    assert int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1)) == 8  # additive: the version number stays


def test_the_header_states_geometry_orders_and_the_workspace_formula():
    text = " ".join(re.sub(r"\n \*", "\n", open(HEADER).read()).split())  # (the comment's text without its line prefixes)
    block =text[text.index("partitioned FFT convolution, opt-in per plan") : text.index("HIPFEAT_REVERB_FFT_API hipfeat_status hipfeat_reverb_plan_method(hipfeat_reverb* reverb")]
    for needle in ("rir.py:78-153", "utils.py:49-75", "block B = 1024", "transform size 2 B = 2048", "P = ceil(L / 1024)", "p ASCENDING",
                   "fmaf(-h.im, x.im, fmaf(h.re, x.re, re))", "times 2^-11", "computed in float64 and rounded once", "Sx = the sum over i ascending", "Sy = the sum over j ascending",
                   "Workspace formula", "2048 x (sum of P over the DISTINCT", "transformed once", "method: 0 direct", "min_fft_taps", "h_info[8]",
                   "nothing is allocated per call"):
        assert needle in block, needle
    kernel = " ".join(re.sub(r"\n//", "\n", open(os.path.join(CSRC, "kernel_reverb_fft.hpp")).read()).split())
    for needle in ("rir.py:78-153", "utils.py:49-75", "ACCUMULATION ORDER", "p ascending", "wave_sum_f64", "No atomics"):
        assert needle in kernel, needle


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(tempfile.mkdtemp(prefix="rftab_"), "librftab.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", out])
    lib = ctypes.CDLL(out)
    lib.rf_plan.restype = ctypes.c_int
    lib.rf_plan.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 6 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong] + [ctypes.c_void_p] * 7
    return lib


@pytest.fixture(scope="module")
def direct_shim():
    """The shim of hipfeat_reverb_plan's table (tests/test_reverb_abi.py), to compare method 0 with."""
    out = os.path.join(tempfile.mkdtemp(prefix="rvtab_"), "librvtab.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", DIRECT_SHIM, "-o", out])
    lib = ctypes.CDLL(out)
    lib.rt_plan.restype = ctypes.c_int
    lib.rt_plan.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 6 + [ctypes.c_longlong] + [ctypes.c_void_p] * 4
    return lib


def plan(shim, src_offsets, src_lens, rir_offsets, rir_lens, shifts, normalize=None, tail_start=0, method=FFT, min_fft_taps=0):
    """-> (status, info[8], out_offsets, direct items, fft items, rirs, message); the outputs start as POISON."""
    so, sl, ro, rl, sh = (_lib.i64(a) for a in (src_offsets, src_lens, rir_offsets, rir_lens, shifts))
    n = len(so)
    if not (len(sl) == len(ro) == len(rl) == len(sh) == n):
        raise ValueError("one entry per item in every table")
    nm = np.ascontiguousarray(np.zeros(n) if normalize is None else normalize, dtype=np.int32)
    info, offs, counts = np.full(8, POISON, np.int64), np.full(n, POISON, np.int64), np.zeros(3, np.int64)
    direct, fft, rirs, msg = np.zeros(n, DIRECT_DTYPE), np.zeros(n, FFT_DTYPE), np.zeros(n, RIR_DTYPE), ctypes.create_string_buffer(256)
    st = shim.rf_plan(n, *(a.ctypes.data for a in (so, sl, ro, rl, sh, nm)), int(tail_start), int(method), int(min_fft_taps), offs.ctypes.data, info.ctypes.data,
                      direct.ctypes.data, fft.ctypes.data, rirs.ctypes.data, counts.ctypes.data, ctypes.addressof(msg))
    return st, info, offs, direct[: counts[0]], fft[: counts[1]], rirs[: counts[2]], msg.value.decode()


GOOD = dict(src_offsets=[0, 5000, 9100], src_lens=[5000, 4097, 100], rir_offsets=[10000, 13001, 10000], rir_lens=[3001, 20, 3001], shifts=[1025, 3, 3000],
            normalize=[1, 0, 1], tail_start=13021)


def test_the_tables_are_what_the_kernels_read(shim):
    assert (FFT_DTYPE.itemsize, RIR_DTYPE.itemsize) == (80, 32)
    assert (shim.rf_block(), shim.rf_spec_floats(), shim.rf_waves(), shim.rf_grid_slots()) == (1024, 2048, 4, 1792)
    st, info, offs, direct, fft, rirs, msg = plan(shim, **GOOD)
    assert st == OK and len(direct) == 0 and len(fft) == 3 and len(rirs) == 2, msg
    assert offs.tolist() == [13024, 13024 + 5000, 13024 + 5000 + 4100] == fft["out_off"].tolist()
    ws = 13024 + 5000 + 4100 + 100
    # items 0 and 2 share the impulse response at 10000: ONE set of 3 spectra; item 1's own has 1
    assert rirs["rir_off"].tolist() == [10000, 13001] and rirs["parts"].tolist() == [3, 1] and rirs["first"].tolist() == [0, 3]
    assert rirs["spec_off"].tolist() == [ws, ws + 3 * 2048] and fft["hspec_off"].tolist() == [ws, ws + 3 * 2048, ws]
    # item 0: outputs yf[1025, 6025) = blocks 1 ... 5, inputs x[-1024, 1024) ... = blocks 0 ... 5; item 1: blocks 0 ... 4, inputs 0 ... 4;
    # item 2: outputs yf[3000, 3100) = block 2 (then 3: 3100 > 3072), inputs 0 and 1 (block 1 holds no sample of x but block 2 reads it)
    assert fft["j0"].tolist() == [1, 0, 2] and fft["ny"].tolist() == [5, 5, 2] and fft["nx"].tolist() == [6, 5, 2] and fft["parts"].tolist() == [3, 1, 3]
    assert fft["a_first"].tolist() == [4, 10, 15] and fft["b_first"].tolist() == [0, 5, 10] and fft["g_first"].tolist() == [0, 3, 6]
    assert fft["xspec_off"].tolist() == [ws + 2048 * k for k in (4, 10, 15)]
    assert fft["normalize"].tolist() == [1, 0, 1] and fft["pad"].tolist() == [0, 0, 0] and rirs["pad"].tolist() == [0, 0]
    assert info.tolist() == [0, ws + 2048 * 17, 0, 13 + 12, 17, 12, 7, 2]


def test_info_sizes_equal_reverb_fft_tail_floats(shim):
    g = GOOD
    st, info, *_ = plan(shim, **g)
    aligned = (g["tail_start"] + 3) & ~3
    assert int(info[1]) == aligned + A.reverb_fft_tail_floats(g["src_lens"], g["rir_lens"], g["shifts"], g["rir_offsets"]) - 3
    # without the offsets every item counts an impulse response of its own: an upper bound (3 more spectra here)
    assert A.reverb_fft_tail_floats(g["src_lens"], g["rir_lens"], g["shifts"]) == int(info[1]) - aligned + 3 + 3 * 2048
    private = dict(g, rir_offsets=[10000, 13001, 10000 - 0], rir_lens=[3001, 20, 3000], shifts=[1025, 3, 2999])  # another length: another RIR
    st, info2, _, _, _, rirs, _ = plan(shim, **private)
    assert st == OK and len(rirs) == 3
    assert int(info2[1]) == aligned + A.reverb_fft_tail_floats(private["src_lens"], private["rir_lens"], private["shifts"], private["rir_offsets"]) - 3
    assert A.reverb_workspace_floats(g["src_lens"], g["rir_lens"], g["shifts"], g["rir_offsets"], "direct") == 0
    assert A.reverb_workspace_floats(g["src_lens"], g["rir_lens"], g["shifts"], g["rir_offsets"], "fft") == 17 * 2048
    assert A.reverb_workspace_floats(g["src_lens"], g["rir_lens"], g["shifts"], g["rir_offsets"], "auto", 21) == (3 + 6 + 2) * 2048
    assert A.reverb_workspace_floats(g["src_lens"], g["rir_lens"], g["shifts"], g["rir_offsets"], "auto") == 0 or A.REVERB_AUTO_MIN_TAPS <= 3001
    assert isinstance(A.reverb_fft_tail_floats([7], [1], [0]), int)


def test_method_direct_is_hipfeat_reverb_plan_and_auto_splits_at_the_threshold(shim, direct_shim):
    g = GOOD
    st0, info0, offs0, items0, msg0 = direct_plan(direct_shim, *(g[k] for k in ("src_offsets", "src_lens", "rir_offsets", "rir_lens", "shifts", "normalize", "tail_start")))
    st, info, offs, direct, fft, rirs, msg = plan(shim, **g, method=DIRECT)
    assert st == st0 == OK and info[:4].tolist() == info0.tolist() and info[4:].tolist() == [0, 0, 0, 0] and offs.tolist() == offs0.tolist()
    assert len(fft) == 0 and len(rirs) == 0 and direct.tobytes() == items0.tobytes()
    # auto with every impulse response under the threshold is the same plan
    st, info_a, offs_a, direct_a, fft_a, _, _ = plan(shim, **g, method=AUTO, min_fft_taps=3002)
    assert st == OK and info_a.tolist() == info.tolist() and direct_a.tobytes() == direct.tobytes() and len(fft_a) == 0
    # at 3001 the two long ones take the FFT route, the 20-tap one stays: one ticket, both tables, the same output offsets
    st, info_m, offs_m, direct_m, fft_m, rirs_m, _ = plan(shim, **g, method=AUTO, min_fft_taps=3001)
    assert st == OK and offs_m.tolist() == offs0.tolist() and len(direct_m) == 1 and len(fft_m) == 2 and len(rirs_m) == 1
    assert direct_m["src_off"].tolist() == [5000] and direct_m["item_first"].tolist() == [0] and direct_m["out_off"].tolist() == [offs0[1]]
    assert fft_m["src_off"].tolist() == [0, 9100] and fft_m["out_off"].tolist() == [offs0[0], offs0[2]]
    assert info_m.tolist() == [0, int(info0[1]) + 2048 * (3 + 6 + 2), 3, 2 * 3 + (8 + 7), 11, 7, 4, 1]


def test_plan_time_errors_are_decided_on_the_host(shim):
    def refused(**kw):
        st, info, offs, _, _, _, msg = plan(shim, **{**GOOD, **kw})
        assert st == INVALID and msg and (info == POISON).all() and (offs == POISON).all(), (kw, st, msg)
        return msg

    assert "method 3 is not" in refused(method=3)
    refused(method=-1)
    assert "min_fft_taps -1 is negative" in refused(method=AUTO, min_fft_taps=-1)
    refused(min_fft_taps=-5)  # (whatever the method)
    refused(shifts=[1025, 20, 3000])  # the refusals of hipfeat_reverb_plan, unchanged
    assert "reaches into the arena's tail" in refused(tail_start=13020)
    refused(src_lens=[5000, 0, 100])
    with pytest.raises(ValueError):  # unequal tables never reach the library: HipReverb.plan checks them first, as for the direct form
        plan(shim, **{**GOOD, "shifts": [0, 0]})
    src = inspect.getsource(A.HipReverb.plan)
    assert src.index("one entry per item in every table") < src.index('self.lib.check("hipfeat_reverb_plan_method"')
    with pytest.raises(ValueError):
        A.reverb_method_code("overlap-add")
    assert [A.reverb_method_code(m) for m in ("direct", "fft", "auto")] == [DIRECT, FFT, AUTO]


def test_stand_alone_program_of_the_shim(tmp_path):
    exe = str(tmp_path / "rftab")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DREVERB_FFT_TABLES_MAIN", SHIM, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr


def test_the_transform_omits_a_direct_method_and_round_trips_another():
    rir = np.zeros((1, 8), np.float32)
    today = {"name": "HipReverbWithImpulseResponse",
             "kwargs": {"rir": rir, "normalize_output": True, "early_only": False, "rir_channels": [0], "rir_generator": None, "device": "cuda"}}
    for tf in (A.HipReverbWithImpulseResponse(rir=rir), A.HipReverbWithImpulseResponse(rir=rir, method="direct")):
        d = tf.to_dict()
        assert d["name"] == today["name"] and list(d["kwargs"]) == list(today["kwargs"]) and "method" not in d["kwargs"]
        assert all(d["kwargs"][k] is today["kwargs"][k] or d["kwargs"][k] == today["kwargs"][k] for k in today["kwargs"] if k != "rir") and d["kwargs"]["rir"] is rir
    for method in ("fft", "auto"):
        tf = A.HipReverbWithImpulseResponse(rir=rir, method=method, normalize_output=False)
        d = tf.to_dict()
        assert d["kwargs"]["method"] == method and list(d["kwargs"])[:-1] == list(today["kwargs"])
        back = A.HipReverbWithImpulseResponse.from_dict(d) if hasattr(A.HipReverbWithImpulseResponse, "from_dict") else A.HipReverbWithImpulseResponse(**d["kwargs"])
        assert back.method == method and back.normalize_output is False and back.to_dict()["kwargs"]["method"] == method
    with pytest.raises(ValueError):
        A.HipReverbWithImpulseResponse(rir=rir, method="overlap-add")
    with pytest.raises(_lib.HipFeatError) as e:  # (still pinned: the random generator is not served)
        A.HipReverbWithImpulseResponse(rir=None, method="fft")
    assert e.value.status == _lib.ERR_UNSUPPORTED


def test_the_keyword_reaches_the_one_place_the_reverb_is_planned():
    for fn in (IS.FusedMiniBatch.features_of_tracks, IS.FusedAudioBatch.audio_of_tracks, IS._ArenaChain._tracks_chain, IS.FusedMiniBatch._mix_and_extract):
        assert inspect.signature(fn).parameters["reverb_method"].default == "direct", fn
    assert inspect.signature(IS._reverb_in_arena).parameters["method"].default == "direct"
    assert inspect.signature(A.reverb_in_arena).parameters["method"].default == "direct"
    assert inspect.signature(A.HipReverb.plan).parameters["method"].default == "direct" and inspect.signature(A.HipReverb.plan).parameters["min_fft_taps"].default is None
    src = inspect.getsource(IS)
    assert len(re.findall(r"_reverb_in_arena\(", src)) == 2  # its definition and ONE call, in _tracks_chain
    assert "reverb_method: str = \"direct\"" in src and src.count("self.reverb_method = _checked_reverb_method(reverb_method)") == 2  # the two strategies
    with pytest.raises(ValueError):
        IS._checked_reverb_method("overlap-add")
    assert isinstance(A.REVERB_AUTO_MIN_TAPS, int) and A.REVERB_AUTO_MIN_TAPS >= 1
