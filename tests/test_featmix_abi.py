"""CPU: the feature-mix entry points (additive to ABI v8) are declared in the header with their own export macro, mirrored in
``_lib._FEATMIX_SIGNATURES`` and exported by the built library (its symbol table; no device is touched); the plan -- the cut and track
tables, every plan-time refusal with its status and the 16 ticket slots -- is what csrc/featmix_tables.hpp decides, checked here through
tests/native/featmix_tables_capi.cpp without a device."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from lhotse_amd import _lib, build
from lhotse_amd import augmentation as A
from lhotse_amd.augmentation import FEATMIX_COPY as COPY, FEATMIX_FOLD as FOLD, FeatCut, FeatTrack

from test_abi import HEADER, ROOT, declared_functions

FEATMIX_API = {"hipfeat_featmix_create", "hipfeat_featmix_destroy", "hipfeat_featmix_plan", "hipfeat_featmix_run"}
SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "featmix_tables_capi.cpp")
OK, INVALID, UNSUPPORTED = 0, 1, 3
POISON = -12345
CUT_DTYPE = np.dtype([("track_first", "<i4"), ("track_count", "<i4"), ("form", "<i4"), ("num_frames", "<i4"), ("dst_first", "<i4"), ("mix_frames", "<i4"),
                      ("ref_track", "<i4"), ("pad_value", "<f4")])
TRACK_DTYPE = np.dtype([("src_off", "<i8"), ("frames", "<i4"), ("rows", "<i4"), ("first", "<i4"), ("f16", "<i4"), ("part_first", "<i4"), ("part_count", "<i4"),
                        ("ratio", "<f8"), ("value", "<f4"), ("pad", "<i4")])


def test_featmix_entry_points_are_declared_mirrored_and_exported():
    declared = set(re.findall(r"HIPFEAT_FEATMIX_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\(", open(HEADER).read()))
    assert declared == FEATMIX_API == set(_lib._FEATMIX_SIGNATURES)
    # ... and absent from the v8 set and from the sets added before, which older tests count
    assert set(declared_functions()) == set(_lib._SIGNATURES)
    assert not FEATMIX_API & (set(_lib._SIGNATURES) | set(_lib._LEVEL_SIGNATURES) | set(_lib._COLLATE_SIGNATURES) | set(_lib._SINC_SIGNATURES))
    assert all(callable(_lib.load().fn(name)) for name in FEATMIX_API)  # the loaded library binds them
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hipfeat_\w+)", out))
    assert FEATMIX_API <= exported
    assert set(_lib._SIGNATURES) | set(_lib._LEVEL_SIGNATURES) | set(_lib._COLLATE_SIGNATURES) | set(_lib._SINC_SIGNATURES) <= exported  # every earlier export


def test_the_abi_version_is_still_8_and_the_header_states_the_arithmetic():
    text = open(HEADER).read()
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", text).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version") == 8
    doc = text[text.index("v8 libraries built from this commit on also carry hipfeat_featmix_*"): text.index("typedef struct hipfeat_featmix hipfeat_featmix;")]
    for cited in ("lhotse/dataset/collation.py:115-145", "mixed.py:1223-1243", "mixed.py:1245-1307", "lhotse/features/mixer.py",
                  "lhotse/features/kaldi/extractors.py:135-152", "lhotse/cut/mono.py:61-64", "mixed.py:1294-1300", "max(EPSILON, e + g_t * exp(x_t))"):
        assert cited in doc, cited


def test_prototypes_match_the_signature_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(FEATMIX_API):
        proto = re.search(r"HIPFEAT_FEATMIX_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert _lib._FEATMIX_SIGNATURES[name] == ("int", args), (name, args)


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipfeat.h"\nint main(void) { hipfeat_featmix* m = 0; int64_t i[4];\n'
                   "  (void)sizeof(hipfeat_featmix_plan(m, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, i)); (void)sizeof(hipfeat_featmix_run(m, 0, 0, 0, 0, 0, 0));\n"
                   "  return HIPFEAT_ABI_VERSION == 8 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_null_handles_are_refused_without_a_device():
    lib = _lib.load()
    info = np.zeros(4, dtype=np.int64)
    assert lib.raw("hipfeat_featmix_plan", None, 0, *([None] * 13), 1, 0, _lib.addr(info)) == INVALID
    assert lib.raw("hipfeat_featmix_run", None, 0, None, 0, None, 0, None) == INVALID
    assert lib.raw("hipfeat_featmix_create", 0, None) == INVALID and lib.raw("hipfeat_featmix_destroy", None) == OK


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(tempfile.mkdtemp(prefix="fmtab_"), "libfmtab.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", out])
    lib = ctypes.CDLL(out)
    lib.ft_plan.restype = ctypes.c_int
    lib.ft_plan.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 13 + [ctypes.c_longlong, ctypes.c_longlong] + [ctypes.c_void_p] * 4
    lib.ft_slots_plan.restype = ctypes.c_longlong
    lib.ft_slots_run.argtypes = [ctypes.c_longlong]
    lib.ft_tiles.restype = ctypes.c_longlong
    lib.ft_tiles.argtypes = [ctypes.c_longlong]
    return lib


def raw_plan(shim, lay, F=None, row_frames=None, cuts=None):
    """The shim over the arrays of a layout -> (status, info, cut table, track table, message); ``info`` is pre-filled with POISON so that
    "plans nothing" can be seen."""
    n = len(lay["h_form"]) if cuts is None else cuts
    info, msg = np.full(4, POISON, np.int64), ctypes.create_string_buffer(256)
    ct, tt = np.zeros(max(n, 0), CUT_DTYPE), np.zeros(len(lay["h_src_offset"]), TRACK_DTYPE)
    st = shim.ft_plan(n, *(None if lay[k] is None else lay[k].ctypes.data for k in A._FEATMIX_ARGS), lay["num_features"] if F is None else F,
                      lay["row_frames"] if row_frames is None else row_frames, info.ctypes.data, ct.ctypes.data, tt.ctypes.data, ctypes.addressof(msg))
    return st, info, ct, tt, msg.value.decode()


def arrays(cuts, F, row_frames=None):
    """The tables of ``cuts`` WITHOUT the checks of featmix_layout (so that the shim sees what the layout would have refused)."""
    cuts = [FeatCut(*c) for c in cuts]
    tr = [FeatTrack(*t) for c in cuts for t in c.tracks]
    first = np.cumsum([0] + [len(c.tracks) for c in cuts])
    if row_frames is None:
        row_frames = max(c.dst_first + c.num_frames for c in cuts)
    return {"h_track_first": _lib.i64(first), "h_form": np.array([c.form for c in cuts], np.int32), "h_num_frames": _lib.i64([c.num_frames for c in cuts]),
            "h_pad_value": np.array([c.pad_value for c in cuts], np.float64), "h_dst_first": _lib.i64([c.dst_first for c in cuts]),
            "h_ref_track": np.array([c.ref_track for c in cuts], np.int32), "h_src_offset": _lib.i64([t.offset for t in tr]),
            "h_src_rows": _lib.i64([t.frames if t.rows is None else t.rows for t in tr]), "h_frames": _lib.i64([t.frames for t in tr]),
            "h_dtype": np.array([int(t.f16) for t in tr], np.int32), "h_first": _lib.i64([t.first for t in tr]),
            "h_snr_db": np.array([np.nan if t.snr is None else t.snr for t in tr], np.float64), "h_value": np.array([t.value for t in tr], np.float64),
            "num_features": F, "row_frames": row_frames}


GOOD = [FeatCut([FeatTrack(6, 70, 69, True)], 77, COPY, -23.0, 1),
        FeatCut([FeatTrack(-1, 9, value=-23.0), FeatTrack(1 << 33, 500, 501, False, 9, 10.0), FeatTrack(12, 0, 0, False, 5, 5.0), FeatTrack(4000, 30, None, True, 480)],
                510, FOLD, 0.0, 2, 1)]


def test_the_tables_are_what_the_kernels_read(shim):
    assert CUT_DTYPE.itemsize == 32 and TRACK_DTYPE.itemsize == 48
    assert shim.ft_tile() == A.FEATMIX_TILE == 4096 and shim.ft_energy_block() == A.FEATMIX_ENERGY_BLOCK == 16384
    assert shim.ft_max_tracks() == A.FEATMIX_MAX_TRACKS == 256 and shim.ft_slots() == 16
    F = 80
    lay = A.featmix_layout(1 << 40, GOOD, F)
    assert lay["row_frames"] == 512
    st, info, ct, tt, msg = raw_plan(shim, lay)
    assert st == OK, msg
    tiles = (512 * F - 1 + 3) // 4096 + 1
    assert shim.ft_tiles(512 * F) == tiles == 11 and shim.ft_tiles(0) == 0 and shim.ft_tiles(4093) == 1 and shim.ft_tiles(4094) == 2
    parts = (500 * F + 16383) // 16384  # the one stored track with an SNR, which is the reference too
    # {ticket, bytes the arena must hold (the stored row too many is not read), energy work items, fold work items}
    assert info.tolist() == [0, (1 << 33) + 500 * F * 4, parts, 2 * tiles] and lay["arena_need"] == info[1]
    assert ct["track_first"].tolist() == [0, 1] and ct["track_count"].tolist() == [1, 4] and ct["form"].tolist() == [COPY, FOLD]
    assert ct["num_frames"].tolist() == [77, 510] and ct["dst_first"].tolist() == [1, 2] and ct["mix_frames"].tolist() == [70, 510]
    assert ct["ref_track"].tolist() == [-1, 2] and ct["pad_value"].tolist() == [-23.0, 0.0]
    assert tt["src_off"].tolist() == [6, -1, 1 << 33, 12, 4000] and tt["frames"].tolist() == [70, 9, 500, 0, 30] and tt["rows"].tolist() == [69, 9, 501, 0, 30]
    assert tt["first"].tolist() == [0, 0, 9, 5, 480] and tt["f16"].tolist() == [1, 0, 0, 0, 1] and tt["value"].tolist() == [0.0, -23.0, 0.0, 0.0, 0.0]
    assert tt["part_first"].tolist() == [0, 0, 0, parts, parts] and tt["part_count"].tolist() == [0, 0, parts, 0, 0]
    assert tt["ratio"][2] == pytest.approx(0.1) and tt["ratio"][3] == pytest.approx(10 ** -0.5) and (tt["ratio"][[0, 1, 4]] == -1.0).all()
    # NULL tables take their defaults: float32, frame 0, no SNR, no reference, rows == frames
    lay2 = arrays([FeatCut([FeatTrack(0, 5), FeatTrack(400, 5)], 5, FOLD)], 3)
    for k in ("h_pad_value", "h_dst_first", "h_ref_track", "h_src_rows", "h_dtype", "h_first", "h_snr_db", "h_value"):
        lay2[k] = None
    st, info, ct, tt, msg = raw_plan(shim, lay2)
    assert st == OK and info.tolist() == [0, 400 + 5 * 3 * 4, 0, 1] and tt["rows"].tolist() == [5, 5] and ct["ref_track"].tolist() == [-1], msg


def test_plan_time_errors_are_decided_on_the_host_and_by_the_layout(shim):
    def refused(cuts, F=4, row_frames=None, status=INVALID, word=""):
        st, info, _, _, msg = raw_plan(shim, arrays(cuts, F, row_frames))
        assert (st == status and msg and word in msg and info.tolist() == [POISON] * 4) or st == OK, (st, msg)  # a refusal plans nothing
        if st != OK:  # ... and the pure-host layout refuses the same table before anything is planned
            with pytest.raises(ValueError):
                A.featmix_layout(1 << 62, cuts, F, row_frames)
        else:
            A.featmix_layout(1 << 62, cuts, F, row_frames)
        return st != OK

    T = FeatTrack
    assert not refused([FeatCut([T(0, 8)], 8)])
    assert refused([FeatCut([T(-2, 8)], 8)], word="negative") and refused([FeatCut([T(0, 8, first=-1)], 8, FOLD)], word="negative")
    assert refused([FeatCut([T(2, 8)], 8)], word="aligned") and refused([FeatCut([T(1, 8, f16=True)], 8)], word="aligned")
    assert not refused([FeatCut([T(2, 8, f16=True)], 8)]) and not refused([FeatCut([T(4, 8)], 8)])
    assert refused([FeatCut([T(0, 8)], 8)], row_frames=7, word="do not fit") and refused([FeatCut([T(0, 8)], 8, dst_first=1)], row_frames=8, word="do not fit")
    assert refused([FeatCut([T(0, 8)], -1)], row_frames=8) and refused([FeatCut([T(0, 8)], 8, dst_first=-1)], row_frames=8)
    assert refused([FeatCut([T(0, -1)], 8)]) and refused([FeatCut([T(0, 8)], 8)], F=0) and refused([FeatCut([T(0, 8)], 8)], F=2 ** 30)
    assert refused([FeatCut([T(0, 8)], 8)], F=4, row_frames=2 ** 28)  # a row beyond 2^30 elements
    assert refused([FeatCut([T(0, 8, rows=10)], 8)], word="stored rows") and refused([FeatCut([T(0, 8, rows=6)], 8)], word="stored rows")
    assert refused([FeatCut([T(0, 1, rows=0)], 1)], word="stored rows") and not refused([FeatCut([T(0, 8, rows=9)], 8), FeatCut([T(0, 8, rows=7)], 8)])
    assert refused([FeatCut([T(0, 9)], 8)], word="does not fit") and not refused([FeatCut([T(0, 7)], 8)])  # copy: the track is longer than the cut
    assert refused([FeatCut([T(0, 8), T(0, 8)], 8)], word="one track") and refused([FeatCut([T(0, 8, first=1)], 9)], word="frame 0")
    assert refused([FeatCut([T(0, 8), T(0, 8, first=4)], 10, FOLD)], word="mix to 12") and refused([FeatCut([T(0, 8)], 10, FOLD)], word="mix to 8")
    assert not refused([FeatCut([T(0, 8), T(0, 8, first=4)], 11, FOLD)]) and not refused([FeatCut([T(0, 8), T(0, 8, first=4)], 13, FOLD)])
    assert refused([FeatCut([T(0, 0)], 1, FOLD)], word="mix to 0")  # nothing to repeat
    assert refused([FeatCut([T(0, 8)], 8, FOLD, ref_track=1)], word="reference") and refused([FeatCut([T(0, 8)], 8, FOLD, ref_track=-2)], word="reference")
    assert refused([FeatCut([T(0, 8)], 8, form=2)], word="form") and refused([FeatCut([], 8)], word="at least one track")
    assert refused([FeatCut([T(0, 8), T(0, 8, snr=-1e9)], 8, FOLD, ref_track=0)], word="SNR") and not refused([FeatCut([T(0, 8), T(0, 8, snr=-3000.0)], 8, FOLD)])
    many = [T(0, 3)] * 257
    assert refused([FeatCut(many, 3, FOLD)], status=UNSUPPORTED, word="up to 256 per cut") and not refused([FeatCut(many[:256], 3, FOLD)])
    st, _, _, _, msg = raw_plan(shim, arrays([FeatCut([T(0, 8)], 8)], 4), cuts=0)
    assert st == INVALID and "1 ... 65535" in msg
    lay = arrays([FeatCut([T(0, 8)], 8)], 4)
    lay["h_track_first"] = _lib.i64([1, 2])
    assert raw_plan(shim, lay)[0] == INVALID
    lay = arrays([FeatCut([T(0, 8)], 8)], 4)
    lay["h_dtype"] = np.array([2], np.int32)
    assert raw_plan(shim, lay)[0] == INVALID
    with pytest.raises(ValueError, match="arena too small"):
        A.featmix_layout(127, [FeatCut([T(0, 8)], 8)], 4)
    assert A.featmix_layout(128, [FeatCut([T(0, 8)], 8)], 4)["arena_need"] == 128


def test_a_17th_plan_while_16_are_outstanding_is_refused(shim):
    shim.ft_slots_reset()
    assert [shim.ft_slots_plan() for _ in range(16)] == list(range(16))
    assert shim.ft_slots_plan() == -1 and shim.ft_slots_plan() == -1  # refused, and nothing planned: the 16 stay what they were
    assert shim.ft_slots_run(16) == INVALID and shim.ft_slots_run(-1) == INVALID  # unknown tickets
    assert shim.ft_slots_run(5) == OK and shim.ft_slots_plan() == -1  # the slot ticket 16 would take (0) is still planned
    assert shim.ft_slots_run(0) == OK and shim.ft_slots_run(0) == INVALID  # a ticket runs once
    assert shim.ft_slots_plan() == 16 and shim.ft_slots_run(16) == OK


def test_offsets_past_2_31_travel_unchanged(shim):
    far = 2 ** 40 + 2
    st, info, ct, tt, msg = raw_plan(shim, arrays([FeatCut([FeatTrack(far, 77, f16=True)], 77), FeatCut([FeatTrack(2 ** 31 + 4, 3)], 3)], 80))
    assert st == OK and tt["src_off"].tolist() == [far, 2 ** 31 + 4] and info.tolist()[1] == far + 77 * 80 * 2, msg


def test_stand_alone_program_of_the_shim(tmp_path):
    exe = str(tmp_path / "fmtab")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DFEATMIX_TABLES_MAIN", SHIM, "-o", exe])
    # (bounds and overflow are what is looked for; the leak check at exit needs ptrace, which not every container grants)
    res = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
