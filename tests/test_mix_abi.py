"""CPU: the mixer entry points (ABI v6 on) are declared in the header, mirrored in ``_lib._SIGNATURES`` and exported by the built library
(its symbol table; no device is touched), and the host-only parts of the Python layer agree with the rule of tests/_mix_ref.py; the plan
-- the tables and every plan-time error -- is what csrc/mix_tables.hpp decides, checked here through tests/native/mix_tables_capi.cpp
without a device; the launch constants the large GPU shapes of the augmentation chain sit on are what the sources say."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from lhotse_amd import _lib, build
from lhotse_amd.augmentation import _mix_tables, mixed_num_samples, mixed_tail_floats

from test_abi import HEADER, declared_functions

MIX_API = {"hipfeat_mixer_create", "hipfeat_mixer_destroy", "hipfeat_mix_plan", "hipfeat_mix_run"}
SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "mix_tables_capi.cpp")
OK, INVALID, UNSUPPORTED = 0, 1, 3
CUT_DTYPE = np.dtype([("out_off", "<i8"), ("out_len", "<i4"), ("item_first", "<i4"), ("track_first", "<i4"), ("track_count", "<i4"), ("ref_track", "<i4"),
                      ("pad", "<i4")])
TRACK_DTYPE = np.dtype([("src_off", "<i8"), ("src_len", "<i4"), ("dst_off", "<i4"), ("part_first", "<i4"), ("part_count", "<i4"), ("ratio", "<f8")])
POISON = -0x5A5A5A5A


def test_mixer_entry_points_are_declared_mirrored_and_exported():
    names = set(declared_functions())
    assert MIX_API <= names and MIX_API <= set(_lib._SIGNATURES)
    assert names == set(_lib._SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    assert MIX_API <= set(re.findall(r" T (hipfeat_\w+)", out))


def test_abi_version_agrees_everywhere_and_knows_the_mixer():
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version")
    assert header >= 6  # the mixer entry points arrived with version 6


def test_prototypes_match_the_signature_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(MIX_API):
        proto = re.search(r"HIPFEAT_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert args == _lib._SIGNATURES[name][1], (name, args)


def test_mixed_sizes_follow_the_rule():
    first, lens, offs = [0, 2, 3, 6], [1000, 500, 7, 2000, 100, 3000], [0, 900, 0, 0, 2950, 0]
    assert mixed_num_samples(first, lens, offs).tolist() == [1400, 7, 3050]
    assert mixed_num_samples(first, lens, offs, [1399, -1, 4000]).tolist() == [1399, 7, 3050]
    assert mixed_tail_floats(first, lens, offs, [1399, -1, 4000]) == 1400 + 8 + 3052 + 3
    assert isinstance(mixed_tail_floats(first, lens, offs), int) and np.all(mixed_num_samples(first, lens, offs) > 0)


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(tempfile.mkdtemp(prefix="mixtab_"), "libmixtab.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", out])
    lib = ctypes.CDLL(out)
    lib.mt_plan.restype = ctypes.c_int
    lib.mt_plan.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 7 + [ctypes.c_longlong] + [ctypes.c_void_p] * 6
    return lib


def plan(shim, track_first, src_offsets, src_lens, dst_offsets, snrs=None, ref_tracks=None, max_samples=None, tail_start=0):
    """The arguments of ``HipMixer.plan`` -> (status, info, out_offsets, out_lens, cuts, tracks, message); the outputs start as POISON."""
    first, so, sl, do, snr, ref, cap = _mix_tables(track_first, src_offsets, src_lens, dst_offsets, snrs, ref_tracks, max_samples)
    n = len(first) - 1
    info, offs, lens = np.full(4, POISON, np.int64), np.full(n, POISON, np.int64), np.full(n, POISON, np.int64)
    cuts, tracks, msg = np.zeros(n, CUT_DTYPE), np.zeros(max(int(first[-1]), 0), TRACK_DTYPE), ctypes.create_string_buffer(256)
    st = shim.mt_plan(n, *(a.ctypes.data for a in (first, so, sl, do, snr, ref, cap)), int(tail_start), offs.ctypes.data, lens.ctypes.data, info.ctypes.data,
                      cuts.ctypes.data, tracks.ctypes.data, ctypes.addressof(msg))
    return st, info, offs, lens, cuts, tracks, msg.value.decode()


def test_the_tables_are_what_the_kernels_read(shim):
    assert CUT_DTYPE.itemsize == TRACK_DTYPE.itemsize == 32
    assert (shim.mt_block(), shim.mt_energy_block(), shim.mt_max_tracks()) == (4096, 16384, 256)
    # cut 0: speech (the reference) + noise at 10 dB from sample 10 + a padding track; cut 1: one track, capped at 4099 of its 4100 samples;
    # cut 2: noise in FRONT of its reference (track 1), which then needs its energy too
    first, so = [0, 3, 4, 6], [0, 20000, -1, 40000, 50000, 60000]
    sl, do = [20000, 16385, 30000, 4100, 500, 600], [0, 10, 0, 0, 0, 100]
    st, info, offs, lens, cuts, tracks, msg = plan(shim, first, so, sl, do, [None, 10.0, None, None, -3.0, None], [0, -1, 1], [-1, 4099, -1], 70001)
    assert st == OK, msg
    assert lens.tolist() == [30000, 4099, 700] == cuts["out_len"].tolist()
    assert offs.tolist() == [70004, 70004 + 30000, 70004 + 30000 + 4100] == cuts["out_off"].tolist()  # (each on a 16-byte boundary behind tail_start)
    assert cuts["item_first"].tolist() == [0, 8, 10] and cuts["track_first"].tolist() == [0, 3, 4] and cuts["track_count"].tolist() == [3, 1, 2]
    assert cuts["ref_track"].tolist() == [0, -1, 5] and cuts["pad"].tolist() == [0, 0, 0]  # (an index into the track table)
    assert tracks["src_off"].tolist() == so and tracks["src_len"].tolist() == sl and tracks["dst_off"].tolist() == do
    # partials: 16384 samples each, for a scaled track and for the reference of a cut that has one
    assert tracks["part_count"].tolist() == [2, 2, 0, 0, 1, 1] and tracks["part_first"].tolist() == [0, 2, 4, 4, 4, 5]
    assert tracks["ratio"].tolist() == [-1.0, 10.0 ** -1.0, -1.0, -1.0, 10.0 ** 0.3, -1.0]
    assert info.tolist() == [0, 70004 + 30000 + 4100 + 700, 6, 8 + 2 + 1]
    # the first track being the reference itself carries no gain (mixed.py:1346-1350), whatever its SNR says
    st, info, _, _, _, tracks, msg = plan(shim, [0, 2], [0, 100], [100, 100], [0, 0], [5.0, None], [0], None, 200)
    assert st == OK and tracks["part_count"].tolist() == [0, 0] and tracks["ratio"].tolist() == [-1.0, -1.0] and info.tolist() == [0, 300, 0, 1], msg


def test_plan_time_errors_are_decided_on_the_host(shim):
    """The refusals of tests/test_gpu_mix.py::test_bad_tables_are_refused_and_launch_nothing, with its tables; a refusal writes no output."""
    good = dict(track_first=[0, 2], src_offsets=[0, 1000], src_lens=[1000, 500], dst_offsets=[0, 10], snrs=[None, 10.0], ref_tracks=[0], max_samples=None,
                tail_start=1500)

    def status(**kw):
        st, info, offs, lens, _, _, msg = plan(shim, **{**good, **kw})
        if st != OK:
            assert msg and (info == POISON).all() and (offs == POISON).all() and (lens == POISON).all()
        return st

    assert status() == OK
    assert status(src_offsets=[0, 1200]) == INVALID  # a source reaches into the tail, where the mixed cuts are written
    assert status(ref_tracks=[2]) == INVALID and status(ref_tracks=[-2]) == INVALID  # reference index outside the cut
    assert status(src_offsets=[-1, 1000]) == INVALID  # the reference track is a padding track
    assert status(dst_offsets=[0, -1]) == INVALID and status(src_offsets=[0, -5]) == INVALID  # negative offsets
    assert status(track_first=[0, 0], src_offsets=[], src_lens=[], dst_offsets=[], snrs=[], ref_tracks=[-1]) == INVALID  # a cut without tracks
    assert status(src_lens=[1000, 0]) == INVALID
    n = 257
    assert status(track_first=[0, n], src_offsets=[0] * n, src_lens=[10] * n, dst_offsets=[0] * n, snrs=[None] * n, ref_tracks=[-1]) == UNSUPPORTED
    assert status(track_first=[0, n - 1], src_offsets=[0] * 256, src_lens=[10] * 256, dst_offsets=[0] * 256, snrs=[None] * 256, ref_tracks=[-1]) == OK
    # ... and the ones no GPU test reaches
    assert status(tail_start=-1) == INVALID and status(track_first=[1, 2]) == INVALID
    assert status(snrs=[None, 4000.0]) == OK and status(snrs=[None, -4000.0]) == INVALID  # 10^(-snr/10): 0 is a ratio, inf is not
    assert status(max_samples=[0]) == INVALID  # the mix is empty
    assert status(src_lens=[1000, 2 ** 30]) == INVALID
    assert "reaches into the arena's tail" in plan(shim, **{**good, "src_offsets": [0, 1200]})[6]
    assert "serves up to 256 per cut" in plan(shim, [0, n], [0] * n, [10] * n, [0] * n, None, [-1], None, 1500)[6]


def test_stand_alone_program_of_the_shim(tmp_path):
    exe = str(tmp_path / "mixtab")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DMIX_TABLES_MAIN", SHIM, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr


def test_launch_constants_the_gpu_shapes_sit_on():
    """tests/test_gpu_reverb.py, test_gpu_mix.py and test_gpu_minibatch.py choose batch sizes ON the limits at which a launch changes its
    path: 3328 bytes of tables (kernel arguments | staged), 24576 (searched in LDS | in HBM), 1792 workgroups (one work item each | a
    second trip of the loop), with 48-byte reverb items and 32-byte mix descriptors.  If a source moves one of them, this fails, so the
    GPU shapes cannot silently stop sitting on the boundaries."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "csrc")
    names = ("kernel_minibatch.hpp", "kernel_reverb.hpp", "kernel_mix.hpp", "reverb_tables.hpp", "mix_tables.hpp", "hipfeat.hip")
    text = {name: open(os.path.join(csrc, name)).read() for name in names}

    def constant(name, source):
        return int(re.search(r"constexpr int %s = (\d+)\s*;" % name, text[source]).group(1))

    inline_bytes, lds_bytes = constant("kMbInlineBytes", "kernel_minibatch.hpp"), constant("kMbLdsTableBytes", "kernel_minibatch.hpp")
    assert (inline_bytes, lds_bytes) == (3328, 24576)
    # the descriptors and block sizes live in the pure host headers, which the kernel headers include
    assert "static_assert(sizeof(RvItem) == 48," in text["reverb_tables.hpp"] and '#include "reverb_tables.hpp"' in text["kernel_reverb.hpp"]
    assert "static_assert(sizeof(MixTrack) == 32 && sizeof(MixCut) == 32," in text["mix_tables.hpp"] and '#include "mix_tables.hpp"' in text["kernel_mix.hpp"]
    assert re.search(r"constexpr int kRvBlock = 256 \* kRvLane;", text["reverb_tables.hpp"]) and constant("kRvLane", "reverb_tables.hpp") == 8
    assert (constant("kMixBlock", "mix_tables.hpp"), constant("kMixEnergyBlock", "mix_tables.hpp")) == (4096, 16384)
    for moved in ("struct RvItem", "kRvLane =", "kRvBlock ="):
        assert moved not in text["kernel_reverb.hpp"]
    for moved in ("struct MixTrack", "struct MixCut", "kMixBlock =", "kMixEnergyBlock ="):
        assert moved not in text["kernel_mix.hpp"]
    # the workgroup limit of the launch functions: grid = ceil(items / ceil(items / 1792)), stated once, in the helper all of them call
    hip = text["hipfeat.hip"]
    helper = re.search(r"static unsigned items_grid\(int64_t items, int64_t slots = 1792\) \{\n(.*?)\n\}", hip, flags=re.S).group(1)
    assert "per_wg = std::max<int64_t>(1, (items + slots - 1) / slots);" in helper and "(items + per_wg - 1) / per_wg" in helper
    assert hip.count("1792") == 2 and "1791" not in hip  # (the helper's default, and the experiment switch of the mini-batch run below)
    runs = ("hipfeat_minibatch_run", "hipfeat_mix_run", "hipfeat_reverb_run", "hipfeat_level_run")
    body = {fn: hip[hip.index('hipfeat_status %s(' % fn) :] for fn in runs}
    body = {fn: b[: b.index("\n}\n")] for fn, b in body.items()}
    assert re.search(r"atoi\(exp_env\(\"HIPFEAT_MB_SLOTS\"\)\)\) : 1792;", body["hipfeat_minibatch_run"])
    assert "items_grid(items, mb_slots)" in body["hipfeat_minibatch_run"]
    assert body["hipfeat_mix_run"].count("items_grid(p.energy_items)") == 1 and body["hipfeat_mix_run"].count("items_grid(p.mix_items)") == 1
    assert "items_grid(p.work_items)" in body["hipfeat_reverb_run"] and "items_grid(p.work_items)" in body["hipfeat_level_run"]
    # every route decision compares with the two table limits: one function decides, and all four launch functions ask it and nobody else
    route = re.search(r"static TableRoute table_route\(bool allow_inline, size_t bytes\) \{\n(.*?)\n\}", hip, flags=re.S).group(1)
    assert "bytes <= (size_t)kMbInlineBytes" in route and "bytes <= (size_t)kMbLdsTableBytes ? bytes : 0" in route
    assert hip.count("kMbInlineBytes") == 1 and hip.count("kMbLdsTableBytes") == 1
    for fn, b in body.items():
        assert b.count("table_route(") == 1 and ".dyn, st, h)" in b, fn
    # ... and the GPU test files state the same numbers
    import test_gpu_minibatch
    import test_gpu_mix
    import test_gpu_reverb

    assert (test_gpu_reverb.INLINE_BYTES, test_gpu_reverb.LDS_TABLE_BYTES, test_gpu_reverb.MAX_WORKGROUPS) == (inline_bytes, lds_bytes, 1792)
    assert (test_gpu_reverb.RV_ITEM_BYTES, test_gpu_reverb.RV_BLOCK) == (48, 2048)
    assert (test_gpu_mix.INLINE_BYTES, test_gpu_mix.LDS_TABLE_BYTES, test_gpu_mix.MAX_WORKGROUPS) == (inline_bytes, lds_bytes, 1792)
    assert (test_gpu_mix.DESCRIPTOR_BYTES, test_gpu_mix.MIX_BLOCK, test_gpu_mix.ENERGY_BLOCK) == (32, 4096, 16384)
    assert test_gpu_minibatch.LDS_TABLE_BYTES == lds_bytes
    # the boundary batches: 69 | 70 and 512 | 513 reverb items, 104 | 105 and 768 | 769 mix descriptors
    assert (inline_bytes // 48, lds_bytes // 48, inline_bytes // 32, lds_bytes // 32) == (69, 512, 104, 768)
