"""CPU: the sinc entry points (additive to ABI v8) are declared in the header with their own export macro, mirrored in
``_lib._SINC_SIGNATURES`` and exported by the built library (its symbol table; no device is touched), the header still compiles as C99, every
earlier export is still there; the plan -- lengths, the row table and every plan-time refusal with its status -- is what
csrc/sinc_tables.hpp decides, checked here through tests/native/sinc_tables_capi.cpp without a device."""
import os
import re
import subprocess

import numpy as np
import pytest

from lhotse_amd import _lib, build

from test_abi import HEADER, ROOT, declared_functions
from test_sinc_tables import plan, shim  # noqa: F401  (the shim fixture)

SINC_API = {"hipfeat_sinc_create", "hipfeat_sinc_destroy", "hipfeat_sinc_plan", "hipfeat_sinc_run", "hipfeat_sinc_weights"}
OK, INVALID, UNSUPPORTED = 0, 1, 3
POISON = -7


def test_sinc_entry_points_are_declared_mirrored_and_exported():
    declared = set(re.findall(r"HIPFEAT_SINC_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\(", open(HEADER).read()))
    assert declared == SINC_API == set(_lib._SINC_SIGNATURES)
    # ... and absent from the v8 set and from the sets added before, which older tests count
    assert set(declared_functions()) == set(_lib._SIGNATURES) and len(_lib._SIGNATURES) == 52
    assert not SINC_API & (set(_lib._SIGNATURES) | set(_lib._LEVEL_SIGNATURES) | set(_lib._COLLATE_SIGNATURES))
    assert all(callable(_lib.load().fn(name)) for name in SINC_API)  # the loaded library binds them
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hipfeat_\w+)", out))
    assert SINC_API <= exported
    assert set(_lib._SIGNATURES) | set(_lib._LEVEL_SIGNATURES) | set(_lib._COLLATE_SIGNATURES) <= exported  # every earlier export


def test_the_abi_version_is_still_8_and_the_header_cites_what_it_replaces():
    text = open(HEADER).read()
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", text).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version") == 8
    doc = text[text.index("v8 libraries built from this commit on also carry hipfeat_sinc_*"): text.index("typedef struct hipfeat_sinc hipfeat_sinc;")]
    for cited in ("lhotse/augmentation/resample.py:184-315", "resample.py:239-281", "resample.py:309", "lhotse/dataset/cut_transforms/lowpass.py",
                  "lhotse/augmentation/torchaudio.py:86-139"):
        assert cited in doc, cited


def test_prototypes_match_the_signature_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(SINC_API):
        proto = re.search(r"HIPFEAT_SINC_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert _lib._SINC_SIGNATURES[name] == ("int", args), (name, args)


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipfeat.h"\nint main(void) { hipfeat_sinc* s = 0; int32_t d[3]; int64_t i[4];\n'
                   "  (void)sizeof(hipfeat_sinc_plan(s, 0, 0, 0, 0, 0, 0, 0, 0, i)); (void)sizeof(hipfeat_sinc_weights(s, 1, 2, 0, 0, d, 0));\n"
                   "  (void)sizeof(hipfeat_sinc_run(s, 0, 0, 0, 0)); return HIPFEAT_ABI_VERSION == 8 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_null_handles_are_refused_without_a_device():
    lib = _lib.load()
    info = np.zeros(4, dtype=np.int64)
    assert lib.raw("hipfeat_sinc_plan", None, 0, None, None, None, None, None, 0, None, _lib.addr(info)) == INVALID
    assert lib.raw("hipfeat_sinc_run", None, 0, None, 0, None) == INVALID
    assert lib.raw("hipfeat_sinc_weights", None, 16000, 9346, None, None, None, None) == INVALID
    assert lib.raw("hipfeat_sinc_create", 0, None) == INVALID and lib.raw("hipfeat_sinc_destroy", None) == OK


def test_plan_time_refusals_have_their_own_status_and_message(shim):  # noqa: F811
    def refused(status, needle, *a):
        st, out_len, info, rows, msg = plan(shim, *a)
        assert st == status and needle in msg, (st, msg)
        assert out_len.tolist() == [POISON] * len(out_len) and info.tolist() == [POISON] * 4  # a refusal plans nothing
        return True

    A = 1 << 20
    st, out_len, info, rows, msg = plan(shim, [0], [16000], [16000], [9346], [16000], A)
    assert st == OK and out_len.tolist() == [9346] and info.tolist() == [0, 16000 + 9346, 19, 24], msg
    assert refused(INVALID, "overlaps the input of row 0", [0], [16000], [16000], [9346], [15999], A)  # its own input
    assert refused(INVALID, "overlaps the input of row 1", [0, 40000], [16000, 16000], [16000, 16000], [9346, 9346], [50000, 70000], A)  # another row's
    assert refused(INVALID, "their outputs overlap", [0, 16000], [16000, 16000], [16000, 16000], [9346, 9346], [40000, 49345], A)
    assert plan(shim, [0, 16000], [16000, 16000], [16000, 16000], [9346, 9346], [40000, 49346], A)[0] == OK  # back to back is fine
    assert refused(INVALID, "output 16000 + 9346 lies past the arena", [0], [16000], [16000], [9346], [16000], 16000 + 9345)
    assert refused(INVALID, "input 0 + 16000 lies past the arena", [0], [16000], [16000], [9346], [0], 15999)
    assert refused(INVALID, "equal rates", [0], [16000], [16000], [16000], [16000], A)
    assert refused(INVALID, "both must be positive", [0], [16000], [0], [16000], [16000], A)
    assert refused(INVALID, "both must be positive", [0], [16000], [16000], [-8000], [16000], A)
    assert refused(UNSUPPORTED, "window of 100 taps", [0], [16000], [48000], [6000], [16000], A)
    assert refused(INVALID, "negative offset", [-1], [16000], [16000], [9346], [16000], A)
    assert refused(INVALID, "negative offset", [0], [16000], [16000], [9346], [-4], A)
    assert refused(INVALID, "samples, must be", [0], [-1], [16000], [9346], [16000], A)
    assert refused(INVALID, "samples, must be", [0], [2 ** 30], [16000], [9346], [2 ** 30], 2 ** 40)
    assert refused(INVALID, "samples come out", [0], [2 ** 29], [8000], [48000], [2 ** 30], 2 ** 40)
    # a refused row anywhere refuses the whole plan
    assert refused(UNSUPPORTED, "row 1", [0, 16000], [16000, 16000], [16000, 48000], [9346, 6000], [40000, 60000], A)


def test_valid_edge_plans_and_offsets_past_2_31(shim):  # noqa: F811
    st, out_len, info, rows, msg = plan(shim, [], [], [], [], [], 0)  # no rows: a plan whose run launches nothing
    assert st == OK and info.tolist() == [0, 0, 0, 0], msg
    st, out_len, info, rows, msg = plan(shim, [5, 5], [0, 0], [16000, 9346], [9346, 16000], [5, 5], 8)  # rows of no samples read and write nothing
    assert st == OK and out_len.tolist() == [0, 0] and info.tolist() == [0, 0, 0, 0] and len(rows) == 0, msg
    far = 2 ** 31 + 8
    st, out_len, info, rows, msg = plan(shim, [far, 0], [16000, 16000], [16000, 16000], [9346, 9346], [16000, 2 ** 33], 2 ** 34)
    assert st == OK and rows["in_off"].tolist() == [far, 0] and rows["out_off"].tolist() == [16000, 2 ** 33] and info[1] == 2 ** 33 + 9346, msg
