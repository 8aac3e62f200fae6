"""CPU: the statistics entry points (additive to ABI v8) are declared in the header with their own export macro, mirrored in
``_lib._STATS_SIGNATURES`` and exported by the built library (its symbol table; no device is touched)."""
import os
import re
import subprocess

import numpy as np

from lhotse_amd import _lib, build

from test_abi import HEADER, ROOT, declared_functions

STATS_API = {"hipfeat_stats_create", "hipfeat_stats_destroy", "hipfeat_stats_update", "hipfeat_stats_merge", "hipfeat_stats_get", "hipfeat_stats_reset"}
EARLIER = [_lib._SIGNATURES, _lib._LEVEL_SIGNATURES, _lib._COLLATE_SIGNATURES, _lib._SINC_SIGNATURES, _lib._FEATMIX_SIGNATURES]
OK, INVALID = 0, 1


def test_stats_entry_points_are_declared_mirrored_and_exported():
    declared = set(re.findall(r"HIPFEAT_STATS_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\(", open(HEADER).read()))
    assert declared == STATS_API == set(_lib._STATS_SIGNATURES)
    assert STATS_API <= set(_lib._ADDED_SIGNATURES)
    # ... and absent from the v8 set and from the sets added before, which older tests count
    assert set(declared_functions()) == set(_lib._SIGNATURES) and len(_lib._SIGNATURES) == 52
    for earlier in EARLIER:
        assert not STATS_API & set(earlier)
    assert all(callable(_lib.load().fn(name)) for name in STATS_API)  # the loaded library binds them
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hipfeat_\w+)", out))
    assert STATS_API <= exported
    assert set().union(*EARLIER) <= exported  # every earlier export


def test_the_abi_version_is_still_8_and_the_header_states_the_arithmetic():
    text = open(HEADER).read()
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", text).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version") == 8
    doc = text[text.index("v8 libraries built from this commit on also carry hipfeat_stats_*"): text.index("typedef struct hipfeat_stats hipfeat_stats;")]
    for cited in ("lhotse/features/base.py:957-1033", "lhotse/cut/set.py:2533-2583", "sum((x - mean_cut)^2)", "E[x^2] - E[x]^2 is never formed",
                  "r = total_frames / curr_frames", "(total_sum / r - curr_sum)^2", "Chan, Golub and LeVeque", "A cut of 0 frames contributes NOTHING"):
        assert cited in doc, cited


def test_prototypes_match_the_signature_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(STATS_API):
        proto = re.search(r"HIPFEAT_STATS_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert _lib._STATS_SIGNATURES[name] == ("int", args), (name, args)


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipfeat.h"\nint main(void) { hipfeat_stats* s = 0; hipfeat_stats** p = 0; int64_t n = 0; double d[2];\n'
                   "  (void)sizeof(hipfeat_stats_create(0, 80, p)); (void)sizeof(hipfeat_stats_destroy(s));\n"
                   "  (void)sizeof(hipfeat_stats_update(s, 0, 0, 0, 1, 0, &n, 80, 0)); (void)sizeof(hipfeat_stats_merge(s, 0, d, d, 0));\n"
                   "  (void)sizeof(hipfeat_stats_get(s, &n, d, d, 0)); (void)sizeof(hipfeat_stats_reset(s, 0));\n"
                   "  return HIPFEAT_ABI_VERSION == 8 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_null_handles_are_refused_without_a_device():
    lib = _lib.load()
    n, d = np.ones(1, dtype=np.int64), np.zeros(4, dtype=np.float64)
    assert lib.raw("hipfeat_stats_update", None, None, 0, 0, 1, None, _lib.addr(n), 4, None) == INVALID
    assert lib.raw("hipfeat_stats_merge", None, 1, _lib.addr(d), _lib.addr(d), None) == INVALID
    assert lib.raw("hipfeat_stats_get", None, _lib.addr(n), _lib.addr(d), _lib.addr(d), None) == INVALID and n[0] == 1
    assert lib.raw("hipfeat_stats_reset", None, None) == INVALID
    assert lib.raw("hipfeat_stats_create", 0, 4, None) == INVALID and lib.raw("hipfeat_stats_destroy", None) == OK
    out = np.zeros(1, dtype=np.uint64)
    assert lib.raw("hipfeat_stats_create", 0, 0, _lib.addr(out)) == INVALID and lib.raw("hipfeat_stats_create", 0, 65536, _lib.addr(out)) == INVALID and out[0] == 0
