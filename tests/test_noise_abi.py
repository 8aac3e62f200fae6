"""CPU: ``hipfeat_noise_run`` (additive to ABI v8) is declared under its own export macro, mirrored in ``_lib._NOISE_SIGNATURES``,
exported by the built library, and refuses bad arguments before it touches a device; and the statement the GPU tests hold the kernel
to (tests/_noise_ref.py) is the published Philox4x32-10 and gives standard normals."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _noise_ref as R
from lhotse_amd import _lib, build

from test_abi import HEADER, ROOT

INVALID = 1
NAME = "hipfeat_noise_run"


def test_the_entry_point_is_declared_mirrored_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+HIPFEAT_NOISE_API\s+HIPFEAT_API\b", text)
    protos = re.findall(r"HIPFEAT_NOISE_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\((.*?)\)\s*;", text, flags=re.S)
    assert [name for name, _ in protos] == [NAME] == list(_lib._NOISE_SIGNATURES)
    args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in protos[0][1].split(",")]
    assert _lib._NOISE_SIGNATURES[NAME] == ("int", args) == _lib._ADDED_SIGNATURES[NAME]
    assert NAME not in _lib._SIGNATURES and len(_lib._SIGNATURES) == 52
    assert _lib.load().raw("hipfeat_abi_version") == _lib.ABI_VERSION == 8
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    assert NAME in re.findall(r" T (hipfeat_\w+)", out)


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipfeat.h"\nint main(void) { float x[4], s[1]; int64_t k[1];\n'
                   "  (void)sizeof(hipfeat_noise_run(x, x, 1, 4, 4, 4, HIPFEAT_NOISE_FLOAT32, s, k, k, 1, -1.0f, 1.0f, 0));\n"
                   "  return HIPFEAT_ABI_VERSION == 8 && HIPFEAT_NOISE_BFLOAT16 == 2 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


# every refusal comes before any device call: the pointers (16, 32, ... or NULL) are never followed
OK = dict(x=16, out=32, rows=2, cols=100, in_row=100, out_row=100, dtype=0, sigma=48, keys=64, lengths=80, seed=1, lo=-1.0, hi=1.0)


@pytest.mark.parametrize("change", [
    dict(x=None), dict(out=None), dict(sigma=None), dict(rows=-1), dict(cols=-1), dict(dtype=3), dict(dtype=-1), dict(in_row=99), dict(out_row=99),
    dict(out_row=-100), dict(x=18), dict(out=34), dict(dtype=1, x=17), dict(dtype=2, out=33), dict(sigma=50), dict(keys=68), dict(lengths=84),
    dict(lo=1.0, hi=-1.0), dict(lo=math.nan),
])
def test_bad_arguments_are_refused_without_a_device(change):
    assert _lib.load().raw(NAME, *{**OK, **change}.values(), None) == INVALID


def test_the_statement_is_the_published_philox_and_gives_standard_normals():
    zero = np.zeros(1, dtype=np.uint64)
    assert [int(w[0]) for w in R.philox4x32_10((zero, zero, zero, zero), (0, 0))] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    N = 2**20
    for dtype in (np.float64, np.float32):
        n = R.normals((1 << 32) + 12345, (1 << 33) + 5, N, dtype).astype(np.float64)
        assert np.isfinite(n).all()
        assert abs(n.mean()) <= 6 / math.sqrt(N) and abs(n.var() - 1) <= 6 * math.sqrt(2 / N)
