"""CPU: the ``hipfeat_narrowband_*`` entry points (additive to ABI v8) are declared under their own export macro, mirrored in
``_lib._NARROWBAND_SIGNATURES``, exported by the built library and refuse bad arguments before they touch a device; and the tables the
kernel runs on (lhotse_amd/csrc/narrowband_tables.hpp through ``hipfeat_narrowband_tables``) are the windows of tests/_sinc_ref.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _sinc_ref as SR
import lhotse_amd
from lhotse_amd import _lib, build

from test_abi import HEADER, ROOT
from test_sinc_tables import ulps_apart

INVALID, UNSUPPORTED = 1, 3
NAMES = ["hipfeat_narrowband_create", "hipfeat_narrowband_destroy", "hipfeat_narrowband_tables", "hipfeat_narrowband_geometry", "hipfeat_narrowband_run"]


def test_the_entry_points_are_declared_mirrored_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+HIPFEAT_NARROWBAND_API\s+HIPFEAT_API\b", text)
    protos = re.findall(r"HIPFEAT_NARROWBAND_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\((.*?)\)\s*;", text, flags=re.S)
    assert [name for name, _ in protos] == NAMES == list(_lib._NARROWBAND_SIGNATURES)
    for name, params in protos:
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in params.split(",")]
        assert _lib._NARROWBAND_SIGNATURES[name] == ("int", args) == _lib._ADDED_SIGNATURES[name] and name not in _lib._SIGNATURES
    assert len(_lib._SIGNATURES) == 52 and _lib.load().raw("hipfeat_abi_version") == _lib.ABI_VERSION == 8
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (hipfeat_\w+)", out))


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipfeat.h"\nint main(void) { float x[4]; int64_t n[1]; int32_t d[8]; hipfeat_narrowband* h = 0;\n'
                   "  (void)sizeof(hipfeat_narrowband_create(16000, &h)); (void)sizeof(hipfeat_narrowband_run(h, x, x, 1, 4, 4, 4, n, 1, 0));\n"
                   "  (void)sizeof(hipfeat_narrowband_tables(16000, d, x, d, x, d)); (void)sizeof(hipfeat_narrowband_geometry(16000, d));\n"
                   "  return hipfeat_narrowband_destroy(h) == HIPFEAT_OK && HIPFEAT_ABI_VERSION == 8 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)


# every refusal comes before any device call: the handle and the pointers (16, 32, ... or NULL) are never followed
RUN_OK = dict(h=16, x=32, out=48, rows=2, cols=100, in_row=100, out_row=100, lengths=64, restore=1)
CASES = [("run", c, INVALID) for c in (
    dict(h=None), dict(x=None), dict(out=None), dict(rows=-1), dict(cols=-1), dict(cols=2**30 + 1, in_row=2**31, out_row=2**31), dict(in_row=99),
    dict(out_row=-100), dict(x=34), dict(out=50), dict(lengths=68))]
CASES += [("create", (0, 16), INVALID), ("create", (-8000, 16), INVALID), ("create", (16000, None), INVALID), ("create", (7999, 16), UNSUPPORTED),
          ("create", (8001, 16), UNSUPPORTED), ("create", (96000, 16), UNSUPPORTED)]


@pytest.mark.parametrize("entry,change,status", CASES)
def test_bad_arguments_are_refused_without_a_device(entry, change, status):
    lib = _lib.load()
    if entry == "run":
        assert lib.raw("hipfeat_narrowband_run", *{**RUN_OK, **change}.values(), None) == status
    else:
        slot = np.zeros(1, dtype=np.uint64)
        assert lib.raw("hipfeat_narrowband_create", change[0], change[1] and slot.ctypes.data) == status and slot[0] == 0
        assert status == INVALID or str(change[0]) in lib.last_error()  # the message names the rate


@pytest.mark.parametrize("sr", (16000, 44100, 11025, 48000))
def test_the_tables_are_the_windows_of_the_statement(sr):
    lib = _lib.load()
    dims = np.zeros(8, dtype=np.int32)
    lib.check("hipfeat_narrowband_tables", sr, dims.ctypes.data, None, None, None, None)  # NULL buffers: the dims alone
    for k, (src, dst) in enumerate(((sr, 8000), (8000, sr))):
        first, w, width, orig, new = SR.window(src, dst)
        assert dims[4 * k: 4 * k + 4].tolist() == [orig, new, width, 2 * width + 2]
    got = [np.zeros((dims[1], dims[3]), np.float32), np.zeros(dims[1], np.int32), np.zeros((dims[5], dims[7]), np.float32), np.zeros(dims[5], np.int32)]
    lib.check("hipfeat_narrowband_tables", sr, dims.ctypes.data, *[a.ctypes.data for a in got])
    for k, (src, dst) in enumerate(((sr, 8000), (8000, sr))):
        first, w = SR.window(src, dst)[:2]
        assert np.array_equal(got[2 * k + 1], first)
        apart = ulps_apart(got[2 * k], w.astype(np.float32))  # the bar of test_sinc_tables.py: the two libms
        assert apart.max() <= 1 and (apart > 0).sum() <= 1e-4 * int((w != 0).sum())


def test_the_twin_follows_the_reference_constructor():
    with pytest.raises(NotImplementedError):
        lhotse_amd.HipNarrowband("lpc10", 16000, True)
    with pytest.raises(ValueError, match="unsupported codec"):
        lhotse_amd.HipNarrowband("gsm", 16000, True)
    t = lhotse_amd.HipNarrowband("mulaw", 16000, True)
    assert t.reverse_timestamps(1.0, 2.0, 16000) == (1.0, 2.0)
    with pytest.raises(lhotse_amd._lib.HipFeatError, match="no CPU fallback"):
        t(torch.zeros(16))  # (a CPU tensor: refused before any device call)
