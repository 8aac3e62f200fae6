"""CPU: the three entry points of the ragged WPE chain (additive to ABI v8) are declared under their own export macro, mirrored in
``_lib._WPESTFT_SIGNATURES``, exported by the built library, and refuse bad arguments before they touch a device."""
import os
import re
import subprocess

import pytest

from lhotse_amd import _lib, build

from test_abi import HEADER, ROOT

INVALID, UNSUPPORTED = 1, 3
NAMES = ["hipfeat_wpe_stft_run", "hipfeat_wpe_run_ragged", "hipfeat_wpe_istft_run"]


def test_the_entry_points_are_declared_mirrored_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+HIPFEAT_WPESTFT_API\s+HIPFEAT_API\b", text)
    protos = re.findall(r"HIPFEAT_WPESTFT_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\((.*?)\)\s*;", text, flags=re.S)
    assert [name for name, _ in protos] == NAMES == list(_lib._WPESTFT_SIGNATURES)
    for name, arglist in protos:
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in arglist.split(",")]
        assert _lib._WPESTFT_SIGNATURES[name] == ("int", args) == _lib._ADDED_SIGNATURES[name]
        assert name not in _lib._SIGNATURES and name not in _lib._WPE_SIGNATURES
    assert _lib.load().raw("hipfeat_abi_version") == _lib.ABI_VERSION == 8
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (hipfeat_\w+)", out))


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipfeat.h"\nint main(void) { float y[2]; int32_t n[1];\n'
                   "  (void)sizeof(hipfeat_wpe_stft_run(y, 1, 1, 1, 1, 1, n, y, 512, 128, y, 1, 1, 1, 1, n, 0));\n"
                   "  (void)sizeof(hipfeat_wpe_run_ragged(y, y, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 10, 3, 3, 0, n, 0));\n"
                   "  (void)sizeof(hipfeat_wpe_istft_run(y, 1, 1, 1, 1, 1, 1, n, y, 512, 128, y, 1, 1, 1, 0));\n"
                   "  return HIPFEAT_ABI_VERSION == 8 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


# every refusal comes before any device call: the pointers (8, 16, ... or NULL) are never followed
STFT_OK = dict(audio=8, batch=2, channels=1, row=4000, chan=4000, samples=4000, lengths=16, window=24, n_fft=512, hop=128, out=32, o_row=1, o_bin=1, o_frame=1,
               frames_max=32, frames=40)
ISTFT_OK = dict(z=8, batch=2, channels=1, i_row=1, i_bin=1, i_frame=1, frames_max=32, frames=16, window=24, n_fft=512, hop=128, out=32, o_row=1, o_chan=1,
                out_samples=3968)
CORE_OK = dict(y=8, out=16, batch=1, channels=1, bins=1, frames=1, s0=1, s1=1, s2=1, s3=1, s4=1, s5=1, taps=10, delay=3, its=3, mode=0, table=24)


@pytest.mark.parametrize("name,ok,change,status", [
    ("hipfeat_wpe_stft_run", STFT_OK, dict(channels=0), INVALID),
    ("hipfeat_wpe_stft_run", STFT_OK, dict(samples=-1), INVALID),
    ("hipfeat_wpe_stft_run", STFT_OK, dict(frames_max=33), INVALID),  # 4000 samples have 32 frames at the most
    ("hipfeat_wpe_stft_run", STFT_OK, dict(n_fft=384, hop=96), UNSUPPORTED),
    ("hipfeat_wpe_stft_run", STFT_OK, dict(hop=100), UNSUPPORTED),
    ("hipfeat_wpe_stft_run", STFT_OK, dict(n_fft=4096, hop=1024), UNSUPPORTED),
    ("hipfeat_wpe_stft_run", STFT_OK, dict(lengths=None), INVALID),
    ("hipfeat_wpe_stft_run", STFT_OK, dict(window=None), INVALID),
    ("hipfeat_wpe_stft_run", STFT_OK, dict(out=36), INVALID),  # complex64 on a 4-byte boundary
    ("hipfeat_wpe_stft_run", STFT_OK, dict(batch=1 << 30, frames_max=1), UNSUPPORTED),  # workgroups
    ("hipfeat_wpe_istft_run", ISTFT_OK, dict(batch=-1), INVALID),
    ("hipfeat_wpe_istft_run", ISTFT_OK, dict(out_samples=-1), INVALID),
    ("hipfeat_wpe_istft_run", ISTFT_OK, dict(n_fft=512, hop=512), UNSUPPORTED),
    ("hipfeat_wpe_istft_run", ISTFT_OK, dict(frames=None), INVALID),
    ("hipfeat_wpe_istft_run", ISTFT_OK, dict(z=None), INVALID),
    ("hipfeat_wpe_istft_run", ISTFT_OK, dict(out=34), INVALID),
    ("hipfeat_wpe_run_ragged", CORE_OK, dict(table=None), INVALID),
    ("hipfeat_wpe_run_ragged", CORE_OK, dict(taps=0), INVALID),
    ("hipfeat_wpe_run_ragged", CORE_OK, dict(channels=5, taps=13), UNSUPPORTED),
    ("hipfeat_wpe_run_ragged", CORE_OK, dict(y=None), INVALID),
])
def test_bad_arguments_are_refused_without_a_device(name, ok, change, status):
    assert _lib.load().raw(name, *{**ok, **change}.values(), None) == status
