"""CPU: hipfeat_wpe_run (additive to ABI v8) is declared in the header under its own export macro, mirrored in ``_lib._WPE_SIGNATURES``,
exported by the built library, and refuses bad arguments before it touches a device."""
import os
import re
import subprocess

from lhotse_amd import _lib, build

from test_abi import HEADER, ROOT

INVALID, UNSUPPORTED = 1, 3


def test_the_entry_point_is_declared_mirrored_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+HIPFEAT_WPE_API\s+HIPFEAT_API\b", text)
    protos = re.findall(r"HIPFEAT_WPE_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\((.*?)\)\s*;", text, flags=re.S)
    assert [name for name, _ in protos] == ["hipfeat_wpe_run"] == list(_lib._WPE_SIGNATURES)
    args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in protos[0][1].split(",")]
    assert _lib._WPE_SIGNATURES["hipfeat_wpe_run"] == ("int", args) and _lib._ADDED_SIGNATURES["hipfeat_wpe_run"] == ("int", args)
    assert "hipfeat_wpe_run" not in _lib._SIGNATURES and _lib.load().raw("hipfeat_abi_version") == _lib.ABI_VERSION == 8
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    assert "hipfeat_wpe_run" in set(re.findall(r" T (hipfeat_\w+)", out))


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipfeat.h"\nint main(void) { float y[2];\n'
                   "  (void)sizeof(hipfeat_wpe_run(y, y, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 10, 3, 3, 0, 0));\n"
                   "  return HIPFEAT_ABI_VERSION == 8 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    run = lambda *a: lib.raw("hipfeat_wpe_run", 8, 16, *a, None)  # noqa: E731  (the pointers are never followed)
    ok = (1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    assert run(*ok, 0, 3, 3, 0) == INVALID and run(*ok, 10, -1, 3, 0) == INVALID and run(*ok, 10, 3, 0, 0) == INVALID and run(*ok, 10, 3, 3, 2) == INVALID
    assert run(1, 0, *ok[2:], 10, 3, 3, 0) == INVALID and run(1, 5, *ok[2:], 13, 3, 3, 0) == UNSUPPORTED and "65" in lib.last_error()
    assert run(1, 4, 1, 40000, *ok[4:], 16, 3, 3, 0) == UNSUPPORTED and "on-chip" in lib.last_error()  # weights alone: 160 000 bytes
