"""CPU: the mixer entry points (ABI v6 on) are declared in the header, mirrored in ``_lib._SIGNATURES`` and exported by the built library
(its symbol table; no device is touched), and the host-only parts of the Python layer agree with the rule of tests/_mix_ref.py."""
import re
import subprocess

import numpy as np

from lhotse_amd import _lib, build
from lhotse_amd.augmentation import mixed_num_samples, mixed_tail_floats

from test_abi import HEADER, declared_functions

MIX_API = {"hipfeat_mixer_create", "hipfeat_mixer_destroy", "hipfeat_mix_plan", "hipfeat_mix_run"}


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
