"""CPU: the reverb entry points (ABI v7 on) are declared in the header, mirrored in ``_lib._SIGNATURES`` and exported by the built library
(its symbol table; no device is touched), and the host-only parts of the Python layer follow their rules."""
import re
import subprocess

import numpy as np
import pytest

from lhotse_amd import _lib, build

from test_abi import HEADER, declared_functions

REVERB_API = {"hipfeat_reverb_create", "hipfeat_reverb_destroy", "hipfeat_reverb_plan", "hipfeat_reverb_run"}


def test_reverb_entry_points_are_declared_mirrored_and_exported():
    names = set(declared_functions())
    assert REVERB_API <= names and REVERB_API <= set(_lib._SIGNATURES)
    assert names == set(_lib._SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    assert REVERB_API <= set(re.findall(r" T (hipfeat_\w+)", out))


def test_abi_version_agrees_everywhere_and_knows_the_reverb():
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version")
    assert header >= 7  # the reverb entry points arrived with version 7


def test_prototypes_match_the_signature_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(REVERB_API):
        proto = re.search(r"HIPFEAT_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert args == _lib._SIGNATURES[name][1], (name, args)


def test_the_library_links_the_hip_runtime_only():
    out = subprocess.run(["readelf", "-d", str(build.build())], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[(.*?)\]", out)
    assert any(n.startswith("libamdhip64") for n in needed)
    assert not [n for n in needed if re.match(r"lib(hipfft|rocfft|rocblas|hipblas|MIOpen)", n)], needed


def test_tail_floats_scaling_and_items_follow_their_rules():
    from lhotse_amd.augmentation import HipReverbWithImpulseResponse, reverb_items, reverb_tail_floats, scaled_rir

    assert reverb_tail_floats([1, 4, 5, 4097]) == 4 + 4 + 8 + 4100 + 3
    assert isinstance(reverb_tail_floats([7]), int) and reverb_tail_floats([]) == 3
    rir = np.array([3, -32768, 32767, 5, 32767], dtype=np.float32) / np.float32(32768.0)
    hs, shift = scaled_rir(rir)
    assert hs.dtype == np.float32 and shift == 2  # the first index of the maximum of the VALUES (np.argmax), not of the magnitudes
    assert np.array_equal(hs.astype(np.float64), rir.astype(np.float64) * 2.0 ** -15)  # the scaling is exact
    # the four cases of the reference (mono / multi-channel input x mono / multi-channel RIR) as (input channel, rir channel) items
    assert reverb_items(1, 1) == [(0, 0)]
    assert reverb_items(1, 3) == [(0, 0), (0, 1), (0, 2)]
    assert reverb_items(2, 1) == [(0, 0), (1, 0)]
    assert reverb_items(2, 2) == [(0, 0), (1, 1)]
    with pytest.raises(ValueError):
        reverb_items(2, 3)
    with pytest.raises(ValueError):
        reverb_items(1, 2, rir_given=False)
    with pytest.raises(_lib.HipFeatError) as e:
        HipReverbWithImpulseResponse(rir=None)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    tf = HipReverbWithImpulseResponse(rir=np.zeros((2, 8), np.float32), rir_channels=[1], early_only=True)
    assert tf.reverse_timestamps(0.25, 1.5, 16000) == (0.25, 1.5) and tf.reverse_timestamps(0.0, None, None) == (0.0, None)
    assert type(tf).__name__ in type(tf).KNOWN_TRANSFORMS or "HipReverbWithImpulseResponse" in tf.KNOWN_TRANSFORMS
