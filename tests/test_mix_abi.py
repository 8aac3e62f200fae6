"""CPU: the mixer entry points (ABI v6 on) are declared in the header, mirrored in ``_lib._SIGNATURES`` and exported by the built library
(its symbol table; no device is touched), and the host-only parts of the Python layer agree with the rule of tests/_mix_ref.py; the
launch constants the large GPU shapes of the augmentation chain sit on are what the sources say."""
import os
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


def test_launch_constants_the_gpu_shapes_sit_on():
    """tests/test_gpu_reverb.py, test_gpu_mix.py and test_gpu_minibatch.py choose batch sizes ON the limits at which a launch changes its
    path: 3328 bytes of tables (kernel arguments | staged), 24576 (searched in LDS | in HBM), 1792 workgroups (one work item each | a
    second trip of the loop), with 48-byte reverb items and 32-byte mix descriptors.  If a source moves one of them, this fails, so the
    GPU shapes cannot silently stop sitting on the boundaries."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("kernel_minibatch.hpp", "kernel_reverb.hpp", "kernel_mix.hpp", "hipfeat.hip")}

    def constant(name, source):
        return int(re.search(r"constexpr int %s = (\d+)\s*;" % name, text[source]).group(1))

    inline_bytes, lds_bytes = constant("kMbInlineBytes", "kernel_minibatch.hpp"), constant("kMbLdsTableBytes", "kernel_minibatch.hpp")
    assert (inline_bytes, lds_bytes) == (3328, 24576)
    assert "static_assert(sizeof(RvItem) == 48," in text["kernel_reverb.hpp"]
    assert "static_assert(sizeof(MixTrack) == 32 && sizeof(MixCut) == 32," in text["kernel_mix.hpp"]
    assert re.search(r"constexpr int kRvBlock = 256 \* kRvLane;", text["kernel_reverb.hpp"]) and constant("kRvLane", "kernel_reverb.hpp") == 8
    assert (constant("kMixBlock", "kernel_mix.hpp"), constant("kMixEnergyBlock", "kernel_mix.hpp")) == (4096, 16384)
    # the workgroup limit of the three launch functions: grid = ceil(items / ceil(items / 1792))
    hip = text["hipfeat.hip"]
    body = {fn: hip[hip.index('hipfeat_status %s(' % fn) :] for fn in ("hipfeat_minibatch_run", "hipfeat_mix_run", "hipfeat_reverb_run")}
    assert re.search(r"atoi\(exp_env\(\"HIPFEAT_MB_SLOTS\"\)\)\) : 1792;", body["hipfeat_minibatch_run"][:6000])
    assert "per_wg = std::max<int64_t>(1, (items + 1791) / 1792);" in body["hipfeat_mix_run"][:6000]
    assert "per_wg = std::max<int64_t>(1, (s.work_items + 1791) / 1792);" in body["hipfeat_reverb_run"][:6000]
    # every route decision compares with the two table limits, in all three functions
    for fn, b in body.items():
        assert "<= (size_t)kMbInlineBytes" in b[:6000] and "<= (size_t)kMbLdsTableBytes" in b[:9000], fn
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
