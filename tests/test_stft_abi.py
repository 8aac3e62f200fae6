"""CPU: the frame / STFT entry points (additive to ABI v8) are declared in the header with their own export macro, mirrored in
``_lib._STFT_SIGNATURES`` and exported by the built library; every refusal that needs no handle returns its status without a device."""
import os
import re
import subprocess

import numpy as np

import lhotse_amd
from lhotse_amd import _lib, build

from test_abi import HEADER, ROOT, declared_functions

STFT_API = {"hipfeat_stft_create", "hipfeat_stft_destroy", "hipfeat_stft_run"}
EARLIER = [_lib._SIGNATURES, _lib._LEVEL_SIGNATURES, _lib._COLLATE_SIGNATURES, _lib._SINC_SIGNATURES, _lib._FEATMIX_SIGNATURES, _lib._STATS_SIGNATURES]
OK, INVALID, UNSUPPORTED = 0, 1, 3


def test_stft_entry_points_are_declared_mirrored_and_exported():
    text = open(HEADER).read()
    declared = set(re.findall(r"HIPFEAT_STFT_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\(", text))
    assert declared == STFT_API == set(_lib._STFT_SIGNATURES)
    assert re.search(r"#define\s+HIPFEAT_STFT_API\s+HIPFEAT_API\b", text)
    assert STFT_API <= set(_lib._ADDED_SIGNATURES)
    # ... and absent from the v8 set and from the sets added before, which older tests count
    assert set(declared_functions()) == set(_lib._SIGNATURES) and len(_lib._SIGNATURES) == 52
    for earlier in EARLIER:
        assert not STFT_API & set(earlier)
    assert all(callable(_lib.load().fn(name)) for name in STFT_API)  # the loaded library binds them
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hipfeat_\w+)", out))
    assert STFT_API <= exported
    assert set().union(*EARLIER) <= exported  # every earlier export
    for name in ("HipWav2Win", "HipWav2FFT"):
        assert hasattr(lhotse_amd, name) and name in lhotse_amd.__all__ and name in lhotse_amd.layers.__all__


def test_the_abi_version_is_still_8_and_the_header_states_the_arithmetic():
    text = open(HEADER).read()
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", text).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version") == 8
    doc = text[text.index("v8 libraries built from this commit on also carry hipfeat_stft_*"): text.index("typedef struct hipfeat_stft hipfeat_stft;")]
    for cited in ("layers.py:151-197", "layers.py:309-324", "layers.py:727-772", "layers.py:859-870", "j < 0 -> -j - 1, j >= S -> 2 S - 1 - j",
                  "x[i] - c x[max(i - 1, 0)]", "(log_energy, 0)", "256, 512, 1024 or 2048", "there is no direct-DFT", "rows of fft_length + 2 floats",
                  "HIPFEAT_ERR_TOO_SHORT", "HIPFEAT_ERR_UNSUPPORTED"):
        assert cited in doc, cited


def test_prototypes_match_the_signature_table_and_the_struct_its_mirror():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(STFT_API):
        proto = re.search(r"HIPFEAT_STFT_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert _lib._STFT_SIGNATURES[name] == ("int", args), (name, args)
    body = re.search(r"typedef struct hipfeat_stft_config \{(.*?)\} hipfeat_stft_config;", text, flags=re.S).group(1)
    fields = re.findall(r"(int32_t|float)\s+(\w+);", body)
    kinds = {"int32_t": "<i4", "float": "<f4"}
    assert [(n, kinds[t]) for t, n in fields] == [(n, _lib.STFT_CONFIG_DTYPE[n].str) for n in _lib.STFT_CONFIG_DTYPE.names]
    assert _lib.STFT_CONFIG_DTYPE.itemsize == 4 * len(fields) == 44
    assert [int(re.search(r"#define\s+%s\s+(\d+)" % m, text).group(1)) for m in ("HIPFEAT_STFT_FRAMES", "HIPFEAT_STFT_SPECTRUM")] == [
        _lib.STFT_FRAMES, _lib.STFT_SPECTRUM] == [0, 1]


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipfeat.h"\nint main(void) { hipfeat_stft* s = 0; hipfeat_stft** p = 0; hipfeat_stft_config c; float w[4]; float* o = 0;\n'
                   "  c.struct_size = (int32_t)sizeof(c); c.output = HIPFEAT_STFT_SPECTRUM; c.frame_length = 4; c.frame_shift = 2; c.pad_length = 4;\n"
                   "  c.snip_edges = 0; c.remove_dc_offset = 1; c.raw_energy = 1; c.want_energy = 1; c.preemph_coeff = 0.97f; c.energy_floor = 0.0f;\n"
                   "  w[0] = 1.0f; (void)sizeof(hipfeat_stft_create(&c, w, 0, p)); (void)sizeof(hipfeat_stft_destroy(s));\n"
                   "  (void)sizeof(hipfeat_stft_run(s, w, 1, 4, 4, o, 0, o, 0));\n"
                   "  return HIPFEAT_ABI_VERSION == 8 && sizeof(hipfeat_stft_config) == 44 && HIPFEAT_STFT_FRAMES == 0 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def make_config(**kw):
    cfg = np.zeros(1, dtype=_lib.STFT_CONFIG_DTYPE)
    base = dict(struct_size=_lib.STFT_CONFIG_DTYPE.itemsize, output=_lib.STFT_SPECTRUM, frame_length=400, frame_shift=160, pad_length=512, snip_edges=0,
                remove_dc_offset=1, raw_energy=1, want_energy=1, preemph_coeff=0.97, energy_floor=1e-10)
    for k, v in {**base, **kw}.items():
        cfg[k] = v
    return cfg


def test_every_refusal_of_create_comes_before_any_device_call():
    lib = _lib.load()
    window = np.ones(2048, dtype=np.float32)
    out = np.full(1, 7, dtype=np.uint64)

    def create(cfg, win=window, dst=out, device=0):
        out[0] = 7
        return lib.raw("hipfeat_stft_create", None if cfg is None else _lib.addr(cfg), None if win is None else _lib.addr(win), device,
                       None if dst is None else _lib.addr(dst))

    # (device 1 << 20 cannot exist: a status other than the expected one would mean the device was asked first)
    far = 1 << 20
    assert create(make_config(), dst=None, device=far) == INVALID
    for bad in (None, make_config(struct_size=40), make_config(struct_size=48), make_config(pad_length=399), make_config(output=0, pad_length=399),
                make_config(frame_shift=0), make_config(frame_shift=-160), make_config(frame_length=0, pad_length=0), make_config(output=2),
                make_config(output=-1)):
        assert create(bad, device=far) == INVALID and out[0] == 0, bad
        assert lib.last_error()
    assert create(make_config(), win=None, device=far) == INVALID and out[0] == 0  # NULL window
    assert create(make_config(pad_length=399), device=far) == INVALID
    assert "pad_length (or fft_length) = 399 cannot be smaller than N = 400" in lib.last_error()
    # unsupported sizes: every fft length but the four, the non-power-of-two frame length of round_to_power_of_two=False among them
    for fft, n in ((400, 400), (128, 100), (4096, 2400), (768, 400), (513, 400), (64, 50)):
        assert create(make_config(pad_length=fft, frame_length=n), device=far) == UNSUPPORTED and out[0] == 0, fft
        assert str(fft) in lib.last_error()
    assert create(make_config(output=0, frame_length=2049, pad_length=2049), device=far) == UNSUPPORTED and out[0] == 0
    # what is supported gets as far as the device: on a machine without one that is a HIP error, never INVALID / UNSUPPORTED
    for fft, n in ((256, 200), (512, 400), (1024, 551), (2048, 1200)):
        assert create(make_config(pad_length=fft, frame_length=n), device=far) == _lib.ERR_HIP and out[0] == 0
    for pad in (400, 401, 512, 3000):
        assert create(make_config(output=0, pad_length=pad), device=far) == _lib.ERR_HIP and out[0] == 0


def test_null_handles_are_refused_without_a_device():
    lib = _lib.load()
    assert lib.raw("hipfeat_stft_run", None, None, 1, 16000, 16000, None, 0, None, None) == INVALID
    assert lib.raw("hipfeat_stft_run", None, None, 0, 0, 0, None, 0, None, None) == INVALID
    assert lib.raw("hipfeat_stft_destroy", None) == OK


def test_layers_refuse_what_needs_no_device():
    import pytest
    import torch

    with pytest.warns(UserWarning, match="snip_edges=True is generally incompatible with Lhotse"):
        lhotse_amd.HipWav2Win(snip_edges=True)
    with pytest.raises(AssertionError, match="pad_length \\(or fft_length\\) = 399 cannot be smaller than N = 400"):
        lhotse_amd.HipWav2Win(pad_length=399)
    for layer in (lhotse_amd.HipWav2Win(), lhotse_amd.HipWav2FFT()):
        with pytest.raises(_lib.HipFeatError, match="no CPU fallback|'cuda"):
            layer(torch.zeros(2, 16000))
        with pytest.raises(TypeError, match="float32"):
            layer(torch.zeros(2, 16000, dtype=torch.float64))
        with pytest.raises(TypeError, match="torch.Tensor"):
            layer(np.zeros((2, 16000), dtype=np.float32))
        with pytest.raises(NotImplementedError, match="inference-only"):
            layer(torch.zeros(2, 16000, requires_grad=True))
    fft = lhotse_amd.HipWav2FFT(sampling_rate=8000, use_energy=False)
    assert (fft.fft_length, fft.wav2win.pad_length, fft.wav2win.return_log_energy, fft.wav2win._length, fft.wav2win._shift) == (256, 256, False, 200, 80)
    assert lhotse_amd.HipWav2FFT(round_to_power_of_two=False).fft_length == 400
