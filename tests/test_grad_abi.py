"""CPU: the gradient entry points (additive to ABI v8) are declared in the header with their own export macro, mirrored in
``_lib._GRAD_SIGNATURES`` and exported by the built library; no config struct was added; every refusal that needs no device returns its
status without one; and ``differentiable_()`` is a private flag that pickling keeps and nothing else shows."""
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch

import lhotse_amd
from lhotse_amd import _lib, build

from test_abi import HEADER, ROOT, declared_functions
from test_stream_abi import FAR, HIP, INVALID, OK, UNSUPPORTED, feature_config, stft_config

GRAD_API = {"hipfeat_grad_create_features", "hipfeat_grad_create_stft", "hipfeat_grad_workspace", "hipfeat_grad_run", "hipfeat_grad_destroy"}
EARLIER = [_lib._SIGNATURES, _lib._LEVEL_SIGNATURES, _lib._COLLATE_SIGNATURES, _lib._SINC_SIGNATURES, _lib._FEATMIX_SIGNATURES, _lib._STATS_SIGNATURES,
           _lib._STFT_SIGNATURES, _lib._STREAM_SIGNATURES]


def test_grad_entry_points_are_declared_mirrored_and_exported():
    text = open(HEADER).read()
    declared = set(re.findall(r"HIPFEAT_GRAD_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\(", text))
    assert declared == GRAD_API == set(_lib._GRAD_SIGNATURES)
    assert re.search(r"#define\s+HIPFEAT_GRAD_API\s+HIPFEAT_API\b", text)
    assert GRAD_API <= set(_lib._ADDED_SIGNATURES)
    assert set(declared_functions()) == set(_lib._SIGNATURES) and len(_lib._SIGNATURES) == 52
    for earlier in EARLIER:
        assert not GRAD_API & set(earlier)
    assert not re.search(r"HIPFEAT_(STFT_|STREAM_)?API\s+hipfeat_status\s+hipfeat_grad_", text)  # nothing new under an older macro
    assert all(callable(_lib.load().fn(name)) for name in GRAD_API)
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hipfeat_\w+)", out))
    assert GRAD_API <= exported and set().union(*EARLIER) <= exported


def test_the_abi_version_is_still_8_the_block_follows_the_streaming_block_and_states_the_backward():
    text = open(HEADER).read()
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", text).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version") == 8
    start = text.index("v8 libraries built from this commit on also carry hipfeat_grad_*")
    assert start > text.index("HIPFEAT_STREAM_API hipfeat_status hipfeat_stream_destroy")
    doc = text[start: text.index("typedef struct hipfeat_grad hipfeat_grad;")]
    for cited in ("1. seed", "2. adjoint FFT", "3. front end", "4. overlap-add", "layers.py:155-157", "layers.py:859-870", "layers.py:165-167", "layers.py:317, 399, 470",
                  "layers.py:575", "layers.py:708-722", "layers.py:747-772", "Gbar = 2 Pbar X", "Mbar X / |X|", "ybar / (P + 1e-15)", "[mel_m > eps] / mel_m",
                  "e^{+2 pi i k n / fft}", "no direct DFT", "-c pbar_0", "exactly 0.0", "No atomics", "Nr = (N + 3) & ~3", "HIPFEAT_ERR_UNSUPPORTED", "HIPFEAT_ERR_INVALID",
                  "HIPFEAT_ERR_TOO_SHORT", "batch == 0 is", "No new config struct", "a + ib"):
        assert cited in doc, cited


def test_prototypes_match_the_signature_table_and_no_struct_was_added():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(GRAD_API):
        proto = re.search(r"HIPFEAT_GRAD_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert _lib._GRAD_SIGNATURES[name] == ("int", args), (name, args)
    assert _lib.STFT_CONFIG_DTYPE.itemsize == 44 and _lib.CONFIG_DTYPE.itemsize == 76
    block = text.split("typedef struct hipfeat_stream hipfeat_stream;")[1].split("typedef struct hipfeat_archive hipfeat_archive;")[0]
    assert "hipfeat_grad_run" in block and not re.findall(r"typedef struct \w+ \{", block)


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipfeat.h"\nint main(void) { hipfeat_grad* g = 0; hipfeat_grad** p = 0; hipfeat_stft_config c; hipfeat_config f; float w[4];\n'
                   "  float* o = 0; int64_t r = 0, n = 0; c.struct_size = (int32_t)sizeof(c); f.struct_size = (int32_t)sizeof(f); w[0] = 1.0f;\n"
                   "  (void)sizeof(hipfeat_grad_create_stft(&c, w, 0, p)); (void)sizeof(hipfeat_grad_create_features(&f, w, w, w, w, 0, p));\n"
                   "  (void)sizeof(hipfeat_grad_workspace(g, 1, 16000, 1 << 20, &r, &n)); (void)sizeof(hipfeat_grad_destroy(g));\n"
                   "  (void)sizeof(hipfeat_grad_run(g, w, 1, 4, 4, w, 0, w, o, 4, o, 0, 0));\n"
                   "  return HIPFEAT_ABI_VERSION == 8 && sizeof(hipfeat_stft_config) == 44 && sizeof(hipfeat_config) == 76 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_every_refusal_of_create_stft_comes_before_any_device_call():
    lib = _lib.load()
    window = np.ones(2049, dtype=np.float32)
    out = np.full(1, 7, dtype=np.uint64)

    def create(cfg, win=window, dst=out):
        out[0] = 7
        return lib.raw("hipfeat_grad_create_stft", None if cfg is None else _lib.addr(cfg), None if win is None else _lib.addr(win), FAR,
                       None if dst is None else _lib.addr(dst))

    assert create(stft_config(), dst=None) == INVALID
    for bad in (None, stft_config(struct_size=40), stft_config(pad_length=399), stft_config(frame_shift=0), stft_config(frame_length=0, pad_length=0),
                stft_config(output=2), stft_config(output=-1)):
        assert create(bad) == INVALID and out[0] == 0 and lib.last_error(), bad
    assert create(stft_config(), win=None) == INVALID and out[0] == 0
    for fft, n in ((400, 400), (128, 100), (4096, 2400), (768, 400)):
        assert create(stft_config(pad_length=fft, frame_length=n, frame_shift=n // 2)) == UNSUPPORTED and out[0] == 0 and str(fft) in lib.last_error()
    assert create(stft_config(output=0, frame_length=2049, pad_length=2049)) == UNSUPPORTED and out[0] == 0
    assert create(stft_config(frame_shift=401)) == UNSUPPORTED and out[0] == 0
    # the refusals are those of the streaming handle, word for word
    for cfg in (stft_config(struct_size=48), stft_config(pad_length=768), stft_config(frame_shift=401), stft_config(output=0, frame_length=2049, pad_length=2049)):
        one = (create(cfg), lib.last_error())
        two = (lib.raw("hipfeat_stream_create_stft", _lib.addr(cfg), _lib.addr(window), FAR, _lib.addr(out)), lib.last_error())
        assert one == two
    # what is supported gets as far as the device: on a machine without one that is a HIP error
    for fft, n in ((256, 200), (512, 400), (1024, 551), (2048, 1200)):
        assert create(stft_config(pad_length=fft, frame_length=n)) == HIP and out[0] == 0
    for pad in (400, 401, 512, 3000):
        assert create(stft_config(output=0, pad_length=pad)) == HIP and out[0] == 0


def test_every_refusal_of_create_features_comes_before_any_device_call():
    lib = _lib.load()
    window = np.ones(2048, dtype=np.float32)
    mel = np.zeros((1025, 128), dtype=np.float32)
    dct = np.zeros((128, 40), dtype=np.float32)
    lifter = np.ones(40, dtype=np.float32)
    out = np.full(1, 7, dtype=np.uint64)

    def create(cfg, win=window, m=mel, d=dct, li=lifter, dst=out):
        out[0] = 7
        a = lambda v: None if v is None else _lib.addr(v)  # noqa: E731
        return lib.raw("hipfeat_grad_create_features", a(cfg), a(win), a(m), a(d), a(li), FAR, a(dst))

    assert create(feature_config(), dst=None) == INVALID
    for bad in (None, feature_config(struct_size=72), feature_config(kind=-1), feature_config(kind=6), feature_config(frame_length=0), feature_config(frame_shift=0),
                feature_config(fft_length=399), feature_config(num_filters=0), feature_config(kind=3, num_filters=23, num_ceps=0)):
        assert create(bad) == INVALID and out[0] == 0 and lib.last_error(), bad
    assert create(feature_config(), win=None) == INVALID and create(feature_config(), m=None) == INVALID
    assert create(feature_config(kind=3, num_filters=23, num_ceps=13), d=None) == INVALID
    assert create(feature_config(kind=3, num_filters=23, num_ceps=13, apply_lifter=1), li=None) == INVALID
    for bad in (feature_config(kind=4, fft_length=400), feature_config(kind=5), feature_config(fft_length=400), feature_config(fft_length=4096),
                feature_config(fft_length=128, frame_length=100, frame_shift=40), feature_config(num_filters=129), feature_config(frame_shift=401),
                feature_config(dither=1.0)):
        assert create(bad) == UNSUPPORTED and out[0] == 0 and lib.last_error(), bad
    for cfg in (feature_config(), feature_config(kind=0, num_filters=0), feature_config(kind=1, num_filters=0, fft_length=2048, frame_length=1200, frame_shift=480),
                feature_config(kind=3, num_filters=40, num_ceps=40, apply_lifter=1), feature_config(fft_length=256, frame_length=200, frame_shift=80, num_filters=23)):
        assert create(cfg) == HIP and out[0] == 0


def test_null_handles_are_refused_without_a_device():
    lib = _lib.load()
    sizes = np.full(2, 7, dtype=np.int64)
    assert lib.raw("hipfeat_grad_run", None, None, 1, 16000, 16000, None, 0, None, None, 16000, None, 0, None) == INVALID
    assert lib.raw("hipfeat_grad_run", None, None, 0, 0, 0, None, 0, None, None, 0, None, 0, None) == INVALID  # (also with batch == 0)
    assert lib.raw("hipfeat_grad_workspace", None, 1, 16000, 1 << 20, sizes.ctypes.data, sizes.ctypes.data + 8) == INVALID and lib.last_error()
    assert lib.raw("hipfeat_grad_destroy", None) == OK


@pytest.mark.parametrize("name", lhotse_amd.layers.__all__)
def test_differentiable_is_a_private_flag_that_pickling_keeps(name):
    layer = getattr(lhotse_amd, name)()
    before = (set(vars(layer)), repr(layer), set(layer.state_dict()))
    assert layer.differentiable is False
    with pytest.raises(NotImplementedError, match=f"{name} is inference-only \\(no autograd\\); call it under torch.no_grad\\(\\) or detach the input"):
        layer(torch.zeros(2, 1600, requires_grad=True))
    assert layer.differentiable_() is layer and layer.differentiable is True
    assert set(vars(layer)) - before[0] == {"_differentiable"} and repr(layer) == before[1] and set(layer.state_dict()) == before[2]
    assert not [k for k in vars(layer) if not k.startswith("_") and "differentiable" in k]
    with pytest.raises(AttributeError):
        layer.differentiable = False
    copy = pickle.loads(pickle.dumps(layer))
    assert copy.differentiable is True and pickle.loads(pickle.dumps(getattr(lhotse_amd, name)())).differentiable is False
    # on: an input that asks for a gradient gets as far as the device (there is no CPU fallback); one that does not takes the plain path
    with pytest.raises(_lib.HipFeatError, match="no CPU fallback|'cuda"):
        layer(torch.zeros(2, 1600, requires_grad=True))
    with pytest.raises(TypeError, match="float32"):
        layer(torch.zeros(2, 1600, dtype=torch.float64, requires_grad=True))
    with pytest.raises(NotImplementedError, match="inference-only"):
        layer.online_inference(torch.zeros(2, 1600, requires_grad=True))
    assert layer.differentiable_(False) is layer and layer.differentiable is False
    with pytest.raises(NotImplementedError, match="inference-only"):
        layer(torch.zeros(2, 1600, requires_grad=True))
