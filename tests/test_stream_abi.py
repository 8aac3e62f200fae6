"""CPU: the streaming entry points (additive to ABI v8) are declared in the header with their own export macro, mirrored in
``_lib._STREAM_SIGNATURES`` and exported by the built library; ``hipfeat_stream_counts`` is the documented host arithmetic; every refusal
that needs no handle returns its status without a device."""
import itertools
import os
import re
import subprocess

import numpy as np

import lhotse_amd
from lhotse_amd import _lib, build

from test_abi import HEADER, ROOT, declared_functions

STREAM_API = {"hipfeat_stream_counts", "hipfeat_stream_create_features", "hipfeat_stream_create_stft", "hipfeat_stream_run", "hipfeat_stream_destroy"}
EARLIER = [_lib._SIGNATURES, _lib._LEVEL_SIGNATURES, _lib._COLLATE_SIGNATURES, _lib._SINC_SIGNATURES, _lib._FEATMIX_SIGNATURES, _lib._STATS_SIGNATURES,
           _lib._STFT_SIGNATURES]
OK, INVALID, HIP, UNSUPPORTED = 0, 1, 2, 3
FAR = 1 << 20  # a device that cannot exist: a status other than the expected one would mean the device was asked first


def test_stream_entry_points_are_declared_mirrored_and_exported():
    text = open(HEADER).read()
    declared = set(re.findall(r"HIPFEAT_STREAM_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\(", text))
    assert declared == STREAM_API == set(_lib._STREAM_SIGNATURES)
    assert re.search(r"#define\s+HIPFEAT_STREAM_API\s+HIPFEAT_API\b", text)
    assert STREAM_API <= set(_lib._ADDED_SIGNATURES)
    # ... and absent from the v8 set and from the sets added before, which older tests count
    assert set(declared_functions()) == set(_lib._SIGNATURES) and len(_lib._SIGNATURES) == 52
    for earlier in EARLIER:
        assert not STREAM_API & set(earlier)
    assert not re.search(r"HIPFEAT_(STFT_)?API\s+hipfeat_status\s+hipfeat_stream_", text)  # nothing new under an older macro
    assert all(callable(_lib.load().fn(name)) for name in STREAM_API)  # the loaded library binds them
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hipfeat_\w+)", out))
    assert STREAM_API <= exported
    assert set().union(*EARLIER) <= exported  # every earlier export
    assert sorted(lhotse_amd.layers.__all__) == sorted(["HipWav2Win", "HipWav2FFT", "HipWav2Spec", "HipWav2LogSpec", "HipWav2LogFilterBank", "HipWav2MFCC"])
    for name in lhotse_amd.layers.__all__:
        assert callable(getattr(getattr(lhotse_amd, name), "online_inference"))


def test_the_abi_version_is_still_8_the_block_follows_the_stft_block_and_states_the_framing():
    text = open(HEADER).read()
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", text).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version") == 8
    start = text.index("v8 libraries built from this commit on also carry hipfeat_stream_*")
    assert start > text.index("HIPFEAT_STFT_API hipfeat_status hipfeat_stft_run")
    doc = text[start: text.index("typedef struct hipfeat_stream hipfeat_stream;")]
    for cited in ("layers.py:199-224", "326-333", "775-856", "V = [A | x]", "R = min(P, S)", "A(j) = x[R - 1 - j]", "V(j) = A(j) for j < R, x[j - R] otherwise",
                  "T = 1 + (L - N) / s", "V[T s : L]", "L < N: T = 0", "all of V is the remainder", "256, 512, 1024 or 2048", "HIPFEAT_ERR_UNSUPPORTED",
                  "HIPFEAT_ERR_INVALID", "batch == 0 is HIPFEAT_OK"):
        assert cited in doc, cited


def test_prototypes_match_the_signature_table_and_the_config_structs_are_reused_unchanged():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(STREAM_API):
        proto = re.search(r"HIPFEAT_STREAM_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert _lib._STREAM_SIGNATURES[name] == ("int", args), (name, args)
    assert _lib.STFT_CONFIG_DTYPE.itemsize == 44 and _lib.CONFIG_DTYPE.itemsize == 76
    assert len(re.findall(r"typedef struct \w+ \{", text)) == len(re.findall(r"typedef struct \w+ \{", text.split("typedef struct hipfeat_stream hipfeat_stream;")[0]))


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipfeat.h"\nint main(void) { hipfeat_stream* s = 0; hipfeat_stream** p = 0; hipfeat_stft_config c; hipfeat_config f; float w[4];\n'
                   "  float* o = 0; int64_t t = 0, r = 0; c.struct_size = (int32_t)sizeof(c); f.struct_size = (int32_t)sizeof(f); w[0] = 1.0f;\n"
                   "  (void)sizeof(hipfeat_stream_counts(400, 160, 0, 1, 0, 100, &t, &r)); (void)sizeof(hipfeat_stream_create_stft(&c, w, 0, p));\n"
                   "  (void)sizeof(hipfeat_stream_create_features(&f, w, w, w, w, 0, p)); (void)sizeof(hipfeat_stream_destroy(s));\n"
                   "  (void)sizeof(hipfeat_stream_run(s, w, 0, 0, w, 4, 4, 1, o, 0, o, o, 0, 0));\n"
                   "  return HIPFEAT_ABI_VERSION == 8 && sizeof(hipfeat_stft_config) == 44 && sizeof(hipfeat_config) == 76 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def counts(lib, n, s, snip, first, r, chunk):
    out = np.full(2, -7, dtype=np.int64)
    st = lib.raw("hipfeat_stream_counts", n, s, snip, first, r, chunk, out.ctypes.data, out.ctypes.data + 8)
    return st, int(out[0]), int(out[1])


def formula(n, s, snip, first, r, chunk):
    """The issue's statement: A is the context, or at the start of a stream empty (snip_edges) / the flipped first min(P, S) samples."""
    a = (0 if snip else min((n - s) // 2, chunk)) if first else r
    L = a + chunk
    T = 1 + (L - n) // s if L >= n else 0
    return T, L - T * s


def test_counts_agree_with_the_formulas_on_a_grid():
    lib = _lib.load()
    hit = {k: 0 for k in ("S<P", "S=0", "R>2N", "L=N-1", "L=N", "L=N+s-1")}
    for (n, s), snip, first in itertools.product(((400, 160), (200, 80), (551, 220), (1200, 480), (400, 400), (7, 3)), (0, 1), (0, 1)):
        p = (n - s) // 2
        for chunk in sorted({0, 1, max(p - 1, 0), p, p + 1, s, n - 1, n, n + s - 1, n + s, 5 * s + 3, 1234}):
            # (the lengths L = N - 1, N, N + s - 1 through the context as well)
            contexts = [0] if first else sorted({0, 1, n - s, n - 1, n, 2 * n + 3, 5 * n} | {L - chunk for L in (n - 1, n, n + s - 1) if L >= chunk})
            for r in contexts:
                st, T, rem = counts(lib, n, s, snip, first, r, chunk)
                assert st == OK and (T, rem) == formula(n, s, snip, first, r, chunk), (n, s, snip, first, r, chunk, T, rem)
                L = rem + T * s
                assert 0 <= rem < n and (T == 0) == (L < n)
                hit["S<P"] += bool(first and not snip and chunk < p)
                hit["S=0"] += chunk == 0
                hit["R>2N"] += r > 2 * n
                hit["L=N-1"] += L == n - 1
                hit["L=N"] += L == n
                hit["L=N+s-1"] += L == n + s - 1
    assert all(v > 0 for v in hit.values()), hit
    # a first chunk shorter than P reflects only what it has
    assert counts(lib, 400, 160, 0, 1, 0, 50) == (OK, 0, 100) and counts(lib, 400, 160, 0, 1, 0, 400) == (OK, 1, 360)
    assert counts(lib, 400, 160, 1, 1, 0, 400) == (OK, 1, 240)


def test_counts_refusals():
    lib = _lib.load()
    out = np.zeros(2, dtype=np.int64)
    assert lib.raw("hipfeat_stream_counts", 400, 160, 0, 0, 0, 0, None, out.ctypes.data) == INVALID
    assert lib.raw("hipfeat_stream_counts", 400, 160, 0, 0, 0, 0, out.ctypes.data, None) == INVALID
    for args in ((0, 160, 0, 0, 0, 10), (400, 0, 0, 0, 0, 10), (-400, 160, 0, 0, 0, 10), (400, 160, 0, 0, -1, 10), (400, 160, 0, 0, 0, -1),
                 (400, 160, 0, 1, 5, 10)):  # (the start of a stream has no context)
        assert counts(lib, *args)[0] == INVALID and lib.last_error(), args
    assert counts(lib, 160, 400, 0, 0, 0, 10)[0] == UNSUPPORTED


def stft_config(**kw):
    cfg = np.zeros(1, dtype=_lib.STFT_CONFIG_DTYPE)
    base = dict(struct_size=_lib.STFT_CONFIG_DTYPE.itemsize, output=_lib.STFT_SPECTRUM, frame_length=400, frame_shift=160, pad_length=512, snip_edges=0,
                remove_dc_offset=1, raw_energy=1, want_energy=1, preemph_coeff=0.97, energy_floor=1e-10)
    for k, v in {**base, **kw}.items():
        cfg[k] = v
    return cfg


def feature_config(**kw):
    cfg = np.zeros(1, dtype=_lib.CONFIG_DTYPE)
    base = dict(struct_size=_lib.CONFIG_DTYPE.itemsize, kind=2, frame_length=400, frame_shift=160, fft_length=512, num_filters=80, num_ceps=0, snip_edges=0,
                remove_dc_offset=1, use_energy=0, raw_energy=1, use_fft_mag=0, apply_lifter=0, preemph_coeff=0.97, energy_floor=1e-10, mel_floor=1.1920929e-07,
                log_offset=1e-15, dither=0.0, batch_hop=160)
    for k, v in {**base, **kw}.items():
        cfg[k] = v
    return cfg


def test_every_refusal_of_create_stft_comes_before_any_device_call():
    lib = _lib.load()
    window = np.ones(2048, dtype=np.float32)
    out = np.full(1, 7, dtype=np.uint64)

    def create(cfg, win=window, dst=out, device=FAR):
        out[0] = 7
        return lib.raw("hipfeat_stream_create_stft", None if cfg is None else _lib.addr(cfg), None if win is None else _lib.addr(win), device,
                       None if dst is None else _lib.addr(dst))

    assert create(stft_config(), dst=None) == INVALID
    for bad in (None, stft_config(struct_size=40), stft_config(struct_size=48), stft_config(pad_length=399), stft_config(output=0, pad_length=399),
                stft_config(frame_shift=0), stft_config(frame_shift=-160), stft_config(frame_length=0, pad_length=0), stft_config(output=2), stft_config(output=-1)):
        assert create(bad) == INVALID and out[0] == 0, bad
        assert lib.last_error()
    assert create(stft_config(), win=None) == INVALID and out[0] == 0
    for fft, n in ((400, 400), (128, 100), (4096, 2400), (768, 400), (513, 400), (64, 50)):
        assert create(stft_config(pad_length=fft, frame_length=n, frame_shift=n // 2)) == UNSUPPORTED and out[0] == 0, fft
        assert str(fft) in lib.last_error()
    assert create(stft_config(output=0, frame_length=2049, pad_length=2049)) == UNSUPPORTED and out[0] == 0
    assert create(stft_config(frame_shift=401)) == UNSUPPORTED and out[0] == 0
    # what is supported gets as far as the device: on a machine without one that is a HIP error, never INVALID / UNSUPPORTED
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

    def create(cfg, win=window, m=mel, d=dct, li=lifter, dst=out, device=FAR):
        out[0] = 7
        a = lambda v: None if v is None else _lib.addr(v)  # noqa: E731
        return lib.raw("hipfeat_stream_create_features", a(cfg), a(win), a(m), a(d), a(li), device, a(dst))

    assert create(feature_config(), dst=None) == INVALID
    for bad in (None, feature_config(struct_size=72), feature_config(kind=-1), feature_config(kind=6), feature_config(frame_length=0), feature_config(frame_shift=0),
                feature_config(fft_length=399), feature_config(num_filters=0), feature_config(kind=3, num_filters=23, num_ceps=0)):
        assert create(bad) == INVALID and out[0] == 0, bad
        assert lib.last_error()
    assert create(feature_config(), win=None) == INVALID and create(feature_config(), m=None) == INVALID
    assert create(feature_config(kind=3, num_filters=23, num_ceps=13), d=None) == INVALID
    assert create(feature_config(kind=3, num_filters=23, num_ceps=13, apply_lifter=1), li=None) == INVALID
    # unsupported: kinds beyond the four, every fft length but the four, more than 128 filters, a shift longer than the frame, dither
    for bad in (feature_config(kind=4, fft_length=400), feature_config(kind=5), feature_config(fft_length=400), feature_config(fft_length=4096),
                feature_config(fft_length=128, frame_length=100, frame_shift=40), feature_config(num_filters=129), feature_config(frame_shift=401),
                feature_config(dither=1.0)):
        assert create(bad) == UNSUPPORTED and out[0] == 0, bad
        assert lib.last_error()
    for cfg in (feature_config(), feature_config(kind=0, num_filters=0), feature_config(kind=1, num_filters=0, fft_length=2048, frame_length=1200, frame_shift=480),
                feature_config(kind=3, num_filters=40, num_ceps=40, apply_lifter=1), feature_config(fft_length=256, frame_length=200, frame_shift=80, num_filters=23)):
        assert create(cfg) == HIP and out[0] == 0


def test_the_creators_that_share_a_config_refuse_it_with_one_status_and_one_text():
    """hipfeat_stft_create / hipfeat_stream_create_stft and hipfeat_plan_create / hipfeat_stream_create_features check their config
    struct with one piece of code each: a config that breaks one shared rule gets the same status and the same words from both."""
    lib = _lib.load()
    window = np.ones(2049, dtype=np.float32)
    mel = np.zeros((1025, 128), dtype=np.float32)
    dct = np.zeros((128, 40), dtype=np.float32)
    lifter = np.ones(40, dtype=np.float32)
    out = np.full(1, 7, dtype=np.uint64)

    def refusal(name, *tables):
        out[0] = 7
        st = lib.raw(name, *[None if t is None else _lib.addr(t) for t in tables], FAR, _lib.addr(out))
        assert out[0] == 0
        return st, lib.last_error()

    stft = [stft_config(struct_size=40), stft_config(struct_size=48), stft_config(output=-1), stft_config(output=2), stft_config(frame_shift=0),
            stft_config(frame_shift=-160), stft_config(frame_length=0, pad_length=0), stft_config(pad_length=399), stft_config(output=0, pad_length=399),
            stft_config(output=0, frame_length=2049, pad_length=2049)]
    stft += [stft_config(pad_length=fft, frame_length=n, frame_shift=n // 2) for fft, n in ((400, 400), (128, 100), (768, 400), (513, 400), (4096, 2400))]
    for cfg in stft:
        one, two = refusal("hipfeat_stft_create", cfg, window), refusal("hipfeat_stream_create_stft", cfg, window)
        assert one == two and one[0] in (INVALID, UNSUPPORTED) and one[1], (cfg, one, two)

    mfcc = dict(kind=3, num_filters=23, num_ceps=13)
    features = [(feature_config(struct_size=72),), (feature_config(kind=-1),), (feature_config(kind=6),), (feature_config(frame_length=0),),
                (feature_config(frame_shift=0),), (feature_config(fft_length=399),), (feature_config(num_filters=0),),
                (feature_config(kind=3, num_filters=23, num_ceps=0),), (feature_config(), window, None), (feature_config(**mfcc), window, mel, None),
                (feature_config(**mfcc, apply_lifter=1), window, mel, dct, None), (feature_config(frame_shift=401),), (feature_config(dither=1.0),)]
    for cfg, *given in features:
        tables = given + [window, mel, dct, lifter][len(given):]
        one, two = refusal("hipfeat_plan_create", cfg, *tables), refusal("hipfeat_stream_create_features", cfg, *tables)
        assert one == two and one[0] in (INVALID, UNSUPPORTED) and one[1], (cfg, one, two)


def test_null_handles_are_refused_without_a_device():
    lib = _lib.load()
    assert lib.raw("hipfeat_stream_run", None, None, 0, 0, None, 16000, 16000, 1, None, 0, None, None, 0, None) == INVALID
    assert lib.raw("hipfeat_stream_run", None, None, 0, 0, None, 0, 0, 0, None, 0, None, None, 0, None) == INVALID
    assert lib.raw("hipfeat_stream_destroy", None) == OK


def test_layers_refuse_what_needs_no_device():
    import inspect

    import pytest
    import torch

    layers = [getattr(lhotse_amd, name)() for name in lhotse_amd.layers.__all__]
    for layer in layers:
        assert list(inspect.signature(layer.online_inference).parameters) == ["x", "context"]
        assert inspect.signature(layer.online_inference).parameters["context"].default is None
        with pytest.raises(_lib.HipFeatError, match="no CPU fallback|'cuda"):
            layer.online_inference(torch.zeros(2, 1600))
        with pytest.raises(TypeError, match="float32"):
            layer.online_inference(torch.zeros(2, 1600, dtype=torch.float64))
        with pytest.raises(TypeError, match="torch.Tensor"):
            layer.online_inference(np.zeros((2, 1600), dtype=np.float32))
        with pytest.raises(NotImplementedError, match="inference-only"):
            layer.online_inference(torch.zeros(2, 1600, requires_grad=True))
        for bad in (torch.zeros(240), torch.zeros(3, 240), torch.zeros(2, 240, dtype=torch.float64), np.zeros((2, 240), dtype=np.float32)):
            with pytest.raises(AssertionError):
                layer.online_inference(torch.zeros(2, 1600), bad)
