"""The per-row-length entry points (additive to ABI v8): declared inside the stft and grad blocks of the header under their own export
macro, mirrored in ``_lib._RAGGED_SIGNATURES`` and exported by the built library; every refusal returns its status without a launch.

CPU: what needs no handle.  A handle exists only on a gfx950, so the refusals that need one (negative sizes, a length above
``max_samples``, misaligned pointers, a short workspace -- none of which launches anything) and the grid of
``hipfeat_grad_workspace_ragged`` against its Python restatement are marked ``gpu``."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from lhotse_amd import _lib, build

from test_abi import HEADER, ROOT, declared_functions
from test_stream_abi import INVALID, OK, stft_config

RAGGED_API = {"hipfeat_stft_run_ragged", "hipfeat_grad_workspace_ragged", "hipfeat_grad_run_ragged"}
EARLIER = [_lib._SIGNATURES, _lib._LEVEL_SIGNATURES, _lib._COLLATE_SIGNATURES, _lib._SINC_SIGNATURES, _lib._FEATMIX_SIGNATURES, _lib._STATS_SIGNATURES,
           _lib._STFT_SIGNATURES, _lib._STREAM_SIGNATURES, _lib._GRAD_SIGNATURES, _lib._CHANNELS_SIGNATURES, _lib._REVERB_FFT_SIGNATURES]
TOO_SHORT = 4


def test_ragged_entry_points_are_declared_mirrored_and_exported():
    text = open(HEADER).read()
    declared = set(re.findall(r"HIPFEAT_RAGGED_API\s+hipfeat_status\s+(hipfeat_\w+)\s*\(", text))
    assert declared == RAGGED_API == set(_lib._RAGGED_SIGNATURES)
    assert re.search(r"#define\s+HIPFEAT_RAGGED_API\s+HIPFEAT_API\b", text)
    assert RAGGED_API <= set(_lib._ADDED_SIGNATURES)
    assert set(declared_functions()) == set(_lib._SIGNATURES) and len(_lib._SIGNATURES) == 52
    for earlier in EARLIER:
        assert not RAGGED_API & set(earlier)
    assert all(callable(_lib.load().fn(name)) for name in RAGGED_API)
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hipfeat_\w+)", out))
    assert RAGGED_API <= exported and set().union(*EARLIER) <= exported


def test_the_abi_version_is_still_8_and_the_declarations_sit_in_their_blocks_with_their_citation():
    text = open(HEADER).read()
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", text).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version") == 8
    stft = text.index("HIPFEAT_RAGGED_API hipfeat_status hipfeat_stft_run_ragged")
    assert text.index("HIPFEAT_STFT_API hipfeat_status hipfeat_stft_run(") < stft < text.index("---- streaming layers")
    grad = text.index("HIPFEAT_RAGGED_API hipfeat_status hipfeat_grad_run_ragged")
    work = text.index("HIPFEAT_RAGGED_API hipfeat_status hipfeat_grad_workspace_ragged")
    assert text.index("HIPFEAT_GRAD_API hipfeat_status hipfeat_grad_destroy") < work < grad < text.index("---- bulk save path")
    for doc in (text[text.index("hipfeat_stft_run_ragged (additive to ABI v8"): stft], text[text.index("hipfeat_grad_workspace_ragged / hipfeat_grad_run_ragged"): work]):
        for cited in ("layers.py:59-333", "collate_matrices", "x[b, :len_b]", "max_samples", "host array", "before any device call"):
            assert cited.lower() in doc.lower(), cited
    assert not re.findall(r"typedef struct \w+ \{", text[stft: grad])  # no new struct


def test_prototypes_match_the_signature_table():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in sorted(RAGGED_API):
        proto = re.search(r"HIPFEAT_RAGGED_API\s+hipfeat_status\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        args = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in proto.split(",")]
        assert _lib._RAGGED_SIGNATURES[name] == ("int", args), (name, args)
    # the arguments of the uniform twins, plus max_samples in the place of num_samples, the lengths, and the forward's padding value
    twin = {"hipfeat_stft_run_ragged": _lib._STFT_SIGNATURES["hipfeat_stft_run"], "hipfeat_grad_workspace_ragged": _lib._GRAD_SIGNATURES["hipfeat_grad_workspace"],
            "hipfeat_grad_run_ragged": _lib._GRAD_SIGNATURES["hipfeat_grad_run"]}
    for name, (_, args) in twin.items():
        mine = list(_lib._RAGGED_SIGNATURES[name][1])
        mine.remove("const int64_t*")
        if name == "hipfeat_stft_run_ragged":
            mine.remove("float")
        assert mine == args, name


def test_the_header_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "hipfeat.h"\nint main(void) { hipfeat_grad* g = 0; hipfeat_stft* s = 0; float w[4]; float* o = 0; int64_t r = 0, n = 0, l[1];\n'
                   "  w[0] = 1.0f; l[0] = 4;\n"
                   "  (void)sizeof(hipfeat_stft_run_ragged(s, w, 1, 4, 4, l, 0.0f, o, 0, o, 0));\n"
                   "  (void)sizeof(hipfeat_grad_workspace_ragged(g, 1, 4, l, 1 << 20, &r, &n));\n"
                   "  (void)sizeof(hipfeat_grad_run_ragged(g, w, 1, 4, 4, l, w, 0, w, o, 4, o, 0, 0));\n"
                   "  return HIPFEAT_ABI_VERSION == 8 ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_null_handles_are_refused_without_a_device():
    lib = _lib.load()
    lens = np.array([16000], dtype=np.int64)
    sizes = np.full(2, 7, dtype=np.int64)
    assert lib.raw("hipfeat_stft_run_ragged", None, None, 1, 16000, 16000, _lib.addr(lens), 0.0, None, 0, None, None) == INVALID and lib.last_error()
    assert lib.raw("hipfeat_stft_run_ragged", None, None, 0, 0, 0, None, 0.0, None, 0, None, None) == INVALID  # (also with batch == 0)
    assert lib.raw("hipfeat_grad_run_ragged", None, None, 1, 16000, 16000, _lib.addr(lens), None, 0, None, None, 16000, None, 0, None) == INVALID
    assert lib.raw("hipfeat_grad_run_ragged", None, None, 0, 0, 0, None, None, 0, None, None, 0, None, 0, None) == INVALID
    assert lib.raw("hipfeat_grad_workspace_ragged", None, 1, 16000, _lib.addr(lens), 1 << 20, sizes.ctypes.data, sizes.ctypes.data + 8) == INVALID and lib.last_error()


# ---- with a handle: refusals that launch nothing, and the workspace arithmetic ----------------------------------------------------------
N, SHIFT = 400, 160


@pytest.fixture(scope="module")
def handles():
    import torch

    assert torch.cuda.is_available()
    torch.zeros(1, device="cuda")  # (the primary context)
    lib = _lib.load()
    window = np.ones(N, dtype=np.float32)
    made = {}
    for snip in (0, 1):
        for name, create, destroy in (("stft", "hipfeat_stft_create", "hipfeat_stft_destroy"), ("grad", "hipfeat_grad_create_stft", "hipfeat_grad_destroy")):
            out = np.zeros(1, dtype=np.uint64)
            cfg = stft_config(output=_lib.STFT_FRAMES, pad_length=N, snip_edges=snip)
            lib.check(create, _lib.addr(cfg), _lib.addr(window), 0, _lib.addr(out))
            made[name, snip] = (int(out[0]), destroy)
    yield lib, {k: v[0] for k, v in made.items()}
    for handle, destroy in made.values():
        lib.check(destroy, handle)


def num_frames(s, snip):
    return (0 if s < N else 1 + (s - N) // SHIFT) if snip else (s + SHIFT // 2) // SHIFT


def workspace(lens, snip, budget):
    """The documented arithmetic: the uniform call's at T = Tmax."""
    tmax, nr = max([num_frames(s, snip) for s in lens], default=0), (N + 3) & ~3
    if not lens or tmax == 0:
        return 0, 0
    rpp = min(len(lens), max(1, budget // (tmax * nr * 4)))
    return rpp, rpp * tmax * nr


@pytest.mark.gpu
def test_the_workspace_agrees_with_its_restatement_on_a_grid(handles):
    lib, h = handles
    sizes = np.zeros(2, dtype=np.int64)
    row = 100 * N * 4  # one row of 100 frames
    for snip, lens, budget in itertools.product((0, 1), ([], [16000], [16000, 8000, 400], [400, 16000, 15999, 5120, 5280], [399, 0, 17] * 3, [16000] * 7 + [1600]),
                                                (0, 1, row - 1, row, 3 * row + 5, 128 << 20)):
        if not snip and any(s < N for s in lens):
            continue
        a = np.array(lens, dtype=np.int64)
        lib.check("hipfeat_grad_workspace_ragged", h["grad", snip], len(lens), 16000, _lib.addr(a) if lens else None, budget, sizes.ctypes.data, sizes.ctypes.data + 8)
        assert tuple(sizes) == workspace(lens, snip, budget), (snip, lens, budget, tuple(sizes))
        if lens and len(set(lens)) == 1:  # ... and with the uniform entry point on a uniform batch
            uni = np.zeros(2, dtype=np.int64)
            lib.check("hipfeat_grad_workspace", h["grad", snip], len(lens), lens[0], budget, uni.ctypes.data, uni.ctypes.data + 8)
            assert tuple(uni) == tuple(sizes)


@pytest.mark.gpu
def test_every_refusal_with_a_handle_launches_nothing(handles):
    import torch

    lib, h = handles
    x = torch.zeros(2, 4000, device="cuda")
    out = torch.full((2 * 25 * N + 4,), 7.0, device="cuda")
    ws = torch.full((2 * 25 * N + 4,), 7.0, device="cuda")
    lens = np.array([4000, 3000], dtype=np.int64)
    sizes = np.zeros(2, dtype=np.int64)

    def stft(wave=x.data_ptr(), batch=2, smax=4000, stride=4000, le=lens, dst=out.data_ptr(), cap=2 * 25 * N, snip=0):
        return lib.raw("hipfeat_stft_run_ragged", h["stft", snip], wave, batch, smax, stride, None if le is None else _lib.addr(le), 0.0, dst, cap, None, None)

    def grad(wave=x.data_ptr(), batch=2, smax=4000, stride=4000, le=lens, cot=out.data_ptr(), cot_n=2 * 25 * N, dst=x.data_ptr(), dstride=4000, w=ws.data_ptr(),
             w_n=2 * 25 * N, snip=0):
        return lib.raw("hipfeat_grad_run_ragged", h["grad", snip], wave, batch, smax, stride, None if le is None else _lib.addr(le), cot, cot_n, None, dst, dstride, w, w_n,
                       None)

    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    for call in (stft, grad):
        assert call(batch=-1) == INVALID and call(smax=-1) == INVALID and call(le=None) == INVALID and call(stride=3999) == INVALID
        assert call(le=i64(4000, -1)) == INVALID and "row 1" in lib.last_error()
        assert call(le=i64(4001, 4000)) == INVALID and "row 0" in lib.last_error()
        assert call(le=i64(4000, 50)) == TOO_SHORT and "row 1" in lib.last_error()
        assert call(le=i64(4000, 0)) == TOO_SHORT and "row 1" in lib.last_error()
        assert call(wave=None) == INVALID and call(wave=x.data_ptr() + 2) == INVALID
        assert call(batch=0, le=None) == OK
    assert stft(cap=2 * 25 * N - 1) == INVALID and stft(cap=-1) == INVALID and stft(dst=None) == INVALID and stft(dst=out.data_ptr() + 2) == INVALID
    assert grad(cot_n=2 * 25 * N - 1) == INVALID and grad(dst=None) == INVALID and grad(dstride=3999) == INVALID and grad(dst=x.data_ptr() + 1) == INVALID
    assert grad(w_n=25 * N - 1) == INVALID and "workspace" in lib.last_error()  # shorter than one row
    assert grad(w=None) == INVALID and grad(w=ws.data_ptr() + 4) == INVALID and grad(w_n=-1) == INVALID
    assert stft(le=i64(399, 0), snip=1) == OK  # rows without frames are legal with snip_edges: nothing to write
    for bad in ((-1, 4000, lens, 0), (2, -1, lens, 0), (2, 4000, lens, -1), (2, 4000, i64(4000, 4001), 0), (2, 4000, i64(-5, 4000), 0)):
        b, s, le, budget = bad
        assert lib.raw("hipfeat_grad_workspace_ragged", h["grad", 0], b, s, _lib.addr(le), budget, sizes.ctypes.data, sizes.ctypes.data + 8) == INVALID
    assert lib.raw("hipfeat_grad_workspace_ragged", h["grad", 0], 2, 4000, None, 0, sizes.ctypes.data, sizes.ctypes.data + 8) == INVALID
    assert lib.raw("hipfeat_grad_workspace_ragged", h["grad", 0], 2, 4000, _lib.addr(lens), 0, None, sizes.ctypes.data + 8) == INVALID
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (ws == 7.0).all() and not x.any()  # nothing was launched
