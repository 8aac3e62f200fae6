"""CPU: the host side of the bankless sinc resampler (lhotse_amd/csrc/sinc_tables.hpp) through the C shim
tests/native/sinc_tables_capi.cpp, and the banded float64 truth of the GPU tests (tests/_sinc_ref.py).

A  width and W are the reference's arithmetic; per phase the window [i0, i0 + W) holds every tap whose weight in the dense float32 bank of
   ``oracle.resample_ref.sinc_kernel`` is not zero, for 441:160, 160:441, 800:467, 467:800, 8000:4673 and 8000:3501; the header's weights
   (this machine's libm) are the bank's, and ``_sinc_ref.window`` finds the same window on its own;
B  the workgroup table covers every (row, phase, hop) exactly once, for row lengths around a hop and a ``new`` that is no multiple of 256;
C  ``_sinc_ref.resample`` equals ``oracle.resample_ref.resample`` in float64 to 1e-12 where the dense bank is small;
D  the stand-alone program of the shim (its own main, built with -fsanitize=address,undefined) walks the same header over more ratios."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _sinc_ref as SR
from oracle import resample_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "sinc_tables_capi.cpp")
RATIOS = [(441, 160), (160, 441), (800, 467), (467, 800), (8000, 4673), (8000, 3501)]
ROW_DTYPE = np.dtype([("in_off", "<i8"), ("out_off", "<i8"), ("in_len", "<i4"), ("out_len", "<i4"), ("orig", "<i4"), ("nw", "<i4"), ("width", "<i4"),
                      ("tiles", "<i4"), ("hops", "<i4"), ("wg_first", "<i4"), ("base", "<f8"), ("pad", "<i8")])
PHASES, HOPS, MAX_W = 256, 64, 96


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(tempfile.mkdtemp(prefix="sinctab_"), "libsinctab.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", out])
    lib = ctypes.CDLL(out)
    lib.st_supported.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p]
    lib.st_filter.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.st_plan.argtypes = [ctypes.c_longlong] + [ctypes.c_void_p] * 5 + [ctypes.c_longlong] + [ctypes.c_void_p] * 5
    lib.st_walk.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def dims_of(shim, src, dst):
    d = np.zeros(4, dtype=np.int32)
    return shim.st_supported(src, dst, d.ctypes.data), d.tolist()


def filter_of(shim, orig, new, W):
    first, w = np.zeros(new, dtype=np.int32), np.zeros((new, W), dtype=np.float32)
    shim.st_filter(orig, new, first.ctypes.data, w.ctypes.data)
    return first, w


def ulps_apart(a, b):
    """float32 arrays -> how many units in the last place each pair lies apart (+0 and -0: none)"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def test_constants_are_what_the_python_side_and_the_header_say(shim):
    from lhotse_amd import augmentation as A

    assert [shim.st_constants(k) for k in range(3)] == [PHASES, HOPS, MAX_W] and A.SINC_MAX_WINDOW == MAX_W
    assert ROW_DTYPE.itemsize == 64


@pytest.mark.parametrize("orig,new", RATIOS, ids=["%d:%d" % r for r in RATIOS])
def test_the_window_holds_every_non_zero_weight_of_the_dense_bank(shim, orig, new):
    bank, width, o, n = OR.sinc_kernel(2 * orig, 2 * new)  # (unreduced rates in, reduced out)
    assert (o, n) == (orig, new) and bank.dtype == np.float32 and bank.shape == (new, 2 * width + orig)
    st, (d_orig, d_new, d_width, W) = dims_of(shim, 2 * orig, 2 * new)
    assert st == 0 and (d_orig, d_new, d_width, W) == (orig, new, width, 2 * width + 2) and SR.geometry(2 * orig, 2 * new) == (orig, new, width)
    first, w = filter_of(shim, orig, new, W)
    kw = bank.shape[1]
    taps = np.arange(kw)[None, :]
    inside = (taps >= first[:, None]) & (taps < first[:, None] + W)
    assert not np.any((bank != 0) & ~inside), "a non-zero weight outside the window"
    assert int((bank != 0).sum(axis=1).max()) <= 2 * width + 1
    # the window's own weights are the bank's (taps the bank does not have: zero), value for value up to the two libms
    cols = first[:, None] + np.arange(W)[None, :]
    exists = (cols >= 0) & (cols < kw)
    want = np.where(exists, bank[np.arange(new)[:, None], np.clip(cols, 0, kw - 1)], np.float32(0))
    apart = ulps_apart(w, want)
    nonzero = int((want != 0).sum())
    print(f"{orig}:{new}: {nonzero} non-zero weights, {int((apart > 0).sum())} differ from numpy's, at most {int(apart.max())} ulp")
    assert apart.max() <= 1 and (apart > 0).sum() <= 1e-4 * nonzero
    assert np.all(w[~exists] == 0)
    # the truth of the GPU tests finds the same window by itself, with the same weights
    r_first, r_w, r_width, r_orig, r_new = SR.window(2 * orig, 2 * new)
    assert (r_width, r_orig, r_new) == (width, orig, new) and np.array_equal(r_first, first) and r_w.shape == (new, W)
    r_apart = ulps_apart(r_w.astype(np.float32), want)
    assert r_apart.max() <= 1 and (r_apart > 0).sum() <= 1e-4 * nonzero


def test_the_support_rule(shim):
    assert dims_of(shim, 48000, 7000) == (0, [48, 7, 42, 86])  # the low end of the default cutoffs at 48 kHz
    assert dims_of(shim, 16000, 9346) == (0, [8000, 4673, 11, 24]) and dims_of(shim, 9346, 16000) == (0, [4673, 8000, 7, 16])
    assert dims_of(shim, 7, 16)[0] == 0 and dims_of(shim, 11127, 16000) == (0, [11127, 16000, 7, 16])
    st, d = dims_of(shim, 48000, 6000)  # width 49: W = 100 > 96
    assert st == 3 and d == [8, 1, 49, 100]
    assert dims_of(shim, 775, 100)[0] == 0 and dims_of(shim, 776, 100)[0] == 3  # the cap in terms of the ratio: 7.75
    for bad in ((0, 16000), (16000, 0), (-1, 16000), (16000, 16000)):
        assert dims_of(shim, *bad)[0] == 1
    assert dims_of(shim, 2 ** 24 + 1, 2 ** 24)[0] == 3  # reduced rates beyond 2^24: (float)ph would round


def plan(shim, in_off, in_len, src, dst, out_off, arena):
    io, il, oo = (np.ascontiguousarray(v, dtype=np.int64) for v in (in_off, in_len, out_off))
    s, d = np.ascontiguousarray(src, dtype=np.int32), np.ascontiguousarray(dst, dtype=np.int32)
    n = len(io)
    out_len, info, rows, nrows = np.full(n, -7, np.int64), np.full(4, -7, np.int64), np.zeros(n, ROW_DTYPE), np.zeros(1, np.int64)
    msg = ctypes.create_string_buffer(256)
    st = shim.st_plan(n, io.ctypes.data, il.ctypes.data, s.ctypes.data, d.ctypes.data, oo.ctypes.data, arena, out_len.ctypes.data, info.ctypes.data,
                      rows.ctypes.data, nrows.ctypes.data, ctypes.addressof(msg))
    return st, out_len, info, rows[: int(nrows[0])], msg.value.decode()


@pytest.mark.parametrize("orig,new", [(441, 160), (800, 467), (8000, 4673), (7, 16), (4673, 8000)], ids=lambda v: str(v))
def test_the_workgroup_table_covers_every_output_sample_once(shim, orig, new):
    lens = [0, 1, orig - 1, orig, orig + 1, 70 * orig + 3]
    in_off = np.arange(len(lens), dtype=np.int64) * (1 << 20)
    out_off = in_off + (1 << 30)
    st, out_len, info, rows, msg = plan(shim, in_off, lens, [3 * orig] * len(lens), [3 * new] * len(lens), out_off, 1 << 31)
    assert st == 0, msg
    assert out_len.tolist() == [OR.resampled_length(n, orig, new) for n in lens]
    assert len(rows) == len(lens) - 1 and rows["in_len"].tolist() == lens[1:]  # the row of no samples takes no workgroup
    width = SR.geometry(orig, new)[2]
    assert set(rows["width"].tolist()) == {width} and info[3] == 2 * width + 2 and set(rows["base"].tolist()) == {min(orig, new) * 0.99}
    assert rows["tiles"].tolist() == [-(-min(new, int(o)) // PHASES) for o in rows["out_len"]]
    assert rows["hops"].tolist() == [-(-int(o) // new) for o in rows["out_len"]]
    wgs = rows["tiles"].astype(np.int64) * -(-rows["hops"].astype(np.int64) // HOPS)
    assert rows["wg_first"].tolist() == (np.cumsum(wgs) - wgs).tolist() and info[2] == wgs.sum()
    assert info[1] == max(int(o + n) for o, n in zip(out_off, out_len))
    counts = [np.zeros(int(o), dtype=np.int32) for o in rows["out_len"]]
    scratch = np.zeros(int(rows["out_len"].max()), dtype=np.int32)
    for wg in range(int(info[2])):
        scratch[:] = 0
        r = shim.st_walk(rows.ctypes.data, len(rows), wg, scratch.ctypes.data)
        assert r >= 0 and not scratch[len(counts[r]):].any()
        counts[r] += scratch[: len(counts[r])]
    assert all((c == 1).all() for c in counts)
    assert shim.st_walk(rows.ctypes.data, len(rows), int(info[2]), scratch.ctypes.data) == -1


@pytest.mark.parametrize("src,dst", [(44100, 16000), (16000, 9340)], ids=["441:160", "800:467"])
def test_the_banded_truth_equals_the_dense_oracle_in_float64(src, dst):
    rng = np.random.RandomState(5)
    for n in (0, 1, 2, 37, 799, 800, 801, 4673, 16000):
        x = rng.uniform(-0.5, 0.5, n)
        got, want = SR.resample(x, src, dst), OR.resample(x, src, dst, dtype=np.float64)
        assert got.shape == want.shape and (n == 0 or np.abs(got - want).max() <= 1e-12), n


def test_stand_alone_program_of_the_shim(tmp_path):
    exe = str(tmp_path / "sinctab")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSINC_TABLES_MAIN", SHIM, "-o", exe])
    # (bounds and overflow are what is looked for; the leak check at exit needs ptrace, which not every container grants)
    res = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
