"""CPU: the host tables of the gradient kernels (lhotse_amd/csrc/grad_tables.hpp) through tests/native/grad_tables_capi.cpp (plain g++,
ctypes): the banded filterbank in both directions against a dense numpy product and its transpose, the transposed DCT, and the piece
arithmetic of the workspace, a single row over the budget included."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from lhotse_amd import constants

SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "grad_tables_capi.cpp")


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(tempfile.mkdtemp(prefix="gradtab_"), "libgradtab.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", out])
    lib = ctypes.CDLL(out)
    lib.gt_build.restype = ctypes.c_longlong
    lib.gt_build.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong,
                             ctypes.c_void_p]
    lib.gt_pieces.restype = ctypes.c_int
    lib.gt_pieces.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p]
    lib.gt_lds_floats.restype = ctypes.c_longlong
    lib.gt_lds_floats.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.gt_blob_fits.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
    return lib


def build(shim, mel, dct=None, lifter=None):
    K, M = mel.shape
    C = 0 if dct is None else dct.shape[1]
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    offs = np.zeros(4, np.int32)
    n = shim.gt_build(K, M, C, ptr(mel), ptr(dct), ptr(lifter), None, 0, offs.ctypes.data)
    blob = np.full(n, np.nan, np.float32)
    assert shim.gt_build(K, M, C, ptr(mel), ptr(dct), ptr(lifter), blob.ctypes.data, n, offs.ctypes.data) == n
    return blob, offs.tolist()


def banded_products(blob, offs, K, M, power, g):
    """mel_m = sum_k fb[k][m] P_k and Pbar_k = sum_m fb[k][m] g_m the way the kernel walks the blob (float64 accumulation)."""
    words = blob.view(np.int32)
    mel, pbar = np.zeros(M), np.zeros(K)
    for m in range(M):
        lo, length, off, zero = words[offs[0] + 4 * m: offs[0] + 4 * m + 4]
        assert zero == 0 and 0 <= lo and lo + length <= K and off + length <= blob.size
        mel[m] = np.dot(blob[off: off + length].astype(np.float64), power[lo: lo + length])
    for k in range(K):
        lo, length, off, zero = words[offs[1] + 4 * k: offs[1] + 4 * k + 4]
        assert zero == 0 and 0 <= lo and lo + length <= M and off + length <= blob.size
        pbar[k] = np.dot(blob[off: off + length].astype(np.float64), g[lo: lo + length])
    return mel, pbar


@pytest.mark.parametrize("rate,fft,M", [(16000, 512, 80), (8000, 256, 23), (22050, 1024, 40), (44100, 2048, 128)])
def test_banded_filterbank_equals_the_dense_matrix_and_its_transpose(shim, rate, fft, M):
    mel = constants.make_kaldi_mel(M, fft, rate, 20.0, -400.0)
    K = fft // 2 + 1
    blob, offs = build(shim, mel)
    assert offs[0] == 0 and offs[1] == 4 * M and blob.size % 4 == 0 and not np.isnan(blob).any()
    rng = np.random.RandomState(fft)
    power, g = rng.rand(K), rng.standard_normal(M)
    got_mel, got_pbar = banded_products(blob, offs, K, M, power, g)
    dense = mel.astype(np.float64)
    np.testing.assert_allclose(got_mel, power @ dense, rtol=1e-13, atol=1e-300)
    np.testing.assert_allclose(got_pbar, dense @ g, rtol=1e-12, atol=1e-15)
    # a bin lies under at most two triangles: each banded copy holds at most 2 K weights behind the 4 (M + K) descriptor words
    assert blob.size - 4 * (M + K) <= 4 * K + 3
    n = int(0.025 * rate)
    assert shim.gt_blob_fits(fft // 128, n, blob.size) == (1 if fft <= 1024 else 0)  # (at fft 2048 the buffers alone pass the 96 KiB mark)


def test_a_dense_matrix_gets_full_bands_and_is_read_from_global_memory(shim):
    K, M = 1025, 128
    rng = np.random.RandomState(3)
    mel = (rng.rand(K, M) + 0.1).astype(np.float32)
    mel[17, :] = 0.0  # a bin under no filter: an empty band
    mel[:, 5] = 0.0   # a filter without weights
    blob, offs = build(shim, mel)
    power, g = rng.rand(K), rng.standard_normal(M)
    got_mel, got_pbar = banded_products(blob, offs, K, M, power, g)
    np.testing.assert_allclose(got_mel, power @ mel.astype(np.float64), rtol=1e-12)
    np.testing.assert_allclose(got_pbar, mel.astype(np.float64) @ g, rtol=1e-10, atol=1e-12)
    words = blob.view(np.int32)
    assert words[offs[1] + 4 * 17 + 1] == 0 and words[offs[0] + 4 * 5 + 1] == 0
    assert blob.size >= 2 * (K - 1) * (M - 1) and shim.gt_blob_fits(16, 1200, blob.size) == 0  # 1025 x 128 does not fit


def test_dct_is_stored_transposed_with_the_lifter_behind_it(shim):
    M, C = 23, 13
    mel = constants.make_kaldi_mel(M, 512, 16000, 20.0, -400.0)
    dct, lifter = constants.make_dct(C, M), constants.make_lifter(C, 22)
    blob, offs = build(shim, mel, dct, lifter)
    assert np.array_equal(blob[offs[2]: offs[2] + C * M].reshape(C, M), dct.T) and np.array_equal(blob[offs[3]: offs[3] + C], lifter)
    blob, offs = build(shim, mel, dct, None)  # no lifter: ones
    assert np.array_equal(blob[offs[3]: offs[3] + C], np.ones(C, np.float32))
    blob, offs = build(shim, mel)  # fbank: no DCT at all
    assert offs[2] == offs[3]


def pieces(shim, batch, T, N, budget):
    out = np.full(4, -7, np.int64)
    ok = shim.gt_pieces(batch, T, N, budget, out.ctypes.data)
    return ok, out.tolist()


def test_piece_arithmetic(shim):
    # Nr = (N + 3) & ~3; rows_per_piece = max(1, budget / (T Nr 4)), at most the batch
    assert pieces(shim, 48, 1000, 400, 128 << 20) == (1, [400, 400000, 48, 48 * 400000])
    assert pieces(shim, 48, 1000, 401, 128 << 20)[1][0] == 404 and pieces(shim, 1, 10, 551, 1 << 20)[1][0] == 552
    budget = 10 * 400000 * 4
    assert pieces(shim, 48, 1000, 400, budget)[1][2:] == [10, 10 * 400000]
    assert pieces(shim, 48, 1000, 400, budget - 1)[1][2:] == [9, 9 * 400000]
    # a single row over the budget gets a workspace of its own size
    assert pieces(shim, 48, 1000, 400, 16)[1][2:] == [1, 400000] and pieces(shim, 48, 1000, 400, 0)[1][2:] == [1, 400000]
    T = 5_400_000  # one row past 2^31 floats
    ok, (nr, row, rpp, floats) = pieces(shim, 1, T, 400, 128 << 20)
    assert ok and rpp == 1 and floats == row == T * 400 > 2 ** 31
    # nothing to do: no rows, or no frames
    assert pieces(shim, 0, 1000, 400, 1 << 20)[1][2:] == [0, 0] and pieces(shim, 3, 0, 400, 1 << 20)[1][2:] == [0, 0]
    # overflow is refused, not wrapped
    assert pieces(shim, 1, 2 ** 62, 400, 1 << 20)[0] == 0 and pieces(shim, -1, 10, 400, 1 << 20)[0] == 0


def test_lds_floats_are_what_the_kernel_carves(shim):
    for n1, N in ((2, 200), (4, 400), (8, 551), (16, 1200), (16, 2048)):
        assert shim.gt_lds_floats(n1, N) == 4 * (288 * n1 + 16) + ((N + 3) & ~3) + 512 * n1
        assert shim.gt_lds_floats(n1, N) * 4 <= 160 * 1024  # the gfx950 workgroup limit, without the blob
    text = open(os.path.join(os.path.dirname(SHIM), "..", "..", "lhotse_amd", "csrc", "kernel_grad.hpp")).read()
    assert "constexpr int grad_buf_floats(int N1) { return 288 * N1 + 16; }" in text
