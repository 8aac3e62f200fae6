"""CPU: the host side of the matrix-core resampler (lhotse_amd/csrc/resample_tables.hpp) through the C shim
tests/native/resample_tables_capi.cpp, and ABI v8.

A  geometry (padded taps / phases, hop tiles, LDS floats, workgroups per cut) and the padded transposed bank against numpy, for
   441:160, 441:320, 441:640, 147:80 and 160:441 with the banks ``constants.sinc_resample_kernel`` computes for them;
B  the stand-alone program of the shim (its own main) walks the same header over more ratios;
C  header = ``_lib.ABI_VERSION`` = library = 8, ``hipfeat_resampler_kernel_name`` is declared, mirrored and exported, and the
   earlier exports are all still there."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from lhotse_amd import _lib, build
from lhotse_amd import constants as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "native", "resample_tables_capi.cpp")
HEADER = os.path.join(ROOT, "include", "hipfeat.h")
RATES = [(44100, 16000), (22050, 16000), (11025, 16000), (44100, 24000), (16000, 44100)]
REDUCED = [(441, 160), (441, 320), (441, 640), (147, 80), (160, 441)]
LDS_BUDGET = 65536


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(tempfile.mkdtemp(prefix="restab_"), "librestab.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SHIM, "-o", out])
    lib = ctypes.CDLL(out)
    lib.rt_blocks.restype = ctypes.c_longlong
    lib.rt_blocks.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
    return lib


def geometry(lib, orig, nw, width):
    out = np.zeros(10, dtype=np.int64)
    lib.rt_geometry(orig, nw, width, out.ctypes.data_as(ctypes.c_void_p))
    names = ["kw", "kwp", "nwp", "hop_tiles", "hops_per_block", "outs_per_block", "span_floats", "lds_bytes", "fits", "routed"]
    return dict(zip(names, out.tolist()))


def expected_geometry(orig, nw, width):
    kw = 2 * width + orig
    kwp, nwp = -(-kw // 16) * 16, -(-nw // 16) * 16
    for ht in (4, 2, 1):
        span = ((16 * ht - 1) * orig + kwp + 3) & ~3
        if 4 * span <= LDS_BUDGET:
            return dict(kw=kw, kwp=kwp, nwp=nwp, hop_tiles=ht, hops_per_block=16 * ht, outs_per_block=16 * ht * nw, span_floats=span,
                        lds_bytes=4 * span, fits=1, routed=int(nw >= 16 and orig % 2 == 1))
    return None


@pytest.mark.parametrize("rates,reduced", list(zip(RATES, REDUCED)), ids=["%d:%d" % r for r in REDUCED])
def test_geometry_and_padded_bank_against_numpy(lib, rates, reduced):
    kernel, width, orig, nw = C.sinc_resample_kernel(*rates)
    assert (orig, nw) == reduced and kernel.shape == (nw, 2 * width + orig) and kernel.dtype == np.float32
    g = geometry(lib, orig, nw, width)
    assert g == expected_geometry(orig, nw, width)
    # what the kernel's bounds rest on: the last float a lane reads (row hops_per_block - 1, tap kwp - 1) lies inside the staged span
    assert (g["hops_per_block"] - 1) * orig + g["kwp"] - 1 < g["span_floats"]
    # the routing rule without a measurement: many phases and an odd hop
    assert g["routed"] == (0 if reduced == (160, 441) else 1)
    kt = np.full((g["kwp"], g["nwp"]), np.nan, dtype=np.float32)
    lib.rt_bank(kernel.ctypes.data_as(ctypes.c_void_p), nw, g["kw"], g["kwp"], g["nwp"], kt.ctypes.data_as(ctypes.c_void_p))
    want = np.zeros((g["kwp"], g["nwp"]), dtype=np.float32)
    want[: g["kw"], :nw] = kernel.T
    assert np.array_equal(kt.view(np.uint32), want.view(np.uint32))  # bit for bit, zeros are +0
    for hops in (0, 1, g["hops_per_block"] - 1, g["hops_per_block"], g["hops_per_block"] + 1, 1000):
        for out_len in {max(hops * nw - 1, 0), hops * nw, hops * nw + 1}:
            assert lib.rt_blocks(orig, nw, width, out_len) == -(-(-(-out_len // nw)) // g["hops_per_block"]), (hops, out_len)


def test_hop_tiles_follow_the_lds_budget_and_small_ratios_are_not_routed(lib):
    assert geometry(lib, 441, 160, 17)["hop_tiles"] == 2 and geometry(lib, 147, 80, 12)["hop_tiles"] == 4
    assert geometry(lib, 1021, 16, 6)["hop_tiles"] == 1
    g = geometry(lib, 20001, 16, 7)  # one tile of 16 hops does not fit: left to the generic kernel's own size check
    assert g["fits"] == 0 and g["routed"] == 0 and lib.rt_blocks(20001, 16, 7, 1000) == 0
    assert geometry(lib, 9, 10, 7)["routed"] == 0  # fewer than 16 phases
    assert geometry(lib, 3, 16, 7)["routed"] == 1 and geometry(lib, 2, 16, 7)["routed"] == 0


def test_gpu_ratios_reach_every_instance_and_every_path_of_the_kernel(lib):
    """What the list of tests/_resample_rates.py is for: over the ratios tests/test_gpu_resample_mfma.py runs, `res_mfma_geometry` yields
    every hop-tile instance of resample_mfma_kernel (the dispatch of hipfeat_resample), an even and an odd number of trips of the tap loop
    (its two register sets take turns: behind an odd count the last fetched set is not used), and fewer, as many and more phase tiles
    than a workgroup has waves (waves without work; waves with a second tile); one ratio's last tile is partly filled."""
    import _resample_rates as RATES

    assert len(set(RATES.ALL)) == len(RATES.ALL) == len(RATES.ROUTED) + 1 + len(RATES.EXTRA)
    geo = {}
    for rates in RATES.ALL:
        _, width, orig, nw = C.sinc_resample_kernel(*rates)
        g = geometry(lib, orig, nw, width)
        assert g["fits"] == 1 and nw >= 16  # (what HIPFEAT_RESAMPLE_MFMA=1 needs to put a ratio on the kernel)
        assert g["routed"] == (0 if rates in (RATES.EVEN_HOP, RATES.ONE_HOP_TILE) else 1)
        geo[rates] = dict(g, orig=orig, nw=nw, trips=g["kwp"] // 16, tiles=g["nwp"] // 16)
    assert {g["hop_tiles"] for g in geo.values()} == {1, 2, 4}
    assert {g["trips"] % 2 for g in geo.values()} == {0, 1}
    tiles = {g["tiles"] for g in geo.values()}
    assert min(tiles) < 4 and 4 in tiles and max(tiles) > 4
    assert any(g["nw"] % 16 for g in geo.values()) and any(g["nw"] % 16 == 0 for g in geo.values())
    one = geo[RATES.ONE_HOP_TILE]
    assert (one["orig"], one["nw"], one["kw"], one["kwp"], one["trips"], one["tiles"], one["hop_tiles"]) == (640, 441, 658, 672, 42, 28, 1)
    assert (geo[RATES.ONE_PHASE_TILE]["orig"], geo[RATES.ONE_PHASE_TILE]["nw"], geo[RATES.ONE_PHASE_TILE]["tiles"]) == (49, 16, 1)
    assert (geo[RATES.FOUR_PHASE_TILES]["orig"], geo[RATES.FOUR_PHASE_TILES]["nw"], geo[RATES.FOUR_PHASE_TILES]["tiles"]) == (147, 64, 4)


def test_stand_alone_program_of_the_shim(tmp_path):
    exe = str(tmp_path / "restab")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DRESAMPLE_TABLES_MAIN", SHIM, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr


def test_abi_v8_and_the_kernel_name_export():
    text = open(HEADER).read()
    header = int(re.search(r"#define\s+HIPFEAT_ABI_VERSION\s+(\d+)", text).group(1))
    assert header == _lib.ABI_VERSION == _lib.load().raw("hipfeat_abi_version") == 8
    name = "hipfeat_resampler_kernel_name"
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"HIPFEAT_API\s+const char\*\s+%s\s*\(\s*const hipfeat_resampler\*\s+\w+\s*\)\s*;" % name, plain)
    assert _lib._SIGNATURES[name] == ("const char*", ["const hipfeat_resampler*"])
    out = subprocess.run(["nm", "-D", "--defined-only", str(build.build())], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hipfeat_\w+)", out))
    assert name in exported
    assert len(_lib._SIGNATURES) == 52 and set(_lib._SIGNATURES) <= exported  # the 51 exports of ABI v7 and this one
    assert _lib.load().string(name, 0) == ""  # NULL handle: no device is touched
    assert "lhotse/augmentation/resample.py:284-315" in text[text.index("ABI v8") : text.index(name)]
