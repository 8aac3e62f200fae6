"""CPU: what the 16-byte feature store of fft512c_kernel (transposed 4 x 4 x 1 accumulators: lane = 4 slot + frame, register = filter
4g .. 4g + 3; fft_common.hpp::mel4_store_wide) takes for granted about the lane table of lhotse_amd/csrc/mel4_schedule.hpp, checked on the
very tables the plan uploads:

  * the reduction masks m4 / m8 are a property of the SLOT: equal on its four lanes, so the row_shr multiply-adds do the same on the
    transposed block as on the plain one;
  * a slot with an output holds the columns 4g + lane % 4 of ONE filter group, 4g a multiple of 4: quad lane 0 names the first of the
    four consecutive columns that a lane stores;
  * with a filter count that is a multiple of 4 a slot has four outputs or none, so ONE lane mask per slot covers the store.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from lhotse_amd import constants as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_COLUMN = 1 << 20  # kMel4NoColumn

# (prow_stride, [(max_sets, max_steps) in the order the plan tries them]) per kernel family
FFT512C = (272, [(2, 16), (1, 32)])  # kCPRowStride; kCMaxSets x kCMaxSteps, else 1 set of twice the steps (plan_tables.hpp::build_fft512c_tables)
FFT256C = (144, [(2, 8)])  # kDPRowStride, kDSets x kDSteps

# name, family, fft length, sampling rate: the 16 kHz default (25 ms), 32 ms frames at 16 kHz (the same 512-point filterbank: the frame
# length does not enter it), 8 kHz (256-point)
GEOMETRIES = [("16k", FFT512C, 512, 16000), ("16k_32ms", FFT512C, 512, 16000), ("8k", FFT256C, 256, 8000)]
FILTERS = (23, 40, 64, 80)


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(tempfile.mkdtemp(prefix="mel4w_"), "libmel4.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "mel4_schedule_capi.cpp"), "-o", out])
    return ctypes.CDLL(out)


def lane_table(lib, mel, prow_stride, shapes):
    """(nsets, 64 lanes, 4) lane table of the first schedule shape that takes the filterbank, None if none does"""
    K, M = mel.shape
    mel = np.ascontiguousarray(mel, dtype=np.float32)
    for max_sets, max_steps in shapes:
        nsets = ctypes.c_int(0)
        steps, step0 = (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
        wtab, ltab = np.zeros(64 * 64, dtype=np.float32), np.zeros(4 * 256, dtype=np.float32)
        n = lib.mel4_build(mel.ctypes.data_as(ctypes.c_void_p), M, K, prow_stride, max_sets, max_steps, ctypes.byref(nsets), steps, step0,
                           wtab.ctypes.data_as(ctypes.c_void_p), wtab.size, ltab.ctypes.data_as(ctypes.c_void_p), ltab.size)
        assert n >= 0, "table capacity"
        if n > 0:
            return ltab[: nsets.value * 256].reshape(nsets.value, 64, 4)
    return None


@pytest.mark.parametrize("M", FILTERS)
@pytest.mark.parametrize("name,family,fft,sr", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_every_slot_meets_what_the_wide_store_relies_on(lib, name, family, fft, sr, M):
    mel = np.asarray(C.make_kaldi_mel(M, fft, sr, 20.0, -400.0), dtype=np.float32)  # (fft / 2 + 1, M)
    ltab = lane_table(lib, mel, *family)
    if ltab is None:
        # outside the static schedule: the plan takes another kernel and nothing here applies.  The filter counts that the wide store serves
        # at the 16 kHz default must be inside.
        assert not (family is FFT512C), (name, M)
        return
    col = np.ascontiguousarray(ltab[:, :, 1]).view(np.int32).reshape(-1, 16, 4)  # [set][slot][quad lane]
    m4 = ltab[:, :, 2].reshape(-1, 16, 4)
    m8 = ltab[:, :, 3].reshape(-1, 16, 4)
    assert (m4 == m4[:, :, :1]).all() and (m8 == m8[:, :, :1]).all(), "m4 / m8 differ inside a slot"
    assert np.isin(m4, (0.0, 1.0)).all() and np.isin(m8, (0.0, 1.0)).all()
    seen = np.zeros(M, dtype=int)
    for s in range(col.shape[0]):
        for b in range(16):
            c = col[s, b]
            has = c < M
            assert ((c == NO_COLUMN) | has).all(), (s, b, c)
            if not has.any():
                continue
            g4 = int(c[has][0]) - int(np.flatnonzero(has)[0])  # the group's first column 4g
            assert g4 >= 0 and g4 % 4 == 0, (s, b, c)
            assert (c[has] == g4 + np.flatnonzero(has)).all(), (s, b, c)
            assert has[0] and c[0] == g4, "quad lane 0 must name the slot's first column"
            assert (has == (g4 + np.arange(4) < M)).all(), (s, b, c)  # only the columns past M are missing
            if M % 4 == 0:
                assert has.all(), (s, b, c)  # four outputs or none
            seen[c[has]] += 1
    assert (seen == 1).all(), "every filter is stored by exactly one lane"
