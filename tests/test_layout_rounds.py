"""CPU: the rounds per workgroup build_descs picks for a layout (lhotse_amd/csrc/layout_rounds.hpp, through the C shim
tests/native/layout_rounds_capi.cpp) against the Python restatement tests/_layout_rounds.py that the GPU tests of the fused Whisper
normalisation use to prove which sweep route their layout enters."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import _layout_rounds as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(tempfile.mkdtemp(prefix="rounds_"), "librounds.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "layout_rounds_capi.cpp"), "-o", out])
    L = ctypes.CDLL(out)
    L.layout_rounds_per_cut.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.layout_rounds_quads.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    return L


def native_per_cut(lib, frames, unit, rmax, bpc):
    a = np.ascontiguousarray(frames, dtype=np.int64)
    return lib.layout_rounds_per_cut(a.ctypes.data_as(ctypes.c_void_p), len(a), unit, rmax, bpc)


def random_batch(rs):
    """Uniform or ragged, 1 .. 3000 cuts (both sides of the sampling stride of batch / 512), frames from one quad to 30 s at a 10 ms hop."""
    pick = rs.randint(4)
    batch = [rs.randint(1, 9), rs.randint(1, 512), rs.randint(512, 1025), rs.randint(1, 3001)][pick]
    top = int(rs.choice([8, 100, 1000, 3000, 60000]))
    if rs.rand() < 0.4:
        frames = np.full(batch, rs.randint(1, top + 1), dtype=np.int64)
    else:
        frames = rs.randint(1, top + 1, size=batch).astype(np.int64)
    return frames


def test_restatement_agrees_with_the_header_on_random_batches(lib):
    rs = np.random.RandomState(2024)
    seen_r, strided, n = set(), 0, 0
    for unit in (32, 16, 8):
        for rmax in (16, 32, 64):
            for _ in range(250):  # 9 x 250 = 2250 batches
                frames = random_batch(rs)
                bpc = int(rs.randint(1, 5))
                want = native_per_cut(lib, frames, unit, rmax, bpc)
                got = R.rounds_per_cut(frames.tolist(), unit, rmax, bpc)
                assert got == want, (unit, rmax, bpc, len(frames), frames[:8])
                assert min(2, rmax) <= got <= rmax
                quads = int(((frames + 3) // 4).sum())
                assert R.rounds_quads(quads, unit, rmax, bpc) == lib.layout_rounds_quads(quads, unit, rmax, bpc), (quads, unit, rmax, bpc)
                seen_r.add(got)
                strided += len(frames) >= 1024
                n += 1
    assert n >= 2000 and strided >= 200 and len(seen_r) >= 10, (n, strided, sorted(seen_r))


@pytest.mark.parametrize("bpc", [1, 2, 3, 4])
def test_hand_cases(lib, bpc):
    # one small cut: one workgroup whatever the rounds, so the cheapest workgroup (r = 2) wins
    for frames in ([1], [64], [100], [300]):
        assert R.rounds_per_cut(frames, 32, 16, bpc) == 2 == native_per_cut(lib, frames, 32, 16, bpc), frames
    # 256 x blocks/CU cuts of 256 frames: r = 8 fills every slot with one whole cut; r < 8 needs ceil(8 / r) waves of cheaper workgroups
    # (r = 4: 2 x 4.64 > 8.64), r > 8 pays for rounds that hold no frames
    frames = [256] * (256 * bpc)
    assert R.rounds_per_cut(frames, 32, 16, bpc) == 8 == native_per_cut(lib, frames, 32, 16, bpc)
    assert R.workgroups_per_cut(frames, 32, 8) == 256 * bpc == R.slots(bpc)


def test_empty_batch_and_kernel_name(lib):
    assert R.rounds_per_cut([], 32, 16, 4) == 16 == native_per_cut(lib, np.zeros(0, dtype=np.int64), 32, 16, 4)  # cost 0 everywhere: the tie rule
    assert R.blocks_per_cu("whisper3_kernel<2> fft400=16x25 fused-norm lds=65536B blocks/CU=2 mel4=2x16") == 2
    assert R.whisper3_frames_per_workgroup([1100], "whisper3_kernel<2> fft400=16x25 fused-norm lds=1B blocks/CU=2 mel4=2x16") == 64
