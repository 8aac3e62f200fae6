"""Python restatement of lhotse_amd/csrc/layout_rounds.hpp: the rounds per workgroup that build_descs picks for a layout of a
wave-autonomous kernel.  The ABI does not say how many frames a workgroup of a layout holds; the GPU tests that must land on one
code path of the fused Whisper normalisation work it out from here (and assert it), tests/test_layout_rounds.py holds this file to
the header on the CPU.

frames per workgroup = fpb_unit x rounds; whisper3_kernel: fpb_unit = 8 waves x 4 frames = 32, rounds 2 .. 16."""
from __future__ import annotations

import re
from typing import Sequence

import numpy as np

STARTUP = 0.64       # kRoundsStartup
SAMPLED_CUTS = 512   # kRoundsSampledCuts
W3_FPB_UNIT = 32     # whisper3_kernel: kW3Waves x 4 frames
W3_ROUNDS_MAX = 16


def slots(blocks_per_cu: int) -> int:
    return 256 * max(int(blocks_per_cu), 1)


def _cost(nb: int, nslots: int, r: int) -> float:
    waves = nb / nslots if nb >= 8 * nslots else float((nb + nslots - 1) // nslots)
    return waves * (STARTUP + r)


def _argmin(rounds_max: int, nslots: int, workgroups) -> int:
    rounds, best = rounds_max, -1.0
    for r in range(min(2, rounds_max), rounds_max + 1):
        cost = _cost(workgroups(r), nslots, r)
        if best < 0.0 or cost <= best * (1.0 + 1e-9):  # ties go to the larger workgroup
            best, rounds = cost, r
    return rounds


def workgroups_per_cut(num_frames: Sequence[int], fpb_unit: int, rounds: int, step: int = 1) -> int:
    per = fpb_unit * rounds
    batch = len(num_frames)
    picked = np.asarray(num_frames, dtype=np.int64)[::step]
    nb = int(((picked + (per - 1)) // per).sum())
    return nb if step == 1 else (nb * batch + len(picked) // 2) // max(len(picked), 1)


def rounds_per_cut(num_frames: Sequence[int], fpb_unit: int, rounds_max: int, blocks_per_cu: int) -> int:
    """Layout by cuts: a cut's frames are not shared between workgroups."""
    stride = max(1, len(num_frames) // SAMPLED_CUTS)
    return _argmin(rounds_max, slots(blocks_per_cu), lambda r: workgroups_per_cut(num_frames, fpb_unit, r, stride))


def rounds_quads(quads: int, fpb_unit: int, rounds_max: int, blocks_per_cu: int) -> int:
    """Layout by frame quads (fft512c FLAT)."""
    w = fpb_unit // 4
    return _argmin(rounds_max, slots(blocks_per_cu), lambda r: (quads + w * r - 1) // (w * r))


def blocks_per_cu(kernel_name: str) -> int:
    """The occupancy a plan read for its kernel, from hipfeat_plan_kernel_name ("... blocks/CU=4 ...")."""
    m = re.search(r"blocks/CU=(\d+)", kernel_name)
    assert m, kernel_name
    return int(m.group(1))


def whisper3_frames_per_workgroup(num_frames: Sequence[int], kernel_name: str) -> int:
    assert kernel_name.startswith("whisper3_kernel"), kernel_name
    return W3_FPB_UNIT * rounds_per_cut(num_frames, W3_FPB_UNIT, W3_ROUNDS_MAX, blocks_per_cu(kernel_name))
