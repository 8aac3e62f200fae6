"""The numpy statement of the sources form of the collate launch (lhotse_amd/csrc/kernel_collate.hpp, ``collate_mean_kernel``): what
``collate_audio`` (lhotse/dataset/collation.py:215-241) does to the channels of multi-channel cuts that already lie in one arena.  Shared by
the CPU and the GPU tests.

Row ``r`` has ``k = first[r + 1] - first[r]`` sources of ``lengths[r]`` samples: ``k = 0`` -- zeros; ``k = 1`` -- the samples' bits;
``k >= 2`` -- an explicit loop over the sources in float64 from +0.0 in ascending order, ONE float64 division by ``k``, ONE cast to float32
(round to nearest even); then ``collate_ref``'s conversion to the output type (torch's CPU ``.to(dtype)``)."""
import numpy as np
import torch


def downmix_ref(channels) -> np.ndarray:
    """``(C, T)`` float32 (or a list of C rows) -> the ``(T,)`` float32 mean over the channels as the device states it."""
    rows = [np.asarray(x, dtype=np.float32) for x in channels]
    if len(rows) == 1:
        return rows[0].copy()
    acc = np.zeros(rows[0].shape, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for x in rows:  # ascending source order
            acc = acc + x.astype(np.float64)
        return (acc / np.float64(len(rows))).astype(np.float32)


def collate_sources_ref(arena, first, src_offsets, lengths, row_len=None, dst_offsets=None, dtype=torch.float32) -> torch.Tensor:
    """-> a CPU tensor (rows, row_len) of ``dtype``; ``row_len`` None: the longest row; ``dst_offsets`` None: 0."""
    arena = np.asarray(arena.cpu().numpy() if isinstance(arena, torch.Tensor) else arena, dtype=np.float32)
    first, src, lengths = (np.asarray(a, dtype=np.int64) for a in (first, src_offsets, lengths))
    assert len(first) == len(lengths) + 1 and first[0] == 0 and first[-1] == len(src)
    if row_len is None:
        row_len = int(lengths.max()) if len(lengths) else 0
    dst = np.zeros(len(lengths), dtype=np.int64) if dst_offsets is None else np.asarray(dst_offsets, dtype=np.int64)
    out = np.zeros((len(lengths), int(row_len)), dtype=np.float32)
    bits = out.view(np.uint32)  # (copied as bit patterns: a signalling NaN of a k = 1 row stays what it is)
    for r, (n, d) in enumerate(zip(lengths, dst)):
        offs = src[first[r] : first[r + 1]]
        assert 0 <= d and d + n <= row_len and all(0 <= o and o + n <= len(arena) for o in offs if n > 0)
        if len(offs) == 0 or n == 0:
            continue
        bits[r, d : d + n] = downmix_ref([arena[o : o + n] for o in offs]).view(np.uint32)
    return torch.from_numpy(out).to(dtype)


def ulp32(t) -> np.ndarray:
    """The spacing of float32 at the float64 values ``t`` (2^-149 at and below the subnormals)."""
    _, e = np.frexp(np.abs(np.asarray(t, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e - 24, -149))
