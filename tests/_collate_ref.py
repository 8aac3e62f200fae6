"""The numpy statement of the collate launch (lhotse_amd/csrc/kernel_collate.hpp): what ``collate_audio`` (lhotse/dataset/collation.py:148-260)
does to samples that already lie in one arena.  Shared by the CPU and the GPU tests."""
import numpy as np
import torch

TORCH_OF = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def collate_ref(arena, offsets, lengths, row_len=None, dst_offsets=None, dtype=torch.float32) -> torch.Tensor:
    """Row ``i`` = zeros, with ``arena[offsets[i] : offsets[i] + lengths[i]]`` at ``dst_offsets[i]`` (None: 0); ``row_len`` None: the longest
    cut.  float32: the samples' bits; float16 / bfloat16: torch's CPU ``.to(dtype)`` (round to nearest even).  -> a CPU tensor (B, row_len)."""
    arena = np.asarray(arena.cpu().numpy() if isinstance(arena, torch.Tensor) else arena, dtype=np.float32)
    offsets, lengths = np.asarray(offsets, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    if row_len is None:
        row_len = int(lengths.max()) if len(lengths) else 0
    dst = np.zeros(len(offsets), dtype=np.int64) if dst_offsets is None else np.asarray(dst_offsets, dtype=np.int64)
    out = np.zeros((len(offsets), int(row_len)), dtype=np.float32)
    bits = out.view(np.uint32)  # (copied as bit patterns: a signalling NaN stays what it is)
    for i, (o, n, d) in enumerate(zip(offsets, lengths, dst)):
        assert 0 <= d and d + n <= row_len and 0 <= o and o + n <= len(arena)
        bits[i, d : d + n] = arena[o : o + n].view(np.uint32)
    return torch.from_numpy(out).to(dtype)


def bits_of(t: torch.Tensor) -> np.ndarray:
    """The raw bits of a float32 / float16 / bfloat16 tensor, as unsigned integers on the host."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint16)
