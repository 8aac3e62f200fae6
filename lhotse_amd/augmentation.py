"""
GPU speed perturbation / sinc resampling behind lhotse's ``AudioTransform`` interface
("next" row 1).

Mirrors lhotse/augmentation/torchaudio.py:26-140 (``Speed``, ``Resample``, ``get_or_create_resampler``) and
lhotse/augmentation/resample.py:42-142 (``Resample`` module, here ``HipResampleTensor``): same names, arguments,
output lengths and dict round trip; the arithmetic -- zero pad, strided polyphase FIR, trim -- runs in
``resample_kernel`` (lhotse_amd/csrc/kernel_resample.hpp) through the C ABI (``hipfeat_resample``).

    fn = HipSpeed(factor=1.1)                      # AudioTransform: numpy (C, T) -> numpy (C, T')
    wave = fn(samples, 16000)
    OnTheFlyFeatures(HipFbank(), wave_transforms=[...])      # unchanged; or, staying on the device:
    ys = get_or_create_resampler(17600, 16000)(x_cuda)       # torch (..., T) -> (..., T') on the same device

There is no CPU fallback: without a HIP device the call raises ``HipFeatError``.
"""
from __future__ import annotations

import threading
from dataclasses import asdict, dataclass
from decimal import ROUND_HALF_DOWN, ROUND_HALF_UP, Decimal
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, constants
from .compat import HAVE_LHOTSE, Seconds

if HAVE_LHOTSE:  # pragma: no cover - authoring container only
    from lhotse.augmentation.transform import AudioTransform  # type: ignore
else:

    class AudioTransform:  # stand-in with the same surface (lhotse/augmentation/transform.py:9-76)
        KNOWN_TRANSFORMS: Dict[str, type] = {}

        def __init_subclass__(cls, **kwargs):
            AudioTransform.KNOWN_TRANSFORMS.setdefault(cls.__name__, cls)
            super().__init_subclass__(**kwargs)

        def to_dict(self) -> dict:
            return {"name": type(self).__name__, "kwargs": asdict(self)}

        @staticmethod
        def from_dict(data: dict) -> "AudioTransform":
            assert data["name"] in AudioTransform.KNOWN_TRANSFORMS, f"Unknown transform type: {data['name']}"
            return AudioTransform.KNOWN_TRANSFORMS[data["name"]](**data["kwargs"])


def perturb_num_samples(num_samples: int, factor: float) -> int:
    """Number of samples after speed perturbation (lhotse/utils.py:649-654)."""
    rounding = ROUND_HALF_UP if factor >= 1.0 else ROUND_HALF_DOWN
    return int(Decimal(round(num_samples / factor, ndigits=8)).quantize(0, rounding=rounding))


def _compute_num_samples(duration: Seconds, sampling_rate: int) -> int:
    """lhotse/utils.py:657-673"""
    return int(Decimal(round(duration * sampling_rate, ndigits=8)).quantize(0, rounding=ROUND_HALF_UP))


MAX_RESAMPLE_BANK_FLOATS = 1 << 20  # the largest dense filter bank (new x (2 width + orig) floats, reduced rates) that is built and uploaded
SINC_MAX_WINDOW = 96  # kSincMaxW of csrc/sinc_tables.hpp: the widest window (2 width + 2 taps per phase) the bankless kernel holds


def _sinc_geometry(source_rate: int, target_rate: int) -> Tuple[int, int, int]:
    """(orig, new, width) of the reference's filter for source -> target (lhotse/augmentation/resample.py:219-239: rates reduced by their
    gcd, lowpass_filter_width 6, rolloff 0.99), from the rates alone."""
    from math import ceil, gcd

    g = gcd(int(source_rate), int(target_rate))
    orig, new = int(source_rate) // g, int(target_rate) // g
    return orig, new, ceil(6 * orig / (min(orig, new) * 0.99))


def _sinc_bank_floats(source_rate: int, target_rate: int) -> int:
    """Floats of the reference's dense filter bank for source -> target, from the rates alone."""
    orig, new, width = _sinc_geometry(source_rate, target_rate)
    return new * (2 * width + orig)


def _dense_kernel_fits(orig: int, new: int, width: int) -> bool:
    """The support rule of ``hipfeat_resampler_create`` for a bank it is given (csrc/hipfeat.hip): the generic kernel stages the input span
    of at least 64 outputs -- ``(ceil(64 / new) + 1) * orig + 2 * width + orig`` floats, rounded up to 4 -- in LDS, next to the bank when
    that has at most 8192 floats, and has 64 KiB."""
    kw = 2 * width + orig
    span = ((-(-64 // new) + 1) * orig + kw + 3) & ~3
    return 4 * (span + (new * kw if new * kw <= 8192 else 0)) <= 64 * 1024


def resample_route(source_rate: int, target_rate: int) -> Optional[str]:
    """THE routing rule of a rate pair: ``"bank"`` -- its dense bank has at most ``MAX_RESAMPLE_BANK_FLOATS`` floats and the dense kernels
    take it (``_dense_kernel_fits``): a cached ``HipResampleTensor`` with the bank in HBM (``hipfeat_resample``) --, ``"sinc"`` -- the
    bankless kernel (``hipfeat_sinc_run``): a window of at most ``SINC_MAX_WINDOW`` taps, reduced rates up to 2^24 --, or None: no kernel
    serves it (16000 -> 2001: a bank of 32 M floats and a window of 100 taps; 16000 -> 202: a bank of 905 K floats whose hop of 8000
    samples does not fit the dense kernel's LDS, and a window of 954 taps)."""
    if int(source_rate) <= 0 or int(target_rate) <= 0 or int(source_rate) == int(target_rate):
        return None
    orig, new, width = _sinc_geometry(source_rate, target_rate)
    if new * (2 * width + orig) <= MAX_RESAMPLE_BANK_FLOATS and _dense_kernel_fits(orig, new, width):
        return "bank"
    return "sinc" if 2 * width + 2 <= SINC_MAX_WINDOW and max(orig, new) <= 1 << 24 else None


class HipResampleTensor:
    """Device counterpart of the ``Resample`` nn.Module (lhotse/augmentation/resample.py:42-142): the filter
    bank lives in HBM; calling it resamples every row of a ``(..., T)`` float32 tensor.  A rate pair whose dense bank would exceed
    ``MAX_RESAMPLE_BANK_FLOATS`` (11127 -> 16000: 178 M floats) builds no bank: it runs the bankless kernel (``HipSincResampler``),
    ``kernel_name == "resample_sinc"``, ``kernel is None``."""

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                 device: Union[str, torch.device, None] = None):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.lowpass_filter_width, self.rolloff = lowpass_filter_width, rolloff
        self.bankless = (lowpass_filter_width, rolloff) == (6, 0.99) and self.orig_freq != self.new_freq and min(self.orig_freq, self.new_freq) > 0 \
            and (_sinc_bank_floats(orig_freq, new_freq) > MAX_RESAMPLE_BANK_FLOATS or resample_route(orig_freq, new_freq) == "sinc")
        if self.bankless:
            self.kernel = None
            self.orig, self.new, self.width = _sinc_geometry(orig_freq, new_freq)
        else:
            self.kernel, self.width, self.orig, self.new = constants.sinc_resample_kernel(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self.lib = _lib.load()
        self.handle = 0
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise _lib.HipFeatError(1, f"HipResampleTensor runs on an AMD GPU ('cuda[:i]' device), got device={dev}")
        if not torch.cuda.is_available():
            raise _lib.HipFeatError(2, "no HIP device is visible (torch.cuda.is_available() is False); there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        if self.bankless:
            if resample_route(orig_freq, new_freq) != "sinc":
                raise _lib.HipFeatError(_lib.ERR_UNSUPPORTED, f"{orig_freq} -> {new_freq}: a window of {2 * self.width + 2} taps per phase, the bankless "
                                                              f"kernel holds {SINC_MAX_WINDOW}")
            self.sinc = get_or_create_sinc(self.device)
            self.kernel_name = "resample_sinc"
            return
        out = np.zeros(1, dtype=np.uint64)
        self.lib.check("hipfeat_resampler_create", self.orig, self.new, self.width, _lib.addr(self.kernel), int(self.device.index), _lib.addr(out))
        self.handle = int(out[0])
        # "resample_fast<9,10,7>" | "resample_mfma" | "resample_generic": the kernel the library chose for this ratio
        self.kernel_name = self.lib.string("hipfeat_resampler_kernel_name", self.handle)

    # ---- lengths -------------------------------------------------------------------------------------------
    def output_length(self, num_samples: int) -> int:
        if self.orig == self.new:
            return int(num_samples)
        return int(self.lib.raw("hipfeat_resampled_length", int(num_samples), self.orig, self.new))

    def output_lengths(self, num_samples: np.ndarray) -> np.ndarray:
        """Vectorised ``output_length`` (same float32 rounding, resample.py:309)."""
        n = _lib.i64(num_samples)
        if self.orig == self.new:
            return n
        return np.ceil((self.new * n / self.orig).astype(np.float32)).astype(np.int64)

    # ---- packed ragged batch, device resident ---------------------------------------------------------------
    def run(self, wave: torch.Tensor, offsets: np.ndarray, lengths: np.ndarray, align: bool = True) -> Tuple[torch.Tensor, np.ndarray, np.ndarray]:
        """wave: contiguous float32 on self.device holding every cut; -> (output buffer, out_offsets, out_lengths).
        With ``align`` every output cut starts on a 16-byte boundary (up to 3 floats of slack between cuts), which is
        what lets the feature kernels take their LDS-DMA load path on the result; otherwise cuts are back to back."""
        assert wave.dtype == torch.float32 and wave.is_contiguous() and wave.device == self.device
        offsets, lengths = _lib.i64(offsets), _lib.i64(lengths)
        out_lens = self.output_lengths(lengths)
        out_offs = np.zeros(len(lengths), dtype=np.int64)
        step = ((out_lens + 3) & ~3) if align else out_lens
        np.cumsum(step[:-1], out=out_offs[1:])
        total = int(out_offs[-1] + out_lens[-1]) if len(lengths) else 0
        if self.bankless:  # one arena: a copy of the input in front, the outputs behind it
            front = (wave.numel() + 3) & ~3
            with torch.cuda.device(self.device):
                arena = torch.empty(front + total, dtype=torch.float32, device=self.device)
                arena[: wave.numel()].copy_(wave)
                ticket, planned, _ = self.sinc.plan(offsets, lengths, [(self.orig_freq, self.new_freq)] * len(lengths), out_offs + front, arena.numel())
                assert np.array_equal(planned, out_lens)  # the library's own length rule
                self.sinc.run(ticket, arena)
            return arena[front:], out_offs, out_lens
        with torch.cuda.device(self.device):
            out = torch.empty(total, dtype=torch.float32, device=self.device)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self.lib.check("hipfeat_resample", self.handle, wave.data_ptr(), _lib.addr(offsets), _lib.addr(lengths), int(len(lengths)),
                           out.data_ptr(), _lib.addr(out_offs), int(stream))
        return out, out_offs, out_lens

    def resample_batch(self, waves: Sequence[Union[np.ndarray, torch.Tensor]]) -> List[torch.Tensor]:
        """Ragged batch of 1-D waveforms (host or device) -> list of resampled device tensors (one launch)."""
        ts = [torch.as_tensor(w).reshape(-1) for w in waves]
        for t in ts:
            if t.dtype != torch.float32:
                raise TypeError(f"expected float32 samples, got {t.dtype}")
        if not ts:
            return []
        from .extractors import pack_to_device  # pinned staging + one H2D for host inputs

        wave, offsets, lengths = pack_to_device(ts, self.device)
        if self.orig == self.new:
            return [wave[o : o + n] for o, n in zip(offsets.tolist(), lengths.tolist())]
        out, out_offs, out_lens = self.run(wave, offsets, lengths)
        return [out[o : o + n] for o, n in zip(out_offs.tolist(), out_lens.tolist())]

    def __call__(self, waveform: torch.Tensor) -> torch.Tensor:
        """(..., T) -> (..., T'), result on the input's device (resample.py:126-142)."""
        if not isinstance(waveform, torch.Tensor):
            raise TypeError("expected a torch.Tensor")
        if self.orig_freq == self.new_freq:
            return waveform
        if waveform.dtype != torch.float32:
            raise TypeError(f"expected float32 samples, got {waveform.dtype}")
        shape = waveform.shape
        T = int(shape[-1])
        rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
        x = waveform.reshape(rows, T).to(self.device).contiguous()
        out, _, out_lens = self.run(x.view(-1), np.arange(rows, dtype=np.int64) * T, np.full(rows, T, dtype=np.int64), align=False)
        y = out.view(shape[:-1] + (int(out_lens[0]) if rows else 0,))
        return y.to(waveform.device)  # the input's device, whichever GPU (or the host) that is

    forward = __call__

    def close(self):
        if self.handle:
            try:
                self.lib.raw("hipfeat_resampler_destroy", self.handle)
            finally:
                self.handle = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_precompiled_resamplers: Dict[Tuple[int, int, int], HipResampleTensor] = {}
_cache_lock = threading.Lock()


def get_or_create_resampler(source_sampling_rate: int, target_sampling_rate: int, device: Union[str, torch.device, None] = None) -> HipResampleTensor:
    """lhotse/augmentation/torchaudio.py:72-83, keyed per device as well."""
    dev = torch.device("cuda" if device is None else device)
    index = dev.index if dev.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)
    key = (int(source_sampling_rate), int(target_sampling_rate), int(index))
    with _cache_lock:
        r = _precompiled_resamplers.get(key)
        if r is None:
            r = _precompiled_resamplers[key] = HipResampleTensor(key[0], key[1], device=torch.device(dev.type, index))
        return r


@dataclass
class HipSpeed(AudioTransform):
    """Speed perturbation (``sox speed``): resample from round(sr * factor) back to sr on the GPU.
    Drop-in for ``lhotse.augmentation.Speed`` (torchaudio.py:26-68)."""

    factor: float
    device: str = "cuda"

    def __call__(self, samples: Union[np.ndarray, torch.Tensor], sampling_rate: int) -> Union[np.ndarray, torch.Tensor]:
        resampler = get_or_create_resampler(round(sampling_rate * self.factor), sampling_rate, self.device)
        if isinstance(samples, torch.Tensor):  # device-resident use: stays a tensor on its device
            return resampler(samples)
        return resampler(torch.from_numpy(np.ascontiguousarray(samples))).numpy()

    def reverse_timestamps(self, offset: Seconds, duration: Optional[Seconds], sampling_rate: int) -> Tuple[Seconds, Optional[Seconds]]:
        """Offset/duration of the original audio that yields the requested perturbed span (torchaudio.py:44-68)."""
        start_sample = perturb_num_samples(_compute_num_samples(offset, sampling_rate), 1 / self.factor)
        num_samples = None if duration is None else perturb_num_samples(_compute_num_samples(duration, sampling_rate), 1 / self.factor)
        return start_sample / sampling_rate, None if num_samples is None else num_samples / sampling_rate


@dataclass
class HipResample(AudioTransform):
    """Sampling-rate conversion (``sox rate``) on the GPU; drop-in for ``lhotse.augmentation.Resample``
    (torchaudio.py:86-164) with the sinc backend."""

    source_sampling_rate: int
    target_sampling_rate: int
    device: str = "cuda"

    def __post_init__(self):
        self.source_sampling_rate = int(self.source_sampling_rate)
        self.target_sampling_rate = int(self.target_sampling_rate)

    @property
    def resampler(self) -> HipResampleTensor:
        return get_or_create_resampler(self.source_sampling_rate, self.target_sampling_rate, self.device)

    def __call__(self, samples: Union[np.ndarray, torch.Tensor], *args, **kwargs) -> Union[np.ndarray, torch.Tensor]:
        if self.source_sampling_rate == self.target_sampling_rate:
            return samples
        if isinstance(samples, torch.Tensor):
            return self.resampler(samples)
        return self.resampler(torch.from_numpy(np.ascontiguousarray(samples))).numpy()

    def reverse_timestamps(self, offset: Seconds, duration: Optional[Seconds], sampling_rate: int) -> Tuple[Seconds, Optional[Seconds]]:
        """Timestamps do not change with the sampling rate (torchaudio.py:142-164): whole-sample snapping only."""
        if self.source_sampling_rate == self.target_sampling_rate:
            return offset, duration
        old_offset = _compute_num_samples(offset, self.source_sampling_rate) / self.source_sampling_rate
        old_duration = None if duration is None else _compute_num_samples(duration, self.source_sampling_rate) / self.source_sampling_rate
        return old_offset, old_duration


# ---- speed perturbation of a packed mini-batch, in place of the host loop of config 5 -------------------------------------------
def perturbed_tail_floats(lengths: np.ndarray, factors: Sequence[float], sampling_rate: int) -> int:
    """Floats the resampled cuts of a mini-batch need behind its inputs (every resampled cut starts on a 16-byte boundary)."""
    total = 0
    for f in sorted(set(float(x) for x in factors)):
        if f == 1.0:
            continue
        idx = np.nonzero(np.asarray(factors, dtype=np.float64) == f)[0]
        orig, new = constants.sinc_resample_kernel(round(sampling_rate * f), sampling_rate)[2:4]
        out = np.ceil((new * _lib.i64(lengths)[idx] / orig).astype(np.float32)).astype(np.int64)
        total += int(((out + 3) & ~3).sum())
    return total


def _grouped_layout(offsets, lengths, keys, ratio_of, tail_start):
    """The placement rule behind ``resample_layout`` and ``perturbed_layout``: cuts whose key is None stay, the others go behind
    ``tail_start`` group by group in ascending order of their keys, every resampled cut on a 16-byte boundary, ``ceil(new * n / orig)``
    samples in float32 (resample.py:309) with orig : new = ``ratio_of(key)`` reduced by their gcd (resample.py:219-222).
    -> (offsets, lengths, first free float behind the resampled cuts, 16-byte aligned, [(key, indices of its cuts)])."""
    from math import gcd

    offsets, lengths = _lib.i64(offsets).copy(), _lib.i64(lengths).copy()
    assert len(keys) == len(lengths)
    tail = (int(tail_start) + 3) & ~3
    groups = []
    for key in sorted(set(k for k in keys if k is not None)):
        idx = np.array([i for i, k in enumerate(keys) if k == key], dtype=np.int64)
        src, dst = (int(v) for v in ratio_of(key))
        g = gcd(src, dst)
        out_lens = np.ceil(((dst // g) * lengths[idx] / (src // g)).astype(np.float32)).astype(np.int64)
        out_offs = np.zeros(len(idx), dtype=np.int64)
        np.cumsum(((out_lens + 3) & ~3)[:-1], out=out_offs[1:])
        out_offs += tail
        offsets[idx], lengths[idx] = out_offs, out_lens
        tail = (int(out_offs[-1] + out_lens[-1]) + 3) & ~3
        groups.append((key, idx))
    return offsets, lengths, tail, groups


def _resample_groups_in_arena(arena, in_offsets, in_lengths, offsets, lengths, groups, ratio_of, what):
    """One ``hipfeat_resample`` launch per group of ``_grouped_layout`` whose ratio has a dense bank (``resample_route``), ONE
    ``hipfeat_sinc_run`` for all the others (what no kernel serves: the plan refuses it by name); input and output in the same arena."""
    assert arena.dtype == torch.float32 and arena.is_contiguous() and arena.ndim == 1
    last = max((int((offsets[idx] + lengths[idx]).max()) for _, idx in groups), default=0)
    if last > arena.numel():
        raise ValueError(f"arena too small: {arena.numel()} floats, the {what} cuts need {last} (see {what}_tail_floats)")
    dev = arena.device
    # a ratio without a dense bank (Speed(1.037) at 16 kHz is 1037 : 1000, a bank of 1.05 M floats) goes, with all its like, into ONE
    # launch of the bankless kernel; the placement is the same
    bankless = [(tuple(int(v) for v in ratio_of(key)), idx) for key, idx in groups if resample_route(*ratio_of(key)) != "bank"]
    _sinc_groups_in_arena(arena, in_offsets, in_lengths, offsets, lengths, bankless)
    for key, idx in groups:
        src, dst = (int(v) for v in ratio_of(key))
        if resample_route(src, dst) != "bank":
            continue
        r = get_or_create_resampler(src, dst, dev)
        in_offs, in_lens = np.ascontiguousarray(in_offsets[idx]), np.ascontiguousarray(in_lengths[idx])  # (named: they must outlive the call)
        out_offs = np.ascontiguousarray(offsets[idx])
        assert np.array_equal(r.output_lengths(in_lens), lengths[idx])  # the library's own length rule
        with torch.cuda.device(dev):
            r.lib.check("hipfeat_resample", r.handle, arena.data_ptr(), _lib.addr(in_offs), _lib.addr(in_lens), int(len(idx)), arena.data_ptr(),
                        _lib.addr(out_offs), int(torch.cuda.current_stream(dev).cuda_stream))


def _ratio_keys(ratios) -> list:
    return [None if r is None else (int(r[0]), int(r[1])) for r in ratios]


def resampled_tail_floats(lengths: np.ndarray, ratios: Sequence[Optional[Tuple[int, int]]]) -> int:
    """Floats the resampled cuts of ``resample_in_arena`` need behind ``tail_start`` (rounded up to 16 bytes)."""
    return int(_grouped_layout(np.zeros(len(lengths), dtype=np.int64), lengths, _ratio_keys(ratios), lambda k: k, 0)[2])


def resample_layout(offsets: np.ndarray, lengths: np.ndarray, ratios: Sequence[Optional[Tuple[int, int]]],
                    tail_start: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """Where ``resample_in_arena`` puts every cut and how long it comes out -- host arithmetic only.  ``ratios[i]`` = (source rate,
    target rate) of cut i, or None for a cut that stays as it is.  Cuts go behind ``tail_start`` ratio by ratio in ascending order of
    (source, target), every resampled cut on a 16-byte boundary, ``ceil(new * n / orig)`` samples in float32 (resample.py:309) with
    orig : new the rates reduced by their gcd (resample.py:219-222).  ``perturbed_layout`` is this rule with the ratios of ``Speed``.
    -> (offsets, lengths, first free float behind the resampled cuts, 16-byte aligned)."""
    return _grouped_layout(offsets, lengths, _ratio_keys(ratios), lambda k: k, tail_start)[:3]


def resample_in_arena(arena: torch.Tensor, offsets: np.ndarray, lengths: np.ndarray, ratios: Sequence[Optional[Tuple[int, int]]],
                      tail_start: int) -> Tuple[np.ndarray, np.ndarray]:
    """Sampling-rate conversion of a device-resident packed mini-batch (``Resample``, lhotse/augmentation/torchaudio.py:86-139 with the
    sinc backend): the generalisation of ``perturb_speed_in_arena`` from speed factors to any (source, target) rates per cut.

    ``arena`` is ONE float32 device buffer: the cuts at ``offsets`` / ``lengths`` in its front part, free space from ``tail_start`` on
    (``resampled_tail_floats`` says how much).  Cuts with ratio None stay where they are; the others are resampled into the tail.  This
    is the ROUTER (``resample_route``): ratios whose dense bank has at most ``MAX_RESAMPLE_BANK_FLOATS`` floats go to their cached
    ``HipResampleTensor`` -- one ``hipfeat_resample`` launch per distinct ratio, in ascending order --, all the others together into ONE
    ``hipfeat_sinc_run`` (``sinc_in_arena``); the placement (``resample_layout``) does not depend on the route.  Returns the per-cut
    (offsets, lengths) inside the same arena.  A second pass (a ``Speed`` behind the ``Resample``) takes these as its input with
    ``tail_start`` = the end ``resample_layout`` reports."""
    keys = _ratio_keys(ratios)
    in_offsets, in_lengths = _lib.i64(offsets), _lib.i64(lengths)
    offsets, lengths, _, groups = _grouped_layout(in_offsets, in_lengths, keys, lambda k: k, tail_start)
    _resample_groups_in_arena(arena, in_offsets, in_lengths, offsets, lengths, groups, lambda k: k, "resampled")  # (routes group by group)
    return offsets, lengths


def _check_arena(arena, offsets, lengths, groups, what):
    assert arena.dtype == torch.float32 and arena.is_contiguous() and arena.ndim == 1
    last = max((int((offsets[idx] + lengths[idx]).max()) for _, idx in groups), default=0)
    if last > arena.numel():
        raise ValueError(f"arena too small: {arena.numel()} floats, the {what} cuts need {last} (see {what}_tail_floats)")


def _sinc_groups_in_arena(arena, in_offsets, in_lengths, offsets, lengths, groups):
    """ONE ``hipfeat_sinc_run`` for the cuts of all ``groups`` of ``_grouped_layout``, input and output in the same arena."""
    if not groups:
        return
    idx = np.concatenate([i for _, i in groups])
    rates = [key for key, i in groups for _ in range(len(i))]
    sinc = get_or_create_sinc(arena.device)
    ticket, out_lens, _ = sinc.plan(in_offsets[idx], in_lengths[idx], rates, offsets[idx], arena.numel())
    assert np.array_equal(out_lens, lengths[idx])  # the library's own length rule
    sinc.run(ticket, arena)


def sinc_in_arena(arena: torch.Tensor, offsets: np.ndarray, lengths: np.ndarray, ratios: Sequence[Optional[Tuple[int, int]]],
                  tail_start: int) -> Tuple[np.ndarray, np.ndarray]:
    """``resample_in_arena`` with every ratio on the bankless kernel, whatever its bank would take: same arguments, same placement
    (``resample_layout``), ONE ``hipfeat_sinc_run`` launch for all cuts, each with its own rates (none when every ratio is None)."""
    keys = _ratio_keys(ratios)
    in_offsets, in_lengths = _lib.i64(offsets), _lib.i64(lengths)
    offsets, lengths, _, groups = _grouped_layout(in_offsets, in_lengths, keys, lambda k: k, tail_start)
    _check_arena(arena, offsets, lengths, groups, "resampled")
    _sinc_groups_in_arena(arena, in_offsets, in_lengths, offsets, lengths, groups)
    return offsets, lengths


class _ArenaHandle:
    """What the per-device objects of the arena launches share: the library's ticketed handle ``hipfeat_<_KIND>`` on one device, created
    here and destroyed by ``close``; ``_lock`` serialises the subclass's ``plan``."""

    _KIND = ""

    def __init__(self, device: Union[str, torch.device, None] = None):
        self.lib = _lib.load()
        self.handle = 0
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise _lib.HipFeatError(1, f"{type(self).__name__} runs on an AMD GPU ('cuda[:i]' device), got device={dev}")
        if not torch.cuda.is_available():
            raise _lib.HipFeatError(2, "no HIP device is visible (torch.cuda.is_available() is False); there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        out = np.zeros(1, dtype=np.uint64)
        self.lib.check(f"hipfeat_{self._KIND}_create", int(self.device.index), _lib.addr(out))
        self.handle = int(out[0])
        self._lock = threading.Lock()

    def close(self):
        if self.handle:
            try:
                self.lib.raw(f"hipfeat_{self._KIND}_destroy", self.handle)
            finally:
                self.handle = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _get_or_create(cache: dict, cls, lock, device: Union[str, torch.device, None]):
    """The one object of ``cls`` per device index, kept in ``cache``."""
    dev = torch.device("cuda" if device is None else device)
    index = dev.index if dev.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)
    with lock:
        r = cache.get(int(index))
        if r is None:
            r = cache[int(index)] = cls(torch.device(dev.type, index))
        return r


class HipSincResampler(_ArenaHandle):
    """The sinc resampler without a filter bank (``hipfeat_sinc``, include/hipfeat.h; csrc/kernel_sinc.hpp): the arithmetic of
    ``ResampleTensor`` (lhotse/augmentation/resample.py:184-315) for ANY rate pair, every row of a launch with its own -- the weights are
    evaluated on the device where they are not zero.  One object per device (``get_or_create_sinc``); it may be shared by threads."""

    _KIND = "sinc"  # hipfeat_sinc_create / _destroy

    def plan(self, in_offsets, in_lens, rates: Sequence[Tuple[int, int]], out_offsets, arena_floats: int):
        """Host only -> (ticket, output lengths, info = [ticket, arena floats needed, workgroups, largest window])."""
        io, il, oo = _lib.i64(in_offsets), _lib.i64(in_lens), _lib.i64(out_offsets)
        src = np.ascontiguousarray([r[0] for r in rates], dtype=np.int32)
        dst = np.ascontiguousarray([r[1] for r in rates], dtype=np.int32)
        n = len(io)
        if not (len(il) == len(oo) == len(src) == n):
            raise ValueError("sinc tables: one entry per row in every table")
        out_lens, info = np.zeros(n, dtype=np.int64), np.zeros(4, dtype=np.int64)
        with self._lock:
            self.lib.check("hipfeat_sinc_plan", self.handle, n, _lib.addr(io), _lib.addr(il), _lib.addr(src), _lib.addr(dst), _lib.addr(oo), int(arena_floats),
                           _lib.addr(out_lens), _lib.addr(info))
        return int(info[0]), out_lens, info

    def run(self, ticket: int, arena: torch.Tensor, stream: Optional[int] = None) -> None:
        assert arena.dtype == torch.float32 and arena.is_contiguous() and arena.ndim == 1 and arena.device == self.device
        with torch.cuda.device(self.device):
            self.lib.check("hipfeat_sinc_run", self.handle, int(ticket), arena.data_ptr(), arena.numel(), int(_raw_stream(arena.device) if stream is None else stream))

    def weights(self, source_rate: int, target_rate: int) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """The filter of a rate pair as the kernel evaluates it -> (weights ``(new, W)`` float32, first taps ``(new,)`` int32, width):
        tap d of phase ph is the reference's ``kernel[ph][first[ph] + d]``."""
        dims = np.zeros(3, dtype=np.int32)
        self.lib.check("hipfeat_sinc_weights", self.handle, int(source_rate), int(target_rate), None, None, _lib.addr(dims), None)
        with torch.cuda.device(self.device):
            w = torch.empty((int(dims[0]), int(dims[1])), dtype=torch.float32, device=self.device)
            first = torch.empty(int(dims[0]), dtype=torch.int32, device=self.device)
            self.lib.check("hipfeat_sinc_weights", self.handle, int(source_rate), int(target_rate), w.data_ptr(), first.data_ptr(), _lib.addr(dims),
                           int(_raw_stream(self.device)))
        return w, first, int(dims[2])


_sincs: Dict[int, HipSincResampler] = {}
_sinc_lock = threading.Lock()  # (its own: get_or_create_resampler holds _cache_lock while a bankless HipResampleTensor asks for the device's object)


def get_or_create_sinc(device: Union[str, torch.device, None] = None) -> HipSincResampler:
    return _get_or_create(_sincs, HipSincResampler, _sinc_lock, device)


def _speed_keys(factors) -> list:
    return [None if f == 1.0 else f for f in np.asarray(factors, dtype=np.float64).tolist()]


def perturbed_layout(offsets: np.ndarray, lengths: np.ndarray, factors: Sequence[float], sampling_rate: int,
                     tail_start: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """Where ``perturb_speed_in_arena`` puts every cut and how long it comes out -- host arithmetic only, THE placement rule: cuts with
    factor 1 stay, the others go behind ``tail_start`` factor by factor in ascending order, every resampled cut on a 16-byte boundary,
    ``ceil(new * n / orig)`` samples in float32 (resample.py:309) with orig : new = round(sr * f) : sr reduced by their gcd
    (resample.py:219-222).  -> (offsets, lengths, first free float behind the resampled cuts, 16-byte aligned)."""
    return _grouped_layout(offsets, lengths, _speed_keys(factors), lambda f: (round(sampling_rate * f), int(sampling_rate)), tail_start)[:3]


def perturb_speed_in_arena(arena: torch.Tensor, offsets: np.ndarray, lengths: np.ndarray, factors: Sequence[float], sampling_rate: int,
                           tail_start: int) -> Tuple[np.ndarray, np.ndarray]:
    """Mixed-factor speed perturbation of a device-resident packed mini-batch (``PerturbSpeed`` picks one factor per cut,
    lhotse/dataset/cut_transforms/perturb_speed.py:8-47; the arithmetic is ``Speed``, lhotse/augmentation/torchaudio.py:26-42).

    ``arena`` is ONE float32 device buffer: the cuts at ``offsets`` / ``lengths`` in its front part, free space from ``tail_start`` on
    (``perturbed_tail_floats`` says how much).  Cuts with factor 1 stay where they are; the others are resampled -- one launch per
    distinct factor -- into the tail.  Returns the per-cut (offsets, lengths) of the perturbed batch inside the same arena, i.e. exactly
    what ``hipfeat_extract*`` takes next: no copy of the unperturbed cuts, no host round trip, no second buffer."""
    in_offsets, in_lengths = _lib.i64(offsets), _lib.i64(lengths)
    ratio_of = lambda f: (round(sampling_rate * f), int(sampling_rate))  # noqa: E731
    offsets, lengths, _, groups = _grouped_layout(in_offsets, in_lengths, _speed_keys(factors), ratio_of, tail_start)
    _resample_groups_in_arena(arena, in_offsets, in_lengths, offsets, lengths, groups, ratio_of, "perturbed")
    return offsets, lengths


def _raw_stream(device: torch.device) -> int:
    """hipStream_t of torch's current stream on `device` as an integer (the private accessor that skips building a Stream object,
    where this torch has it: the call sits on a per-mini-batch path)."""
    try:
        return torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device())
    except AttributeError:  # pragma: no cover
        return torch.cuda.current_stream(device).cuda_stream


# ---- the same in ONE launch for all factors, fused with what else has to precede the feature launch ------------------------------
class HipSpeedBank:
    """The resamplers a mini-batch may refer to, resident on one device (``hipfeat_speed_bank``, include/hipfeat.h): mixed-factor speed
    perturbation of a packed mini-batch + the collated feature extraction as a PAIR of launches with no host -> device copy in front of
    them (``hipfeat_minibatch_plan`` / ``hipfeat_minibatch_run``).  Factors must be among 0.9 / 1.1 (the compile-time ratios of the
    mixed launch) and 1.0; anything else raises ``HipFeatError`` (UNSUPPORTED) -- use ``perturb_speed_in_arena``.

        bank = HipSpeedBank([0.9, 1.0, 1.1], 16000, "cuda:0")
        feats, frames, offs, lens = bank.extract_collated(extractor.plan, arena, offsets, lengths, bank.index_of(factors), tail_start, LOG_EPSILON)

    bit-identical to ``perturb_speed_in_arena`` + ``plan.run_collated``."""

    def __init__(self, factors: Sequence[float], sampling_rate: int, device: Union[str, torch.device, None] = None):
        self.sampling_rate = int(sampling_rate)
        self.factors = sorted({float(f) for f in factors if float(f) != 1.0})
        self.resamplers = [get_or_create_resampler(round(sampling_rate * f), sampling_rate, device) for f in self.factors]
        self.lib = _lib.load()
        if self.resamplers:
            self.device = self.resamplers[0].device
        else:  # a bank without resamplers (plain collated extraction through the launch pair): the device is the caller's
            dev = torch.device("cuda" if device is None else device)
            self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        self.handle = 0
        for f, r in zip(self.factors, self.resamplers):
            if r.handle == 0:  # (no dense bank: not a ratio of the mixed launch either)
                raise _lib.HipFeatError(_lib.ERR_UNSUPPORTED, f"speed factor {f} at {sampling_rate} Hz has no dense filter bank; use perturb_speed_in_arena")
        handles = np.array([r.handle for r in self.resamplers], dtype=np.uint64)
        out = np.zeros(1, dtype=np.uint64)
        self.lib.check("hipfeat_speed_bank_create", _lib.addr(handles) if len(handles) else None, len(handles), _lib.addr(out))
        self.handle = int(out[0])
        self._info = np.zeros(4, dtype=np.int64)
        self._info_addr = _lib.addr(self._info)
        self._plan_fn, self._run_fn = self.lib.fn("hipfeat_minibatch_plan"), self.lib.fn("hipfeat_minibatch_run")  # bound once: this is a per-mini-batch path
        self._lock = threading.Lock()

    def index_of(self, factors: Sequence[float]) -> np.ndarray:
        """Per-cut bank index (int32; -1 = factor 1.0 = the cut stays where it is)."""
        fac = np.asarray(factors, dtype=np.float64)
        idx = np.full(len(fac), -1, dtype=np.int32)
        for k, f in enumerate(self.factors):
            idx[fac == f] = k
        bad = (idx < 0) & (fac != 1.0)
        if bad.any():
            raise ValueError(f"factors {sorted(set(fac[bad].tolist()))} are not in this bank ({self.factors})")
        return idx

    def extract_collated(self, plan, arena: torch.Tensor, offsets: np.ndarray, lengths: np.ndarray, bank_index: np.ndarray, tail_start: int,
                         pad_value: float, max_samples: Optional[np.ndarray] = None, zero_pad_batch: bool = False,
                         stream: Optional[int] = None, group_sizes: Optional[np.ndarray] = None):
        """-> (features (B, Tmax, F) on the arena's device, frame counts, per-cut offsets and lengths of the PERTURBED batch in the arena).
        ``offsets`` / ``lengths`` int64, ``bank_index`` int32 (``index_of``), all C-contiguous numpy arrays; the arena must hold
        ``perturbed_tail_floats`` floats behind ``tail_start``.

        ``group_sizes`` (int64 array, K entries adding up to B): the batch is K mini-batches -- a prefetching loader's -- served by ONE
        pair of launches; the first result then is a LIST of K dense ``(B_k, Tmax_k, F)`` tensors (views of one allocation)."""
        B = len(lengths)
        K = 0 if group_sizes is None else len(group_sizes)
        res = np.empty(3 * B + 2 * K, dtype=np.int64)  # offsets, lengths, frames of the perturbed batch; (first row, rows per cut) per group
        a = res.__array_interface__["data"][0]
        info, fn = self._info, self._plan_fn
        with self._lock:  # (the info block is shared; the library serialises the calls anyway)
            st = fn(self.handle, plan.handle, B, offsets.__array_interface__["data"][0], lengths.__array_interface__["data"][0],
                    bank_index.__array_interface__["data"][0], None if max_samples is None else max_samples.__array_interface__["data"][0],
                    int(tail_start), 1 if zero_pad_batch else 0, K, None if K == 0 else group_sizes.__array_interface__["data"][0],
                    a, a + 8 * B, a + 16 * B, (a + 24 * B) if K else None, self._info_addr)
            if st != 0:
                raise _lib.HipFeatError(int(st), self.lib.last_error())
            ticket, tmax, rows = int(info[0]), int(info[2]), int(info[3])
        F = plan.feature_dim
        if stream is None:
            stream = _raw_stream(arena.device)
        if K > 1:
            flat = torch.empty(rows * F, dtype=torch.float32, device=arena.device)
            st = self._run_fn(self.handle, ticket, arena.data_ptr(), arena.numel(), flat.data_ptr(), -1, float(pad_value), int(stream))
            g = res[3 * B :].tolist()
            out = [flat[g[2 * k] * F : (g[2 * k] + int(group_sizes[k]) * g[2 * k + 1]) * F].view(int(group_sizes[k]), g[2 * k + 1], F) for k in range(K)]
        else:
            out = torch.empty((B, tmax, F), dtype=torch.float32, device=arena.device)
            st = self._run_fn(self.handle, ticket, arena.data_ptr(), arena.numel(), out.data_ptr(), tmax, float(pad_value), int(stream))
            if K == 1:
                out = [out]
        if st != 0:
            raise _lib.HipFeatError(int(st), self.lib.last_error())
        return out, res[2 * B : 3 * B], res[:B], res[B : 2 * B]

    def close(self):
        if self.handle:
            try:
                self.lib.raw("hipfeat_speed_bank_destroy", self.handle)
            finally:
                self.handle = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- mixing the tracks of MixedCuts (CutMix / CutSet.mix / .pad) in the same arena --------------------------------------------
def _mix_tables(track_first, src_offsets, src_lens, dst_offsets, snrs, ref_tracks, max_samples):
    """The host tables of ``hipfeat_mix_plan`` as C-contiguous arrays (``snrs``: None / NaN = no SNR)."""
    first = np.ascontiguousarray(track_first, dtype=np.int64)
    n = int(first[-1]) if len(first) else 0
    snr = np.full(n, np.nan, dtype=np.float64) if snrs is None else np.ascontiguousarray([np.nan if s is None else float(s) for s in snrs], dtype=np.float64)
    ref = np.full(len(first) - 1, -1, dtype=np.int32) if ref_tracks is None else np.ascontiguousarray(ref_tracks, dtype=np.int32)
    cap = np.full(len(first) - 1, -1, dtype=np.int64) if max_samples is None else np.ascontiguousarray(max_samples, dtype=np.int64)
    tabs = (first, np.ascontiguousarray(src_offsets, dtype=np.int64), np.ascontiguousarray(src_lens, dtype=np.int64),
            np.ascontiguousarray(dst_offsets, dtype=np.int64), snr, ref, cap)
    if not (len(tabs[1]) == len(tabs[2]) == len(tabs[3]) == len(snr) == n and len(ref) == len(cap) == len(first) - 1):
        raise ValueError("mix tables: the track tables hold track_first[-1] entries, the cut tables len(track_first) - 1")
    return tabs


def mixed_num_samples(track_first, src_lens, dst_offsets, max_samples=None) -> np.ndarray:
    """Samples of every mixed cut: ``max_t(offset_t + n_t)`` (``AudioMixer.num_samples_total``, lhotse/audio/mixer.py:77-82), cut down
    to ``max_samples`` where that is >= 0 and smaller (lhotse/cut/mixed.py:1381-1385)."""
    first = _lib.i64(track_first)
    end = _lib.i64(src_lens) + _lib.i64(dst_offsets)
    out = np.array([int(end[a:b].max(initial=0)) for a, b in zip(first[:-1], first[1:])], dtype=np.int64)
    if max_samples is not None:
        cap = _lib.i64(max_samples)
        out = np.where(cap >= 0, np.minimum(out, cap), out)
    return out


def mixed_tail_floats(track_first, src_lens, dst_offsets, max_samples=None) -> int:
    """Floats the mixed cuts of a mini-batch need behind ``tail_start`` (every mixed cut starts on a 16-byte boundary)."""
    return int(((mixed_num_samples(track_first, src_lens, dst_offsets, max_samples) + 3) & ~3).sum()) + 3


class HipMixer(_ArenaHandle):
    """The device half of ``MixedCut.load_audio`` (lhotse/cut/mixed.py:1312-1409) for a packed mini-batch: ``hipfeat_mixer``
    (include/hipfeat.h) owns the workspace of the two launches -- track energies, then gains + the scaled sum in track order.  Energies
    and gains never visit the host, so the feature launch can follow on the same stream.  One mixer per device (``get_or_create_mixer``);
    it may be shared by threads."""

    _KIND = "mixer"  # hipfeat_mixer_create / _destroy

    def plan(self, track_first, src_offsets, src_lens, dst_offsets, snrs=None, ref_tracks=None, max_samples=None, tail_start: int = 0):
        """Host only -> (ticket, out_offsets, out_lengths, info = [ticket, arena floats needed, energy items, mix items])."""
        first, so, sl, do, snr, ref, cap = _mix_tables(track_first, src_offsets, src_lens, dst_offsets, snrs, ref_tracks, max_samples)
        n = len(first) - 1
        out_offs, out_lens, info = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(4, dtype=np.int64)
        with self._lock:
            self.lib.check("hipfeat_mix_plan", self.handle, n, _lib.addr(first), _lib.addr(so), _lib.addr(sl), _lib.addr(do), _lib.addr(snr), _lib.addr(ref),
                           _lib.addr(cap), int(tail_start), _lib.addr(out_offs), _lib.addr(out_lens), _lib.addr(info))
        return int(info[0]), out_offs, out_lens, info

    def run(self, ticket: int, arena: torch.Tensor, stream: Optional[int] = None) -> None:
        assert arena.dtype == torch.float32 and arena.is_contiguous() and arena.ndim == 1 and arena.device == self.device
        with torch.cuda.device(self.device):
            self.lib.check("hipfeat_mix_run", self.handle, int(ticket), arena.data_ptr(), arena.numel(), int(_raw_stream(arena.device) if stream is None else stream))


_mixers: Dict[int, HipMixer] = {}


def get_or_create_mixer(device: Union[str, torch.device, None] = None) -> HipMixer:
    return _get_or_create(_mixers, HipMixer, _cache_lock, device)


def mix_in_arena(arena: torch.Tensor, track_first, src_offsets, src_lens, dst_offsets, snrs=None, ref_tracks=None, max_samples=None,
                 tail_start: int = 0, mixer: Optional[HipMixer] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Mix the tracks of a device-resident packed mini-batch of ``MixedCut``s (lhotse/cut/mixed.py:1312-1409, lhotse/audio/mixer.py:10-172);
    the counterpart of ``perturb_speed_in_arena``, and what runs behind it when a track carries a pending ``Speed``.

    ``arena`` is ONE float32 device buffer: all tracks in front of ``tail_start``, free space behind it (``mixed_tail_floats``).  The tracks
    of cut ``c`` are ``[track_first[c], track_first[c + 1])`` of the track tables: ``src_offsets`` (arena offset, -1 = a padding track
    without a source), ``src_lens``, ``dst_offsets`` (first sample inside the cut), ``snrs`` (dB; None / NaN = no SNR); ``ref_tracks[c]``
    = the SNR reference track as an index within the cut (-1 = none), ``max_samples[c]`` = the cut's sample count when the mix comes
    out a sample or two longer (-1 = no cap).  Returns the per-cut (offsets, lengths) of the mixed cuts inside the same arena, i.e.
    what ``hipfeat_extract*`` takes next.  Two launches on the current stream, no device -> host copy, bit-identical from run to run."""
    assert arena.dtype == torch.float32 and arena.is_contiguous() and arena.ndim == 1
    if mixer is None:
        mixer = get_or_create_mixer(arena.device)
    ticket, offs, lens, info = mixer.plan(track_first, src_offsets, src_lens, dst_offsets, snrs, ref_tracks, max_samples, tail_start)
    if int(info[1]) > arena.numel():
        raise ValueError(f"arena too small: {arena.numel()} floats, the mixed cuts need {int(info[1])} (see mixed_tail_floats)")
    mixer.run(ticket, arena)
    return offs, lens


# ---- reverberation with a recorded room impulse response in the same arena ------------------------------------------------------
RIR_SCALING_FACTOR = 0.5 ** 15  # (lhotse/augmentation/rir.py:34)


def reverb_tail_floats(src_lens) -> int:
    """Floats the reverberated channels of a mini-batch need behind ``tail_start`` (every output starts on a 16-byte boundary)."""
    return int(((_lib.i64(src_lens) + 3) & ~3).sum()) + 3


REVERB_METHODS = {"direct": 0, "fft": 1, "auto": 2}  # hipfeat_reverb_plan_method's `method`
REVERB_FFT_BLOCK = 1024        # kRfBlock: new samples per 2048-point transform
REVERB_FFT_SPEC_FLOATS = 2048  # kRfSpecFloats: floats of one spectrum in the workspace
# The crossover of "auto": the smallest tap count of the grid of tools/bench_reverb_fft.py (256 ... 32768) from which the FFT route is
# faster than the direct form at every larger tap count -- profiles/reverb_fft_bench.json, "auto_min_taps" (24 x 200 000 samples: 0.139
# against 0.206 ms at 1024 taps, 0.453 against 5.06 ms at 32768; at 512 taps 0.143 against 0.142 ms, at 256 0.146 against 0.109: the
# direct form) and "auto_min_taps_one_item_30s" (0.063 against 0.066 ms at 1024; 0.063 against 0.055 at 512): both 1024.
REVERB_AUTO_MIN_TAPS = 1024


def reverb_method_code(method: str) -> int:
    if method not in REVERB_METHODS:
        raise ValueError(f"reverb method {method!r}: expected one of {sorted(REVERB_METHODS)}")
    return REVERB_METHODS[method]


def reverb_fft_tail_floats(src_lens, rir_lens, shifts, rir_offsets=None) -> int:
    """Floats the channels of a mini-batch reverberated on the FFT route need behind ``tail_start``: the outputs
    (``reverb_tail_floats``) and behind them the spectra workspace of include/hipfeat.h's formula, 2048 floats per spectrum --
    ``ceil(L / 1024)`` per impulse response and ``min(j1, (N - 1) // 1024 + 1) + 1`` per item, ``j1 = (shift + N - 1) // 1024``.  With
    ``rir_offsets`` an impulse response that several items share (same offset and length) is counted once, as the plan does; without,
    every item counts its own (an upper bound)."""
    n, taps, s = _lib.i64(src_lens), _lib.i64(rir_lens), _lib.i64(shifts)
    if not (len(n) == len(taps) == len(s)):
        raise ValueError("reverb tables: one entry per item in every table")
    parts = (taps + REVERB_FFT_BLOCK - 1) // REVERB_FFT_BLOCK
    if rir_offsets is not None:
        first = {}
        for k, key in enumerate(zip(_lib.i64(rir_offsets).tolist(), taps.tolist())):
            first.setdefault(key, k)
        parts = parts[sorted(first.values())]
    nx = np.minimum((s + n - 1) // REVERB_FFT_BLOCK, (n - 1) // REVERB_FFT_BLOCK + 1) + 1
    return reverb_tail_floats(n) + REVERB_FFT_SPEC_FLOATS * int(parts.sum() + nx.sum())


def reverb_workspace_floats(src_lens, rir_lens, shifts, rir_offsets=None, method: str = "direct", min_fft_taps: Optional[int] = None) -> int:
    """The spectra workspace alone (``reverb_fft_tail_floats`` minus the outputs) of the items that ``method`` sends down the FFT route:
    none with ``"direct"``, all with ``"fft"``, those of at least ``min_fft_taps`` (None: ``REVERB_AUTO_MIN_TAPS``) taps with ``"auto"``."""
    code = reverb_method_code(method)
    n, taps, s = _lib.i64(src_lens), _lib.i64(rir_lens), _lib.i64(shifts)
    keep = np.zeros(len(n), dtype=bool) if code == 0 else np.ones(len(n), dtype=bool) if code == 1 else \
        taps >= int(REVERB_AUTO_MIN_TAPS if min_fft_taps is None else min_fft_taps)
    if not keep.any():
        return 0
    ro = None if rir_offsets is None else _lib.i64(rir_offsets)[keep]
    return reverb_fft_tail_floats(n[keep], taps[keep], s[keep], ro) - reverb_tail_floats(n[keep])


def scaled_rir(rir: np.ndarray) -> Tuple[np.ndarray, int]:
    """One channel of a loaded RIR -> (``hs = rir * 2^-15`` in float32 -- exact --, ``shift`` = first index of ``max(hs)``)
    (lhotse/augmentation/rir.py:139, 145)."""
    hs = np.ascontiguousarray(rir, dtype=np.float32).reshape(-1) * np.float32(RIR_SCALING_FACTOR)
    return hs, int(np.argmax(hs))


class HipReverb(_ArenaHandle):
    """The device half of ``ReverbWithImpulseResponse.__call__`` (lhotse/augmentation/rir.py:78-153) for a packed mini-batch:
    ``hipfeat_reverb`` (include/hipfeat.h) owns the workspace of the two launches -- direct-form float32 convolution with float64 sums
    of squares, then the power-preserving gain; with ``plan(..., method="fft" | "auto")`` the partitioned FFT convolution of
    kernel_reverb_fft.hpp in four launches, its spectra in the arena behind the outputs.  One object per device
    (``get_or_create_reverb``); it may be shared by threads."""

    _KIND = "reverb"  # hipfeat_reverb_create / _destroy

    def plan(self, src_offsets, src_lens, rir_offsets, rir_lens, shifts, normalize=None, tail_start: int = 0, method: str = "direct",
             min_fft_taps: Optional[int] = None):
        """Host only -> (ticket, out_offsets, info = [ticket, arena floats needed, convolution work items, partial sums]).

        ``method``: ``"direct"`` (the default: ``hipfeat_reverb_plan``, the direct form), ``"fft"`` (partitioned FFT convolution,
        kernel_reverb_fft.hpp) or ``"auto"`` (per item: FFT when ``rir_len >= min_fft_taps``, None = ``REVERB_AUTO_MIN_TAPS``).  With
        ``"fft"`` / ``"auto"`` the plan is ``hipfeat_reverb_plan_method``'s and ``info`` has its 8 fields: the arena floats include the
        spectra workspace (``reverb_fft_tail_floats``), then [4:8] = transforms of the spectra launch, output blocks, gain work items of
        the FFT items, distinct impulse-response spectra."""
        so, sl, ro, rl, sh = (_lib.i64(a) for a in (src_offsets, src_lens, rir_offsets, rir_lens, shifts))
        n = len(so)
        if np.ndim(normalize) == 0:
            normalize = np.full(n, 0 if normalize is None else int(bool(normalize)))
        nm = np.ascontiguousarray(normalize, dtype=np.int32)
        if not (len(sl) == len(ro) == len(rl) == len(sh) == len(nm) == n):
            raise ValueError("reverb tables: one entry per item in every table")
        code = reverb_method_code(method)
        if code == 0:
            out_offs, info = np.zeros(n, dtype=np.int64), np.zeros(4, dtype=np.int64)
            with self._lock:
                self.lib.check("hipfeat_reverb_plan", self.handle, n, _lib.addr(so), _lib.addr(sl), _lib.addr(ro), _lib.addr(rl), _lib.addr(sh), _lib.addr(nm),
                               int(tail_start), _lib.addr(out_offs), _lib.addr(info))
            return int(info[0]), out_offs, info
        out_offs, info = np.zeros(n, dtype=np.int64), np.zeros(8, dtype=np.int64)
        with self._lock:
            self.lib.check("hipfeat_reverb_plan_method", self.handle, n, _lib.addr(so), _lib.addr(sl), _lib.addr(ro), _lib.addr(rl), _lib.addr(sh), _lib.addr(nm),
                           int(tail_start), code, int(REVERB_AUTO_MIN_TAPS if min_fft_taps is None else min_fft_taps), _lib.addr(out_offs), _lib.addr(info))
        return int(info[0]), out_offs, info

    def run(self, ticket: int, arena: torch.Tensor, stream: Optional[int] = None) -> None:
        assert arena.dtype == torch.float32 and arena.is_contiguous() and arena.ndim == 1 and arena.device == self.device
        with torch.cuda.device(self.device):
            self.lib.check("hipfeat_reverb_run", self.handle, int(ticket), arena.data_ptr(), arena.numel(), int(_raw_stream(arena.device) if stream is None else stream))


_reverbs: Dict[int, HipReverb] = {}


def get_or_create_reverb(device: Union[str, torch.device, None] = None) -> HipReverb:
    return _get_or_create(_reverbs, HipReverb, _cache_lock, device)


def reverb_in_arena(arena: torch.Tensor, src_offsets, src_lens, rir_offsets, rir_lens, shifts, normalize=None, tail_start: int = 0,
                    reverb: Optional[HipReverb] = None, method: str = "direct", min_fft_taps: Optional[int] = None) -> np.ndarray:
    """Reverberate the channels of a device-resident packed mini-batch (``ReverbWithImpulseResponse.__call__``,
    lhotse/augmentation/rir.py:78-153); the counterpart of ``perturb_speed_in_arena`` / ``mix_in_arena``, run between the two when a
    track carries ``[Speed, Reverb]``.

    ``arena`` is ONE float32 device buffer: all sources and all SCALED impulse responses (``scaled_rir``) in front of ``tail_start``, free
    space behind it (``reverb_tail_floats``).  Item ``i`` convolves the ``src_lens[i]`` samples at ``src_offsets[i]`` with the
    ``rir_lens[i]`` taps at ``rir_offsets[i]``, keeps the samples from ``shifts[i]`` on and, where ``normalize[i]``, scales them to the
    input's power.  Returns the arena offsets of the outputs (``src_lens[i]`` samples each).  Two launches on the current stream, no
    device -> host copy, bit-identical from run to run.

    ``method="fft"`` (or ``"auto"``: per item, from ``min_fft_taps`` / ``REVERB_AUTO_MIN_TAPS`` taps on) takes the partitioned FFT
    convolution instead of the direct form -- four launches, and the free space must also hold the spectra workspace behind the outputs
    (``reverb_fft_tail_floats``)."""
    assert arena.dtype == torch.float32 and arena.is_contiguous() and arena.ndim == 1
    if reverb is None:
        reverb = get_or_create_reverb(arena.device)
    ticket, offs, info = reverb.plan(src_offsets, src_lens, rir_offsets, rir_lens, shifts, normalize, tail_start, method, min_fft_taps)
    if int(info[1]) > arena.numel():
        hint = "reverb_tail_floats" if method == "direct" else "reverb_fft_tail_floats"
        raise ValueError(f"arena too small: {arena.numel()} floats, the reverberated cuts need {int(info[1])} (see {hint})")
    reverb.run(ticket, arena)
    return offs


def reverb_items(num_input_channels: int, num_rir_channels: int, rir_given: bool = True) -> List[Tuple[int, int]]:
    """The reference's four mono / multi-channel cases (lhotse/augmentation/rir.py:90-135) as ``(input channel, rir channel)`` per
    output channel; its assertions as ``ValueError``s with the same conditions."""
    mono = num_input_channels == 1
    if mono:
        if not (rir_given or num_rir_channels == 1):
            raise ValueError("For mono input, either provide an RIR explicitly or set rir_channels to [0].")
    elif not (num_rir_channels == 1 or num_rir_channels == num_input_channels):
        raise ValueError("For multi-channel input, we only support mono RIR or RIR with the same number of channels as the input.")
    d_out = num_rir_channels if mono else num_input_channels
    return [(0 if mono else d, 0 if num_rir_channels == 1 else d) for d in range(d_out)]


def load_rir(rir, rir_channels: Sequence[int], early_only: bool) -> np.ndarray:
    """The RIR samples ``(D_rir, L)`` the way the reference loads them (lhotse/augmentation/rir.py:116-122): its own calls are the
    contract.  ``rir``: a lhotse ``Recording`` / ``Cut``, or -- without lhotse -- an array ``(C, L)`` of already loaded samples."""
    if isinstance(rir, np.ndarray):
        a = np.atleast_2d(rir)[list(rir_channels)]
        return np.ascontiguousarray(a, dtype=np.float32)
    cut = rir.to_cut() if type(rir).__name__ == "Recording" else rir
    cut = cut.with_channels(list(rir_channels))
    if early_only:
        cut = cut.truncate(duration=0.05)
    return np.ascontiguousarray(np.atleast_2d(cut.load_audio()), dtype=np.float32)


@dataclass
class HipReverbWithImpulseResponse(AudioTransform):
    """Reverberation with a recorded room impulse response on the GPU; drop-in for ``lhotse.augmentation.ReverbWithImpulseResponse``
    (rir.py:12-166) with ``rir`` given: same fields, same dict round trip, output of the input's length ("shift output").  The random
    generator (``rir=None``) is not served: ``HipFeatError`` (UNSUPPORTED)."""

    rir: Optional[Union[dict, object]] = None
    normalize_output: bool = True
    early_only: bool = False
    rir_channels: List[int] = None  # type: ignore[assignment]
    rir_generator: Optional[Union[dict, object]] = None
    device: str = "cuda"
    method: str = "direct"  # "direct" | "fft" | "auto" (reverb_in_arena); not a field of the reference: to_dict omits it when "direct"

    def __post_init__(self):
        reverb_method_code(self.method)
        if self.rir_channels is None:
            self.rir_channels = [0]
        self.rir_channels = [int(c) for c in self.rir_channels]
        if isinstance(self.rir, dict):
            if not HAVE_LHOTSE:
                raise ImportError("a serialised RIR manifest needs lhotse to be read back (lhotse.serialization.deserialize_item)")
            from lhotse.serialization import deserialize_item  # type: ignore

            rir = self.rir.copy()  # (rir.py:40-45: deserialisation is destructive)
            if "recording" in self.rir:
                rir["recording"] = rir["recording"].copy()
            self.rir = deserialize_item(rir)
        if self.rir is None:
            raise _lib.HipFeatError(_lib.ERR_UNSUPPORTED, "HipReverbWithImpulseResponse needs a recorded impulse response (rir=...): the random "
                                    "RIR generator of the reference (rir=None, rir_generator) is not served on the device")
        if not isinstance(self.rir, np.ndarray) and not all(c < self.rir.num_channels for c in self.rir_channels):
            raise ValueError("Invalid channel index in `rir_channels`")

    def to_dict(self) -> dict:
        rir = self.rir.to_dict() if hasattr(self.rir, "to_dict") else self.rir
        gen = self.rir_generator if self.rir_generator is None or isinstance(self.rir_generator, dict) else self.rir_generator.to_dict()
        kwargs = {"rir": rir, "normalize_output": self.normalize_output, "early_only": self.early_only,
                  "rir_channels": list(self.rir_channels), "rir_generator": gen, "device": self.device}
        if self.method != "direct":
            kwargs["method"] = self.method
        return {"name": type(self).__name__, "kwargs": kwargs}

    def __call__(self, samples: Union[np.ndarray, torch.Tensor], sampling_rate: int) -> Union[np.ndarray, torch.Tensor]:
        is_tensor = isinstance(samples, torch.Tensor)
        x = samples if is_tensor else torch.from_numpy(np.ascontiguousarray(samples))
        if x.ndim != 2:
            raise ValueError(f"expected samples of shape (channels, num_samples), got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise TypeError(f"expected float32 samples, got {x.dtype}")
        d_in, n = int(x.shape[0]), int(x.shape[1])
        rir = load_rir(self.rir, self.rir_channels, self.early_only)
        items = reverb_items(d_in, int(rir.shape[0]))
        scaled = [scaled_rir(rir[c]) for c in range(rir.shape[0])]
        dev = torch.device(self.device)
        dev = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index) if dev.type == "cuda" else dev
        # one arena: the input channels, the scaled RIRs, the outputs (every part on a 16-byte boundary)
        n4, taps = (n + 3) & ~3, int(rir.shape[1])
        l4 = (taps + 3) & ~3
        front = d_in * n4 + len(scaled) * l4
        host = np.zeros(front, dtype=np.float32)
        for c, (hs, _) in enumerate(scaled):
            host[d_in * n4 + c * l4 : d_in * n4 + c * l4 + taps] = hs
        rir_offs, shifts = [d_in * n4 + b * l4 for _, b in items], [scaled[b][1] for _, b in items]
        tail = reverb_tail_floats([n] * len(items)) if self.method == "direct" else reverb_fft_tail_floats([n] * len(items), [taps] * len(items), shifts, rir_offs)
        arena = torch.empty(front + tail, dtype=torch.float32, device=dev)
        arena[:front].copy_(torch.from_numpy(host))
        arena[: d_in * n4].view(d_in, n4)[:, :n].copy_(x)
        offs = reverb_in_arena(arena, [a * n4 for a, _ in items], [n] * len(items), rir_offs, [taps] * len(items), shifts,
                               [int(bool(self.normalize_output))] * len(items), front, method=self.method)
        out = torch.stack([arena[int(o) : int(o) + n] for o in offs])
        return out.to(samples.device) if is_tensor else out.cpu().numpy()

    def reverse_timestamps(self, offset: Seconds, duration: Optional[Seconds], sampling_rate: Optional[int]) -> Tuple[Seconds, Optional[Seconds]]:
        """The output is shifted to the input's length: timestamps are unchanged (rir.py:155-166)."""
        return offset, duration


# ---- level changes (PerturbVolume, Clipping) in the same arena ------------------------------------------------------------------
LEVEL_MAX_OPS = 4  # ops of one program (kLvMaxOps)
_LV_SCALE, _LV_CLIP = 0, 1
_LV_HARD, _LV_NORMALIZE, _LV_USE_GAIN = 1, 2, 4


def level_op_tables(programs) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``programs`` -- per item a list of ``("volume", factor)`` / ``("clip", hard, gain_db, normalize)`` -- as the op tables of
    ``hipfeat_level_plan``: ``(op_first[n + 1], kind, value, flags)``.  ``g = (float)10**(gain_db / 20)`` and ``|gain_db| >= 0.1``
    are decided here, with the reference's own expressions (lhotse/augmentation/clipping.py:44-45)."""
    first, kind, value, flags = [0], [], [], []
    for prog in programs:
        for op in prog:
            if op[0] == "volume" and len(op) == 2:
                kind.append(_LV_SCALE), value.append(np.float32(op[1])), flags.append(0)
            elif op[0] == "clip" and len(op) == 4:
                _, hard, gain_db, normalize = op
                use_gain = abs(gain_db) >= 0.1
                kind.append(_LV_CLIP), value.append(np.float32(10 ** (gain_db / 20.0)))
                flags.append((_LV_HARD if hard else 0) | (_LV_NORMALIZE if normalize else 0) | (_LV_USE_GAIN if use_gain else 0))
            else:
                raise ValueError(f"unknown level op {op!r}: expected ('volume', factor) or ('clip', hard, gain_db, normalize)")
        first.append(len(kind))
    return _lib.i64(first), np.asarray(kind, dtype=np.int32), np.asarray(value, dtype=np.float32), np.asarray(flags, dtype=np.int32)


class HipLevel(_ArenaHandle):
    """The device half of ``Volume.__call__`` (lhotse/augmentation/torchaudio.py:395-406) and ``Clipping.__call__``
    (lhotse/augmentation/clipping.py:28-61) for a packed mini-batch: ``hipfeat_level`` (include/hipfeat.h) owns the workspace of the two
    launches -- max |x| per item, then the ops.  One object per device (``get_or_create_level``); it may be shared by threads."""

    _KIND = "level"  # hipfeat_level_create / _destroy

    def plan(self, src_offsets, src_lens, programs, dst_offsets=None):
        """Host only -> (ticket, info = [ticket, arena floats needed, peak work items, apply work items])."""
        so, sl = _lib.i64(src_offsets), _lib.i64(src_lens)
        do = so if dst_offsets is None else _lib.i64(dst_offsets)
        first, kind, value, flags = level_op_tables(programs)
        n = len(so)
        if not (len(sl) == len(do) == len(first) - 1 == n):
            raise ValueError("level tables: one entry per item in every table")
        info = np.zeros(4, dtype=np.int64)
        with self._lock:
            self.lib.check("hipfeat_level_plan", self.handle, n, _lib.addr(so), _lib.addr(sl), _lib.addr(do), _lib.addr(first), _lib.addr(kind), _lib.addr(value),
                           _lib.addr(flags), _lib.addr(info))
        return int(info[0]), info

    def run(self, ticket: int, arena: torch.Tensor, stream: Optional[int] = None) -> None:
        assert arena.dtype == torch.float32 and arena.is_contiguous() and arena.ndim == 1 and arena.device == self.device
        with torch.cuda.device(self.device):
            self.lib.check("hipfeat_level_run", self.handle, int(ticket), arena.data_ptr(), arena.numel(), int(_raw_stream(arena.device) if stream is None else stream))


_levels: Dict[int, HipLevel] = {}


def get_or_create_level(device: Union[str, torch.device, None] = None) -> HipLevel:
    return _get_or_create(_levels, HipLevel, _cache_lock, device)


def level_in_arena(arena: torch.Tensor, src_offsets, src_lens, programs, dst_offsets=None, level: Optional[HipLevel] = None) -> np.ndarray:
    """Scale and clip runs of a device-resident packed mini-batch (``Volume`` / ``Clipping``); the counterpart of
    ``perturb_speed_in_arena`` / ``reverb_in_arena`` / ``mix_in_arena``.

    Item ``i`` takes the ``src_lens[i]`` samples at ``src_offsets[i]`` of ``arena`` (ONE float32 device buffer) through ``programs[i]``
    -- 1 to 4 ops ``("volume", factor)`` / ``("clip", hard, gain_db, normalize)``, at most one clip, whose peak is taken over the whole
    item -- and writes them at ``dst_offsets[i]`` (``None``: in place).  A destination may be its item's source, and may overlap
    nothing else.  Returns the destination offsets.  Two launches on the current stream (one when no program clips, none for no items),
    no device -> host copy, bit-identical from run to run."""
    assert arena.dtype == torch.float32 and arena.is_contiguous() and arena.ndim == 1
    so = _lib.i64(src_offsets)
    do = so.copy() if dst_offsets is None else _lib.i64(dst_offsets)
    if len(so) == 0:
        return do
    sl = _lib.i64(src_lens)
    need = int((np.maximum(so, do) + sl).max()) if len(sl) == len(so) == len(do) else 0
    if need > arena.numel():  # (before anything is planned: a plan that is never run would stay outstanding)
        raise ValueError(f"arena too small: {arena.numel()} floats, the items reach to {need}")
    if level is None:
        level = get_or_create_level(arena.device)
    ticket, info = level.plan(so, sl, programs, do)
    assert int(info[1]) == need
    level.run(ticket, arena)
    return do


def _level_call(samples: Union[np.ndarray, torch.Tensor], program, device: str) -> Union[np.ndarray, torch.Tensor]:
    """One array (all its channels: ONE item, as ``np.max(np.abs(samples))`` takes the peak over all of them) through ``program``."""
    is_tensor = isinstance(samples, torch.Tensor)
    x = samples if is_tensor else torch.from_numpy(np.ascontiguousarray(samples))
    if x.dtype != torch.float32:
        raise TypeError(f"expected float32 samples, got {x.dtype}")
    if x.numel() == 0:
        raise ValueError("zero-size array: the reference's np.max raises here too")
    dev = torch.device(device)
    dev = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index) if dev.type == "cuda" else dev
    arena = torch.empty(x.numel(), dtype=torch.float32, device=dev)  # (a copy: the caller's samples stay as they are)
    arena.copy_(x.reshape(-1))
    level_in_arena(arena, [0], [arena.numel()], [program])
    out = arena.view(x.shape)
    return out.to(samples.device) if is_tensor else out.cpu().numpy()


@dataclass
class HipVolume(AudioTransform):
    """Volume perturbation (``sox vol``) on the GPU; drop-in for ``lhotse.augmentation.Volume`` (torchaudio.py:394-418): the samples times
    ``(float)factor``, bit for bit."""

    factor: float
    device: str = "cuda"

    def __call__(self, samples: Union[np.ndarray, torch.Tensor], sampling_rate: int) -> Union[np.ndarray, torch.Tensor]:
        return _level_call(samples, [("volume", self.factor)], self.device)

    def reverse_timestamps(self, offset: Seconds, duration: Optional[Seconds], sampling_rate: Optional[int]) -> Tuple[Seconds, Optional[Seconds]]:
        """Volume perturbation changes no timing (torchaudio.py:408-418)."""
        return offset, duration


@dataclass
class HipClipping(AudioTransform):
    """Clipping / saturation on the GPU; drop-in for ``lhotse.augmentation.Clipping`` (clipping.py:9-67): same fields and defaults; the
    peak is taken over all channels of the array.  Hard clipping reproduces the reference bit for bit; soft clipping is the float64
    ``tanh`` rounded once."""

    hard: bool = False
    gain_db: float = 0.0
    normalize: bool = True
    device: str = "cuda"

    def __call__(self, samples: Union[np.ndarray, torch.Tensor], sampling_rate: int) -> Union[np.ndarray, torch.Tensor]:
        return _level_call(samples, [("clip", self.hard, self.gain_db, self.normalize)], self.device)

    def reverse_timestamps(self, offset, duration, sampling_rate):
        """Clipping changes no timing (clipping.py:63-67)."""
        return offset, duration


# ---- collation: the cuts of the arena as ONE dense zero-padded (B, row_len) tensor ----------------------------------------------
COLLATE_TILE = 4096  # output elements per work item of the collate launch (kCoTile)
_COLLATE_TYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def left_pad_offsets(lengths, row_len: int) -> np.ndarray:
    """Destination offsets that put every cut at the END of its row (``pad_direction="left"``): ``row_len - lengths``."""
    sl = _lib.i64(lengths)
    if len(sl) and int(sl.max()) > int(row_len):
        raise ValueError(f"a cut of {int(sl.max())} samples does not fit a row of {int(row_len)}")
    return int(row_len) - sl


def collate_layout(arena_floats: int, offsets, lengths, row_len: Optional[int] = None, dst_offsets=None):
    """The host arithmetic of ``collate_in_arena`` -> ``(src_offsets, lengths, dst_offsets, row_len)`` as int64; raises ``ValueError``
    for what no launch could serve (tables of unequal length, negative entries, a cut that does not fit its row or the arena)."""
    so, sl = _lib.i64(offsets), _lib.i64(lengths)
    if so.ndim != 1 or so.shape != sl.shape:
        raise ValueError("collate tables: one offset and one length per row")
    if row_len is None:
        row_len = int(sl.max()) if len(sl) else 0
    row_len = int(row_len)
    do = np.zeros(len(so), dtype=np.int64) if dst_offsets is None else _lib.i64(dst_offsets)
    if do.shape != so.shape:
        raise ValueError("collate tables: one destination offset per row")
    if row_len < 0 or (len(so) and (int(so.min()) < 0 or int(sl.min()) < 0 or int(do.min()) < 0)):
        raise ValueError("collate tables: negative offset, length or row length")
    if len(so) and int((do + sl).max()) > row_len:
        raise ValueError(f"a cut reaches to element {int((do + sl).max())} of a row of {row_len}")
    need = int((so + sl)[sl > 0].max()) if (sl > 0).any() else 0
    if need > int(arena_floats):
        raise ValueError(f"arena too small: {int(arena_floats)} floats, the cuts reach to {need}")
    return so, sl, do, row_len


class HipCollator(_ArenaHandle):
    """The device half of ``collate_audio`` (lhotse/dataset/collation.py:148-260) for a packed mini-batch: ``hipfeat_collate``
    (include/hipfeat.h) owns the staged row table of the one launch.  One object per device (``get_or_create_collator``); it may be
    shared by threads."""

    _KIND = "collate"  # hipfeat_collate_create / _destroy

    def plan(self, src_offsets, src_lens, dst_offsets, row_len: int, dtype: torch.dtype = torch.float32):
        """Host only -> (ticket, info = [ticket, arena floats needed, elements of out, work items])."""
        if dtype not in _COLLATE_TYPES:
            raise ValueError(f"collate: float32, float16 or bfloat16 output, got {dtype}")
        so, sl = _lib.i64(src_offsets), _lib.i64(src_lens)
        do = None if dst_offsets is None else _lib.i64(dst_offsets)
        if len(so) != len(sl) or (do is not None and len(do) != len(so)):
            raise ValueError("collate tables: one entry per row in every table")
        info = np.zeros(4, dtype=np.int64)
        with self._lock:
            self.lib.check("hipfeat_collate_plan", self.handle, len(so), _lib.addr(so), _lib.addr(sl), _lib.addr(do), int(row_len), _COLLATE_TYPES[dtype],
                           _lib.addr(info))
        return int(info[0]), info

    def plan_sources(self, first, src_offsets, src_lens, dst_offsets, row_len: int, dtype: torch.dtype = torch.float32):
        """The sources form, host only: row ``r`` is the mean of the ``first[r + 1] - first[r]`` runs of ``src_lens[r]`` samples at
        ``src_offsets[first[r] : first[r + 1]]`` -> (ticket, info) as ``plan``; ``run`` takes the ticket."""
        if dtype not in _COLLATE_TYPES:
            raise ValueError(f"collate: float32, float16 or bfloat16 output, got {dtype}")
        fi, so, sl = _lib.i64(first), _lib.i64(src_offsets), _lib.i64(src_lens)
        do = None if dst_offsets is None else _lib.i64(dst_offsets)
        if len(fi) != len(sl) + 1 or (do is not None and len(do) != len(sl)) or int(fi[-1]) != len(so):
            raise ValueError("collate tables: rows + 1 entries of `first` that end at the number of sources, one length per row")
        info = np.zeros(4, dtype=np.int64)
        with self._lock:
            self.lib.check("hipfeat_collate_plan_sources", self.handle, len(sl), _lib.addr(fi), _lib.addr(so), _lib.addr(sl), _lib.addr(do),
                           int(row_len), _COLLATE_TYPES[dtype], _lib.addr(info))
        return int(info[0]), info

    def run(self, ticket: int, arena: torch.Tensor, out: torch.Tensor, stream: Optional[int] = None) -> None:
        assert arena.dtype == torch.float32 and arena.is_contiguous() and arena.ndim == 1 and arena.device == self.device
        assert out.is_contiguous() and out.device == self.device
        with torch.cuda.device(self.device):
            self.lib.check("hipfeat_collate_run", self.handle, int(ticket), arena.data_ptr(), arena.numel(), out.data_ptr(), out.numel(),
                           int(_raw_stream(arena.device) if stream is None else stream))


_collators: Dict[int, HipCollator] = {}


def get_or_create_collator(device: Union[str, torch.device, None] = None) -> HipCollator:
    return _get_or_create(_collators, HipCollator, _cache_lock, device)


def collate_in_arena(arena: torch.Tensor, offsets, lengths, row_len: Optional[int] = None, dst_offsets=None, dtype: torch.dtype = torch.float32,
                     out: Optional[torch.Tensor] = None, collator: Optional[HipCollator] = None) -> Tuple[torch.Tensor, np.ndarray]:
    """The cuts of a device-resident packed mini-batch as ONE dense zero-padded tensor (``collate_audio``, lhotse/dataset/collation.py:148-260);
    what follows ``perturb_speed_in_arena`` / ``level_in_arena`` / ``reverb_in_arena`` / ``mix_in_arena`` when the consumer wants samples.

    Row ``i`` of the result receives the ``lengths[i]`` samples at ``offsets[i]`` of ``arena`` (ONE float32 device buffer), starting at
    element ``dst_offsets[i]`` (``None``: 0, right padding; ``left_pad_offsets(lengths, row_len)``: left padding; "both" is the caller's
    arithmetic, lhotse halves a duration there, lhotse/cut/set.py:3314-3322); everything else of the row is +0.  ``row_len=None``: the
    longest cut (0 for no rows: an empty (0, 0) tensor, nothing is launched).  ``dtype``: float32 (a bit copy), float16 or bfloat16 (one
    round-to-nearest-even conversion, as ``.to(dtype)``).  ``out``: a contiguous tensor of ``dtype`` on the arena's device with at least
    ``B * row_len`` elements that does not overlap the arena; its first ``B * row_len`` elements are the result.  Returns
    ``(out (B, row_len), lengths as int64 numpy)``.  One launch on the current stream, no memset, no device -> host copy."""
    assert arena.dtype == torch.float32 and arena.is_contiguous() and arena.ndim == 1
    if dtype not in _COLLATE_TYPES:
        raise ValueError(f"collate: float32, float16 or bfloat16 output, got {dtype}")
    so, sl, do, row_len = collate_layout(arena.numel(), offsets, lengths, row_len, dst_offsets)  # (before anything is planned)
    rows = len(so)
    if out is not None:
        if out.dtype != dtype or out.device != arena.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {dtype} tensor on {arena.device}")
        if out.numel() < rows * row_len:
            raise ValueError(f"out too small: {out.numel()} elements, {rows} rows of {row_len} take {rows * row_len}")
        a0, o0 = arena.data_ptr(), out.data_ptr()
        if a0 < o0 + out.numel() * out.element_size() and o0 < a0 + arena.numel() * 4:  # (a plan that is never run would stay outstanding)
            raise ValueError("out overlaps the arena")
        res = out.view(-1)[: rows * row_len].view(rows, row_len)
    else:
        res = torch.empty((rows, row_len), dtype=dtype, device=arena.device)
    if rows * row_len == 0:
        return res, sl
    if collator is None:
        collator = get_or_create_collator(arena.device)
    ticket, info = collator.plan(so, sl, None if dst_offsets is None else do, row_len, dtype)
    collator.run(ticket, arena, res)
    return res, sl


COLLATE_MAX_SOURCES = 32  # sources of one row of the sources form (kCoMaxSources)


def collate_sources_layout(arena_floats: int, first, src_offsets, lengths, row_len: Optional[int] = None, dst_offsets=None):
    """The host arithmetic of ``collate_sources_in_arena`` -> ``(first, src_offsets, lengths, dst_offsets, row_len)`` as int64; raises
    ``ValueError`` for what no launch could serve (``first`` that does not start at 0, decreases or does not end at the number of
    sources, more than ``COLLATE_MAX_SOURCES`` sources in a row, tables of unequal length, negative entries, a row that does not fit
    ``row_len`` or a source that does not fit the arena)."""
    fi, so, sl = _lib.i64(first), _lib.i64(src_offsets), _lib.i64(lengths)
    if fi.ndim != 1 or so.ndim != 1 or sl.ndim != 1 or len(fi) != len(sl) + 1:
        raise ValueError("collate tables: one length per row and rows + 1 entries of `first`")
    k = np.diff(fi)
    if int(fi[0]) != 0 or (len(k) and int(k.min()) < 0) or int(fi[-1]) != len(so):
        raise ValueError("collate tables: `first` starts at 0, does not decrease and ends at the number of sources")
    if len(k) and int(k.max()) > COLLATE_MAX_SOURCES:
        raise ValueError(f"a row of {int(k.max())} sources: a row takes at most {COLLATE_MAX_SOURCES}")
    if row_len is None:
        row_len = int(sl.max()) if len(sl) else 0
    row_len = int(row_len)
    do = np.zeros(len(sl), dtype=np.int64) if dst_offsets is None else _lib.i64(dst_offsets)
    if do.shape != sl.shape:
        raise ValueError("collate tables: one destination offset per row")
    if row_len < 0 or (len(so) and int(so.min()) < 0) or (len(sl) and (int(sl.min()) < 0 or int(do.min()) < 0)):
        raise ValueError("collate tables: negative offset, length or row length")
    if len(sl) and int((do + sl).max()) > row_len:
        raise ValueError(f"a row reaches to element {int((do + sl).max())} of a row of {row_len}")
    ends = so + np.repeat(sl, k)
    read = np.repeat(sl, k) > 0
    need = int(ends[read].max()) if read.any() else 0
    if need > int(arena_floats):
        raise ValueError(f"arena too small: {int(arena_floats)} floats, the sources reach to {need}")
    return fi, so, sl, do, row_len


def collate_sources_in_arena(arena: torch.Tensor, first, src_offsets, lengths, row_len: Optional[int] = None, dst_offsets=None,
                             dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None,
                             collator: Optional[HipCollator] = None) -> Tuple[torch.Tensor, np.ndarray]:
    """``collate_in_arena`` for rows of SEVERAL sources: the channel handling of ``collate_audio`` (lhotse/dataset/collation.py:215-241) in
    ONE launch.  Row ``r`` has the ``k = first[r + 1] - first[r]`` sources ``src_offsets[first[r] : first[r + 1]]``, each ``lengths[r]``
    samples of ``arena``: ``k = 0`` -- the row is +0; ``k = 1`` -- the row ``collate_in_arena`` writes, bit for bit; ``k >= 2`` -- per sample
    ``float32((0.0 + float64(x_0) + ... + float64(x_{k-1})) / float64(k))``, the sum in ascending source order, one division, one rounding
    (the mono downmix ``audio.mean(dim=0)``, correctly rounded wherever the float64 sum is exact, as it is for PCM samples), then
    ``.to(dtype)`` of that value.  The mono downmix of a batch is one row per cut with its channels as sources; its ``(B, C, T)`` form is
    ``B * C`` rows of one source or none -- reshape the result.  ``row_len``, ``dst_offsets``, ``dtype``, ``out`` and the result as for
    ``collate_in_arena``.  One launch on the current stream, no memset, no device -> host copy."""
    assert arena.dtype == torch.float32 and arena.is_contiguous() and arena.ndim == 1
    if dtype not in _COLLATE_TYPES:
        raise ValueError(f"collate: float32, float16 or bfloat16 output, got {dtype}")
    fi, so, sl, do, row_len = collate_sources_layout(arena.numel(), first, src_offsets, lengths, row_len, dst_offsets)  # (before anything is planned)
    rows = len(sl)
    if out is not None:
        if out.dtype != dtype or out.device != arena.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {dtype} tensor on {arena.device}")
        if out.numel() < rows * row_len:
            raise ValueError(f"out too small: {out.numel()} elements, {rows} rows of {row_len} take {rows * row_len}")
        a0, o0 = arena.data_ptr(), out.data_ptr()
        if a0 < o0 + out.numel() * out.element_size() and o0 < a0 + arena.numel() * 4:  # (a plan that is never run would stay outstanding)
            raise ValueError("out overlaps the arena")
        res = out.view(-1)[: rows * row_len].view(rows, row_len)
    else:
        res = torch.empty((rows, row_len), dtype=dtype, device=arena.device)
    if rows * row_len == 0:
        return res, sl
    if collator is None:
        collator = get_or_create_collator(arena.device)
    ticket, info = collator.plan_sources(fi, so, sl, None if dst_offsets is None else do, row_len, dtype)
    collator.run(ticket, arena, res)
    return res, sl


# ---- stored features: the tracks of a mini-batch mixed and collated as ONE (B, row_frames, F) tensor ---------------------------
FEATMIX_TILE = 4096  # output elements per work item of the fold launch (kFmTile)
FEATMIX_ENERGY_BLOCK = 16384  # track elements per work item of the energy launch (kFmEnergyBlock)
FEATMIX_MAX_TRACKS = 256  # tracks of one cut (kFmMaxTracks)
FEATMIX_COPY, FEATMIX_FOLD = 0, 1
_FEATMIX_MAX_ROW = (2 ** 31 - 1) // 2  # elements of one row and of one track


class FeatTrack(NamedTuple):
    """One track of a cut of stored features: ``rows`` stored rows of F values at BYTE ``offset`` of the arena (-1: a constant matrix of
    ``value``, a PaddingCut) that stand for ``frames`` frames (``rows=None``: as many; one more or one less is the MonoCut fix-up,
    lhotse/cut/mono.py:61-64) from frame ``first`` of the cut on; ``f16``: stored as binary16; ``snr``: dB, None = none."""

    offset: int
    frames: int
    rows: Optional[int] = None
    f16: bool = False
    first: int = 0
    snr: Optional[float] = None
    value: float = 0.0


class FeatCut(NamedTuple):
    """One cut of the mini-batch: ``form`` FEATMIX_COPY (ONE track, ``pad_value`` behind it; lhotse/cut/mixed.py:1223-1243) or
    FEATMIX_FOLD (the FeatureMixer fold of the tracks, mixed.py:1245-1307); its ``num_frames`` frames go to frames ``[dst_first,
    dst_first + num_frames)`` of its row; ``ref_track``: the SNR reference as an index within ``tracks``, -1 = none."""

    tracks: Sequence[FeatTrack]
    num_frames: int
    form: int = FEATMIX_COPY
    pad_value: float = 0.0
    dst_first: int = 0
    ref_track: int = -1


def featmix_layout(arena_bytes: int, cuts_table: Sequence[FeatCut], F: int, row_frames: Optional[int] = None) -> dict:
    """The host arithmetic of ``featmix_in_arena``: the tables of ``hipfeat_featmix_plan`` as C-contiguous arrays (keys named like its
    arguments, plus ``num_features`` and ``row_frames``; ``row_frames=None``: the longest ``dst_first + num_frames``).  Raises
    ``ValueError`` for what no launch could serve, before anything is planned."""
    F = int(F)
    if F < 1 or F > _FEATMIX_MAX_ROW:
        raise ValueError(f"featmix: {F} features per frame")
    cuts = [c if isinstance(c, FeatCut) else FeatCut(*c) for c in cuts_table]
    if not 1 <= len(cuts) <= 65535:
        raise ValueError(f"featmix: {len(cuts)} cuts (1 ... 65535)")
    if row_frames is None:
        row_frames = max(int(c.dst_first) + int(c.num_frames) for c in cuts)
    row_frames = int(row_frames)
    if row_frames < 0 or row_frames * F > _FEATMIX_MAX_ROW:
        raise ValueError(f"featmix: a row of {row_frames} frames of {F} features is out of range")
    max_frames = _FEATMIX_MAX_ROW // F
    first, form, frames_c, pad, dst, ref = [0], [], [], [], [], []
    so, rows, frames, dtype, start, snr, value = [], [], [], [], [], [], []
    need = 0
    for ci, c in enumerate(cuts):
        trs = [t if isinstance(t, FeatTrack) else FeatTrack(*t) for t in c.tracks]
        if not trs:
            raise ValueError(f"featmix: cut {ci} has no track")
        if len(trs) > FEATMIX_MAX_TRACKS:
            raise ValueError(f"featmix: cut {ci} has {len(trs)} tracks, the launch serves up to {FEATMIX_MAX_TRACKS} per cut")
        if c.form not in (FEATMIX_COPY, FEATMIX_FOLD):
            raise ValueError(f"featmix: cut {ci}: unknown form {c.form!r}")
        T, d0, r = int(c.num_frames), int(c.dst_first), int(c.ref_track)
        if T < 0 or d0 < 0 or d0 + T > row_frames:
            raise ValueError(f"featmix: cut {ci}: {T} frames at frame {d0} do not fit a row of {row_frames}")
        if not -1 <= r < len(trs):
            raise ValueError(f"featmix: cut {ci}: reference track {r} of {len(trs)}")
        if c.form == FEATMIX_COPY and len(trs) != 1:
            raise ValueError(f"featmix: cut {ci}: the copy form takes one track, got {len(trs)}")
        total = 0
        for ti, t in enumerate(trs):
            off, n, o = int(t.offset), int(t.frames), int(t.first)
            const = off == -1
            nr = n if const or t.rows is None else int(t.rows)
            if off < -1 or o < 0:
                raise ValueError(f"featmix: cut {ci}, track {ti}: negative offset")
            if n < 0 or n > max_frames or o + n > max_frames:
                raise ValueError(f"featmix: cut {ci}, track {ti}: {n} frames at frame {o} out of range")
            if abs(nr - n) > 1 or (n > 0 and nr < 1):
                raise ValueError(f"featmix: cut {ci}, track {ti}: {nr} stored rows for {n} frames (one more or one less at the most)")
            esz = 2 if t.f16 else 4
            if not const and off % esz:
                raise ValueError(f"featmix: cut {ci}, track {ti}: byte offset {off} is not aligned to the track's type")
            scaled = c.form == FEATMIX_FOLD and t.snr is not None and not np.isnan(t.snr) and r >= 0 and not (ti == 0 and r == 0)
            if scaled and -float(t.snr) / 10.0 > 308.0:  # (10^(-snr/10) is not finite)
                raise ValueError(f"featmix: cut {ci}, track {ti}: SNR {t.snr} dB out of range")
            if not const and n > 0:
                need = max(need, off + min(nr, n) * F * esz)
            if n > 0 or ti == 0:
                total = max(total, o + n)
            so.append(off), rows.append(nr), frames.append(n), dtype.append(1 if t.f16 else 0), start.append(o)
            snr.append(np.nan if t.snr is None else float(t.snr)), value.append(float(t.value))
        if c.form == FEATMIX_COPY:
            if start[-1] != 0:
                raise ValueError(f"featmix: cut {ci}: the track of the copy form starts at frame 0")
            if total > T:
                raise ValueError(f"featmix: cut {ci}: a track of {total} frames does not fit a cut of {T}")
        elif abs(total - T) > 1 or (T > 0 and total < 1):
            raise ValueError(f"featmix: cut {ci}: the tracks mix to {total} frames, the cut has {T} (one more or one less at the most)")
        first.append(first[-1] + len(trs)), form.append(int(c.form)), frames_c.append(T), pad.append(float(c.pad_value)), dst.append(d0), ref.append(r)
    if need > int(arena_bytes):
        raise ValueError(f"arena too small: {int(arena_bytes)} bytes, the tracks reach to {need}")
    return {
        "h_track_first": _lib.i64(first), "h_form": np.ascontiguousarray(form, dtype=np.int32), "h_num_frames": _lib.i64(frames_c),
        "h_pad_value": np.ascontiguousarray(pad, dtype=np.float64), "h_dst_first": _lib.i64(dst), "h_ref_track": np.ascontiguousarray(ref, dtype=np.int32),
        "h_src_offset": _lib.i64(so), "h_src_rows": _lib.i64(rows), "h_frames": _lib.i64(frames), "h_dtype": np.ascontiguousarray(dtype, dtype=np.int32),
        "h_first": _lib.i64(start), "h_snr_db": np.ascontiguousarray(snr, dtype=np.float64), "h_value": np.ascontiguousarray(value, dtype=np.float64),
        "num_features": F, "row_frames": row_frames, "arena_need": need,
    }


_FEATMIX_ARGS = ("h_track_first", "h_form", "h_num_frames", "h_pad_value", "h_dst_first", "h_ref_track", "h_src_offset", "h_src_rows", "h_frames", "h_dtype",
                 "h_first", "h_snr_db", "h_value")


class HipFeatureMixer(_ArenaHandle):
    """The device half of ``collate_features`` (lhotse/dataset/collation.py:115-145) over ``MixedCut.load_features``
    (lhotse/cut/mixed.py:1199-1309) for the stored tracks of a mini-batch: ``hipfeat_featmix`` (include/hipfeat.h) owns the workspace of
    the two launches -- track energies, then the fold and the padded batch.  One object per device (``get_or_create_featmixer``); it may
    be shared by threads."""

    _KIND = "featmix"  # hipfeat_featmix_create / _destroy

    def plan(self, layout: dict):
        """Host only: ``layout`` as ``featmix_layout`` returns it -> (ticket, info = [ticket, arena bytes needed, energy items, fold items])."""
        info = np.zeros(4, dtype=np.int64)
        with self._lock:
            self.lib.check("hipfeat_featmix_plan", self.handle, len(layout["h_form"]), *(_lib.addr(layout[k]) for k in _FEATMIX_ARGS),
                           int(layout["num_features"]), int(layout["row_frames"]), _lib.addr(info))
        return int(info[0]), info

    def run(self, ticket: int, arena: torch.Tensor, out: torch.Tensor, stream: Optional[int] = None) -> None:
        assert arena.dtype == torch.uint8 and arena.is_contiguous() and arena.ndim == 1 and arena.device == self.device
        assert out.dtype == torch.float32 and out.is_contiguous() and out.device == self.device
        with torch.cuda.device(self.device):
            self.lib.check("hipfeat_featmix_run", self.handle, int(ticket), arena.data_ptr(), arena.numel(), out.data_ptr(), out.numel(),
                           int(_raw_stream(arena.device) if stream is None else stream))


_featmixers: Dict[int, HipFeatureMixer] = {}


def get_or_create_featmixer(device: Union[str, torch.device, None] = None) -> HipFeatureMixer:
    return _get_or_create(_featmixers, HipFeatureMixer, _cache_lock, device)


def featmix_in_arena(arena_bytes: torch.Tensor, cuts_table: Sequence[FeatCut], F: int, row_frames: Optional[int] = None,
                     out: Optional[torch.Tensor] = None, mixer: Optional[HipFeatureMixer] = None,
                     layout: Optional[dict] = None) -> Tuple[torch.Tensor, np.ndarray]:
    """The stored feature tracks of a mini-batch as ONE padded ``(B, row_frames, F)`` float32 tensor: what ``collate_features``
    (lhotse/dataset/collation.py:115-145) returns for cuts with precomputed features, ``CutMix`` / ``.pad`` included
    (``MixedCut.load_features``, lhotse/cut/mixed.py:1199-1309; ``FeatureMixer``, lhotse/features/mixer.py).

    ``arena_bytes`` is ONE uint8 device buffer that holds every track as it was stored (float32 rows at 4-byte, binary16 rows at 2-byte
    boundaries); ``cuts_table`` one ``FeatCut`` per cut.  ``row_frames=None``: the longest cut.  ``out``: a contiguous float32 tensor on
    the arena's device with at least ``B * row_frames * F`` elements that does not overlap the arena.  Returns ``(out (B, row_frames, F),
    num_frames as int32 numpy)``.  Two launches on the current stream, no memset, no device -> host copy, bit-identical from run to run.
    ``layout``: what ``featmix_layout`` returned for this very table, ``F`` and ``row_frames``, for a caller that has it already."""
    assert arena_bytes.dtype == torch.uint8 and arena_bytes.is_contiguous() and arena_bytes.ndim == 1
    if layout is None:
        lay = featmix_layout(arena_bytes.numel(), cuts_table, F, row_frames)  # (before anything is planned)
    else:
        lay = layout
        if lay["arena_need"] > arena_bytes.numel():
            raise ValueError(f"arena too small: {arena_bytes.numel()} bytes, the tracks reach to {lay['arena_need']}")
    B, T, F = len(lay["h_form"]), lay["row_frames"], lay["num_features"]
    if out is not None:
        if out.dtype != torch.float32 or out.device != arena_bytes.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 tensor on {arena_bytes.device}")
        if out.numel() < B * T * F:
            raise ValueError(f"out too small: {out.numel()} elements, {B} rows of {T} x {F} take {B * T * F}")
        a0, o0 = arena_bytes.data_ptr(), out.data_ptr()
        if a0 < o0 + out.numel() * 4 and o0 < a0 + arena_bytes.numel():  # (a plan that is never run would stay outstanding)
            raise ValueError("out overlaps the arena")
        res = out.view(-1)[: B * T * F].view(B, T, F)
    else:
        res = torch.empty((B, T, F), dtype=torch.float32, device=arena_bytes.device)
    lens = lay["h_num_frames"].astype(np.int32)
    if B * T * F == 0:
        return res, lens
    if mixer is None:
        mixer = get_or_create_featmixer(arena_bytes.device)
    ticket, _ = mixer.plan(lay)
    mixer.run(ticket, arena_bytes, res)
    return res, lens
