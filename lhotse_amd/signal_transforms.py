"""
Post-feature transforms on the collated ``(B, T, F)`` batch, on the HIP path:

* ``HipGlobalMVN``    -- drop-in for ``GlobalMVN`` (lhotse/dataset/signal_transforms.py:16-60): one fused kernel,
  bit-identical results.
* ``HipSpecAugment``  -- drop-in for ``SpecAugment`` (:121-371): same constructor, ``state_dict`` and ``forward(features,
  supervision_segments)``; the random decisions are made on the host with *the reference's own RNG calls in the
  reference's order* (``random.random``, ``np.random.randint``, ``torch.randint``, ``torch.rand`` on the CPU generator),
  so a seeded run masks and warps exactly the frames the reference would; the whole batch is then processed by two
  kernels (time warp + clone + per-sequence sums; mean fill of the masked regions) instead of ~15 small torch kernels
  per sequence.

* ``HipDereverbWPE``  -- drop-in for ``DereverbWPE`` (:404-447), which works on the raw waveforms: ``torch.stft`` of the whole batch,
  ONE launch of the fused WPE kernel (``wpe_on_device``: one workgroup per cut and frequency bin, float64 on chip), ``torch.istft``
  -- instead of a Python loop over the examples with dozens of complex64 launches each.  With ``lengths=`` (a padded batch and its
  ``audio_lens``) the transforms run on the device too (``wpe_stft_on_device``, ``wpe_istft_on_device``: csrc/kernel_wpe_stft.hpp), each
  row reflected, dereverberated and resynthesised within its own length.

* ``HipRandomizedSmoothing`` -- device twin of ``RandomizedSmoothing`` (:63-118), the one transform that works on the waveform batch
  itself: per-row sigma and mask are drawn on the host (B numbers each) and ONE launch adds the noise and clips (``noise_on_device``:
  csrc/kernel_noise.hpp, Philox4x32-10 and Box-Muller inside the kernel) -- instead of ``randn_like`` and four elementwise passes.
  DIFFERENCE TO THE REFERENCE: the noise is a pure function of ``(seed, row key, sample index)`` and not a draw from torch's generator,
  so under ``torch.manual_seed`` neither the noise nor the per-row sigma and mask repeat the reference's numbers (the reference draws
  B * T normals between its two host draws); the distributions are the same.

All need the batch on the GPU (there is no CPU fallback) and return a new tensor on the same device.
"""
from __future__ import annotations

import bisect
import math
import random
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib

__all__ = ["HipGlobalMVN", "HipSpecAugment", "HipDereverbWPE", "wpe_on_device", "wpe_stft_on_device", "wpe_istft_on_device",
           "HipRandomizedSmoothing", "noise_on_device"]

WPE_MAX_TAPS_TIMES_CHANNELS = 64  # kWpeMaxK of csrc/kernel_wpe.hpp
WPE_TILE_FRAMES = 256  # kWpeMaxTile: frames per time tile of the kernel (it halves, down to 32, only where 256 frames of every channel do not fit)
WPE_STFT_SIZES = (256, 512, 1024, 2048)  # n_fft of csrc/kernel_wpe_stft.hpp; the hop is a quarter or half of it
WPE_ISTFT_TILE_HOPS = 8  # kWpeIstftTileHops: output hops per workgroup of the inverse STFT
_WPE_MODES = {"full": 0, "valid": 1}


def _require_cuda(features: torch.Tensor, who: str) -> torch.Tensor:
    if not isinstance(features, torch.Tensor) or features.device.type != "cuda":
        raise _lib.HipFeatError(_lib.ERR_INVALID, f"{who} runs on an AMD GPU: pass a float32 tensor on a 'cuda' device (there is no CPU fallback)")
    if features.dtype != torch.float32:
        raise TypeError(f"{who}: expected float32 features, got {features.dtype}")
    return features.contiguous()


class HipGlobalMVN(torch.nn.Module):
    """Apply global mean and variance normalization (GlobalMVN, signal_transforms.py:16-60)."""

    def __init__(self, feature_dim: int):
        super().__init__()
        self.feature_dim = feature_dim
        self.register_buffer("norm_means", torch.zeros(feature_dim))
        self.register_buffer("norm_stds", torch.ones(feature_dim))

    @classmethod
    def from_cuts(cls, cuts, max_cuts: Optional[int] = None, extractor=None, device_stats: bool = False) -> "HipGlobalMVN":
        """``device_stats=True``: the statistics are estimated on the device too (``lhotse_amd.compute_global_feature_stats``)."""
        if device_stats:
            from .stats import compute_global_feature_stats

            stats = compute_global_feature_stats(cuts, extractor=extractor, max_cuts=max_cuts)
        else:
            stats = cuts.compute_global_feature_stats(max_cuts=max_cuts, extractor=extractor)
        stats = {name: torch.as_tensor(value) for name, value in stats.items()}
        (feature_dim,) = stats["norm_means"].shape
        mvn = cls(feature_dim)
        mvn.load_state_dict(stats)
        return mvn

    @classmethod
    def from_file(cls, stats_file) -> "HipGlobalMVN":
        stats = torch.load(stats_file)
        (feature_dim,) = stats["norm_means"].shape
        mvn = cls(feature_dim)
        mvn.load_state_dict(stats)
        return mvn

    def to_file(self, stats_file):
        torch.save(self.state_dict(), stats_file)

    def _run(self, features: torch.Tensor, inverse: int) -> torch.Tensor:
        x = _require_cuda(features, "HipGlobalMVN")
        if x.shape[-1] != self.feature_dim:
            raise RuntimeError(f"The size of tensor a ({x.shape[-1]}) must match the size of tensor b ({self.feature_dim}) at non-singleton dimension {x.ndim - 1}")
        means = self.norm_means.to(device=x.device, dtype=torch.float32).contiguous()
        stds = self.norm_stds.to(device=x.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.load().check(
                "hipfeat_global_mvn", x.data_ptr(), out.data_ptr(), means.data_ptr(), stds.data_ptr(), x.numel() // self.feature_dim,
                self.feature_dim, inverse, int(torch.cuda.current_stream(x.device).cuda_stream),
            )
        return out

    def forward(self, features: torch.Tensor, supervision_segments: Optional[torch.IntTensor] = None) -> torch.Tensor:
        return self._run(features, 0)

    def inverse(self, features: torch.Tensor) -> torch.Tensor:
        return self._run(features, 1)


class HipSpecAugment(torch.nn.Module):
    """SpecAugment (time warp, feature masks, frame masks) for a ``(B, T, F)`` batch in two launches."""

    def __init__(
        self,
        time_warp_factor: Optional[int] = 80,
        num_feature_masks: int = 2,
        features_mask_size: int = 27,
        num_frame_masks: int = 10,
        frames_mask_size: int = 100,
        max_frames_mask_fraction: float = 0.15,
        p=0.9,
        fast_rng: bool = False,
    ):
        super().__init__()
        assert 0 <= p <= 1
        assert num_feature_masks >= 0
        assert num_frame_masks >= 0
        assert features_mask_size > 0
        assert frames_mask_size > 0
        self.time_warp_factor = time_warp_factor
        self.num_feature_masks = num_feature_masks
        self.features_mask_size = features_mask_size
        self.num_frame_masks = num_frame_masks
        self.frames_mask_size = frames_mask_size
        self.max_frames_mask_fraction = max_frames_mask_fraction
        self.p = p
        # extension (not part of the reference's state): draw all random numbers of a batch with a few vectorised numpy calls --
        # the same distributions, but NOT the reference's random streams; ~20x less host time per batch (0.8 ms -> 0.04 ms at B = 40)
        self.fast_rng = fast_rng

    def _draw_fast(self, batch: int, num_frames: int, feature_dim: int):
        """Vectorised equivalent of ``draw`` without supervision segments: same distributions as _forward_single (:217-266)."""
        rng = np.random.default_rng(np.random.randint(0, 2**31 - 1))  # follows numpy's global seed
        apply = rng.random(batch) <= self.p
        segs = []
        factor = self.time_warp_factor
        if factor is not None and factor >= 1 and num_frames - factor > factor + 1:
            center = rng.integers(factor + 1, num_frames - factor, size=batch)
            warped = rng.integers(center - factor, center + factor + 1)
            for b in np.nonzero(apply & (warped != center))[0]:
                segs.append((int(b), 0, num_frames, int(center[b]), int(warped[b])))
        masks = []

        def add(axis, size, mask_size, times):
            if times == 0:
                return
            values = rng.integers(0, int(mask_size), size=(batch, times))
            starts = (rng.random((batch, times), dtype=np.float32) * (size - values).astype(np.float32)).astype(np.int64)
            for b in np.nonzero(apply)[0]:
                for a, v in zip(starts[b].tolist(), values[b].tolist()):
                    lo, hi, _ = slice(a, a + v).indices(size)
                    masks.append((int(b), axis, lo, max(lo, hi)))

        add(2, feature_dim, self.features_mask_size, self.num_feature_masks)
        max_tot = self.max_frames_mask_fraction * num_frames
        n_frame_masks = min(self.num_frame_masks, math.ceil(max_tot / self.frames_mask_size))
        add(1, num_frames, min(self.frames_mask_size, max_tot // n_frame_masks), n_frame_masks)
        seg_rounds = [np.array(segs, dtype=_lib.WARP_SEGMENT_DTYPE)] if segs else []
        return seg_rounds, np.array(masks, dtype=_lib.MASK_DTYPE)

    # -- the reference's random decisions, call for call -------------------------------------------------------------
    def _draw_warp(self, t: int) -> Optional[Tuple[int, int]]:
        """time_warp (signal_transforms.py:338-353): the (center, warped) pair, or None when nothing is warped."""
        factor = self.time_warp_factor
        if factor is None or factor < 1:
            return None
        if t - factor <= factor + 1:
            return None
        center = np.random.randint(factor + 1, t - factor)
        warped = np.random.randint(center - factor, center + factor + 1)
        if warped == center:
            return None
        return int(center), int(warped)

    @staticmethod
    def _draw_masks(size: int, mask_size, mask_times: int) -> List[Tuple[int, int]]:
        """mask_along_axis_optimized (:297-335): [begin, end) of every mask along an axis of ``size`` entries."""
        values = torch.randint(int(0), int(mask_size), (1, mask_times)).numpy().reshape(-1)
        # torch.rand(1, n) * (size - values): float32 times int64 -> float32; .long() truncates.  Same arithmetic in numpy
        # (the generator calls above and below are what must stay torch's; the rest is host time, 60 sequences per batch)
        min_values = torch.rand(1, mask_times).numpy().reshape(-1) * (size - values).astype(np.float32)
        starts = min_values.astype(np.int64)
        # a mask wider than the axis (features_mask_size > F) makes `size - values` and hence the start negative; the
        # reference then slices with it (features[:, :, start:end], :316-332), so Python's slice rules decide the region
        out = []
        for a, b in zip(starts.tolist(), (starts + values).tolist()):
            lo, hi, _ = slice(a, b).indices(size)
            out.append((lo, max(lo, hi)))
        return out

    def _draw_single(self, t: int, f: int, warp: bool, mask: bool):
        """_forward_single (:217-266) for a (t, f) matrix -> ((center, warped) | None, [(axis, begin, end)])."""
        if random.random() > self.p:
            return None, []
        seg = self._draw_warp(t) if warp else None
        masks: List[Tuple[int, int, int]] = []
        if mask:
            masks += [(2, a, b) for a, b in self._draw_masks(f, self.features_mask_size, self.num_feature_masks)]
            max_tot_mask_frames = self.max_frames_mask_fraction * t
            num_frame_masks = min(self.num_frame_masks, math.ceil(max_tot_mask_frames / self.frames_mask_size))
            max_mask_frames = min(self.frames_mask_size, max_tot_mask_frames // num_frame_masks)
            masks += [(1, a, b) for a, b in self._draw_masks(t, max_mask_frames, num_frame_masks)]
        return seg, masks

    def draw(self, batch: int, num_frames: int, feature_dim: int, supervision_segments=None):
        """All random decisions of one ``forward`` call -> (rounds of warp segments, masks) as numpy records.  Warp
        segments of one sequence that overlap go to successive rounds (the reference applies them one after another)."""
        segs: List[Tuple[int, int, int, int, int]] = []
        masks: List[Tuple[int, int, int, int]] = []
        if supervision_segments is None:
            for b in range(batch):
                seg, ms = self._draw_single(num_frames, feature_dim, True, True)
                if seg is not None:
                    segs.append((b, 0, num_frames, seg[0], seg[1]))
                masks += [(b, ax, lo, hi) for ax, lo, hi in ms]
        else:
            rows = supervision_segments.tolist() if hasattr(supervision_segments, "tolist") else list(supervision_segments)
            for b, start, n in rows:
                b, start, n = int(b), int(start), int(n)
                lo, hi = self._slice_bounds(start, start + n, num_frames)
                seg, _ = self._draw_single(max(0, hi - lo), feature_dim, True, False)
                if seg is not None:
                    segs.append((b if b >= 0 else b + batch, lo, hi - lo, seg[0], seg[1]))
            for b in range(batch):
                _, ms = self._draw_single(num_frames, feature_dim, False, True)
                masks += [(b, ax, lo, hi) for ax, lo, hi in ms]
        rounds: List[List[Tuple[int, int, int, int, int]]] = []
        placed: List[Tuple[int, Tuple[int, int, int, int, int]]] = []
        for s in segs:
            r = 0
            for pr, q in placed:
                if q[0] == s[0] and q[1] < s[1] + s[2] and s[1] < q[1] + q[2]:
                    r = max(r, pr + 1)
            placed.append((r, s))
            while len(rounds) <= r:
                rounds.append([])
            rounds[r].append(s)
        seg_rounds = [np.array(r, dtype=_lib.WARP_SEGMENT_DTYPE) for r in rounds]
        return seg_rounds, np.array(masks, dtype=_lib.MASK_DTYPE)

    @staticmethod
    def _slice_bounds(start: int, end: int, size: int) -> Tuple[int, int]:
        lo, hi, _ = slice(start, end).indices(size)  # what features[b, start:end] selects
        return lo, max(lo, hi)

    def forward(self, features: torch.Tensor, supervision_segments: Optional[torch.IntTensor] = None, *args, **kwargs) -> torch.Tensor:
        assert len(features.shape) == 3, "SpecAugment only supports batches of single-channel feature matrices."
        x = _require_cuda(features, "HipSpecAugment")
        B, T, F = x.shape
        if self.fast_rng and supervision_segments is None:
            seg_rounds, masks = self._draw_fast(B, T, F)
        else:
            seg_rounds, masks = self.draw(B, T, F, supervision_segments)
        return apply_specaug(x, seg_rounds, masks)

    def state_dict(self, **kwargs) -> Dict[str, Any]:
        return dict(
            time_warp_factor=self.time_warp_factor,
            num_feature_masks=self.num_feature_masks,
            features_mask_size=self.features_mask_size,
            num_frame_masks=self.num_frame_masks,
            frames_mask_size=self.frames_mask_size,
            max_frames_mask_fraction=self.max_frames_mask_fraction,
            p=self.p,
        )

    def load_state_dict(self, state_dict: Dict[str, Any]):
        for k in ("time_warp_factor", "num_feature_masks", "features_mask_size", "num_frame_masks", "frames_mask_size", "max_frames_mask_fraction", "p"):
            setattr(self, k, state_dict.get(k, getattr(self, k)))


def apply_specaug(x: torch.Tensor, seg_rounds: List[np.ndarray], masks: np.ndarray) -> torch.Tensor:
    """Run ``hipfeat_specaug`` on a contiguous float32 ``(B, T, F)`` device tensor: one call per round of
    non-overlapping warp segments (almost always one), the masks in the last."""
    lib = _lib.load()
    B, T, F = x.shape
    rounds = list(seg_rounds) if len(seg_rounds) else [np.zeros(0, dtype=_lib.WARP_SEGMENT_DTYPE)]
    with torch.cuda.device(x.device):
        stream = int(torch.cuda.current_stream(x.device).cuda_stream)
        for i, segs in enumerate(rounds):
            last = i == len(rounds) - 1
            m = masks if last else masks[:0]
            segs = np.ascontiguousarray(segs)
            m = np.ascontiguousarray(m)
            out = torch.empty_like(x)
            lib.check("hipfeat_specaug", x.data_ptr(), out.data_ptr(), B, T, F, _lib.addr(segs) if len(segs) else None, len(segs),
                      _lib.addr(m) if len(m) else None, len(m), stream)
            x = out
    return x


def wpe_on_device(Y: torch.Tensor, taps: int = 10, delay: int = 3, iterations: int = 3, statistics_mode: str = "full", *,
                  channels: Optional[int] = None, out: Optional[torch.Tensor] = None, frames: Optional[torch.Tensor] = None) -> torch.Tensor:
    """WPE dereverberation (nara_wpe's ``wpe_v6`` with ``psd_context=0``; the algorithm is stated in csrc/kernel_wpe.hpp) of a batch of
    STFTs in one launch.  ``Y``: complex64 on the device, ``(B, D, F, T)``, or ``(B * D, F, T)`` with ``channels=D`` (what
    ``torch.stft`` returns for ``(B * D, samples)`` input; read in place whatever its strides).  The D channels of a cut are
    dereverberated jointly.  Returns a tensor of Y's shape (``out``, if given: any strides, no overlap with Y).  A bin whose
    correlation matrix has no Cholesky factor (a silent bin, "valid" statistics without a frame) comes back unchanged.
    ``frames``: integer ``(B,)``, CPU or device -- only the first ``frames[b]`` frames of example b exist: its result is what the example
    gives alone, bit for bit (as long as both calls run the same time tile, ``WPE_TILE_FRAMES`` unless the longest row's working set
    forces a smaller one), and the output frames behind them are 0.  A table on the CPU is checked against ``0 ... T``; one on the
    device is not read back, the kernel clamps it."""
    if not isinstance(Y, torch.Tensor) or Y.device.type != "cuda":
        raise _lib.HipFeatError(_lib.ERR_INVALID, "wpe_on_device runs on an AMD GPU: pass a complex64 tensor on a 'cuda' device (there is no CPU fallback)")
    if Y.dtype != torch.complex64:
        raise TypeError(f"wpe_on_device: expected a complex64 STFT, got {Y.dtype}")
    if statistics_mode not in _WPE_MODES:
        raise ValueError(f"wpe_on_device: statistics_mode is 'full' or 'valid', got {statistics_mode!r}")
    if Y.ndim == 4 and channels is None:
        shape, D = Y.shape, Y.shape[1]
        rows = Y.reshape(-1, *Y.shape[2:])  # a view wherever the two leading strides allow one
    elif Y.ndim == 3 and channels is not None and channels >= 1 and Y.shape[0] % channels == 0:
        shape, D, rows = Y.shape, int(channels), Y
    else:
        raise ValueError("wpe_on_device: pass (B, D, F, T), or (B * D, F, T) with channels=D")
    taps, delay, iterations = int(taps), int(delay), int(iterations)
    if taps < 1 or delay < 0 or iterations < 1:
        raise ValueError(f"wpe_on_device: taps >= 1, delay >= 0 and iterations >= 1 are required, got {taps}, {delay}, {iterations}")
    if taps * D > WPE_MAX_TAPS_TIMES_CHANNELS:
        raise NotImplementedError(f"wpe_on_device: taps * channels = {taps * D} exceeds the kernel's limit of {WPE_MAX_TAPS_TIMES_CHANNELS}")
    if out is None:
        out = torch.empty(rows.shape, dtype=torch.complex64, device=Y.device)
    elif out.shape != shape or out.dtype != torch.complex64 or out.device != Y.device:
        raise ValueError("wpe_on_device: `out` must have Y's shape, dtype and device")
    out_rows = out if out.ndim == 3 else out.view(-1, *out.shape[2:])

    def span(t):  # [first, last] byte address a strided tensor touches
        lo = t.data_ptr() + 8 * sum(min(0, (n - 1) * st) for n, st in zip(t.shape, t.stride()))
        return lo, lo + 8 * sum(abs((n - 1) * st) for n, st in zip(t.shape, t.stride())) + 7

    if rows.numel() and span(rows)[0] <= span(out_rows)[1] and span(out_rows)[0] <= span(rows)[1]:
        raise ValueError("wpe_on_device: `out` must not overlap Y in memory (the kernel re-reads Y after it has written earlier frames)")
    N, F, T = rows.shape
    args = (rows.data_ptr(), out_rows.data_ptr(), N // D, D, F, T, *rows.stride(), *out_rows.stride(), taps, delay, iterations, _WPE_MODES[statistics_mode])
    if frames is None:
        _wpe_call(Y.device, "hipfeat_wpe_run", *args)
    else:
        counts = _wpe_counts("wpe_on_device", "frames", frames, N // D, 0, T, Y.device, need_host=False)[1]
        _wpe_call(Y.device, "hipfeat_wpe_run_ragged", *args, counts.data_ptr())
    return out.view(shape)


def _wpe_call(device, name: str, *args) -> None:
    with torch.cuda.device(device):
        try:
            _lib.load().check(name, *args, int(torch.cuda.current_stream(device).cuda_stream))
        except _lib.HipFeatError as e:
            if e.status == _lib.ERR_UNSUPPORTED:
                raise NotImplementedError(str(e)) from e
            raise


def _wpe_sizes(who: str, n_fft: int, hop_length: int) -> Tuple[int, int]:
    n_fft, hop = int(n_fft), int(hop_length)
    if n_fft not in WPE_STFT_SIZES or hop not in (n_fft // 4, n_fft // 2):
        raise NotImplementedError(f"{who}: n_fft is one of {WPE_STFT_SIZES} and hop_length a quarter or half of it, got {n_fft} and {hop}")
    return n_fft, hop


def _wpe_counts(who: str, what: str, counts: torch.Tensor, batch: int, low: int, high: int, device, need_host: bool = True):
    """A per-example table of lengths or frame counts -> (its values on the host, itself as int32 on the device).  The values are checked
    against ``low ... high`` here, before anything is launched.  ``need_host=False``: a table on the device is taken as it is (no
    synchronisation; the kernel clamps it to the buffer) and the host values are None."""
    if not isinstance(counts, torch.Tensor) or counts.is_floating_point() or counts.is_complex() or counts.dtype == torch.bool or counts.shape != (batch,):
        raise ValueError(f"{who}: `{what}` is an integer tensor of shape ({batch},), one entry per example")
    host = None
    if need_host or counts.device.type == "cpu":
        host = counts.tolist()
        for b, n in enumerate(host):
            if not low <= n <= high:
                raise ValueError(f"{who}: {what}[{b}] = {n} lies outside {low} ... {high}" + (
                    " (a row must be longer than n_fft // 2 samples to be reflected, and no longer than the tensor)" if what == "lengths" else ""))
    return host, counts.to(device=device, dtype=torch.int32).contiguous()


def _wpe_stft(audio: torch.Tensor, lengths: torch.Tensor, frames_max: int, n_fft: int, hop: int, window: torch.Tensor, bin_major: bool = True):
    """(B, D, T) float32 with unit sample stride, int32 lengths on the device -> (Y (B * D, F, frames_max), frames).  ``bin_major``: Y is
    (F, frames)-contiguous per row; otherwise (frames, F)-contiguous, torch.stft's own layout."""
    B, D, T = audio.shape
    F = n_fft // 2 + 1
    if bin_major:
        Y = torch.empty((B * D, F, frames_max), dtype=torch.complex64, device=audio.device)
    else:
        Y = torch.empty((B * D, frames_max, F), dtype=torch.complex64, device=audio.device).transpose(1, 2)
    frames = torch.empty(B, dtype=torch.int32, device=audio.device)
    _wpe_call(audio.device, "hipfeat_wpe_stft_run", audio.data_ptr(), B, D, audio.stride(0), audio.stride(1), T, lengths.data_ptr(), window.data_ptr(), n_fft,
              hop, Y.data_ptr(), *Y.stride(), frames_max, frames.data_ptr())
    return Y, frames


def _wpe_istft(Z: torch.Tensor, frames: torch.Tensor, D: int, n_fft: int, hop: int, window: torch.Tensor, out_samples: int,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B * D, F, T) complex64 of any strides, int32 frame counts on the device -> (B * D, out_samples) float32, +0.0 behind each row's end
    (``out``: a float32 tensor of that shape, unit sample stride, row stride uniform across examples)."""
    N, _, T = Z.shape
    z = torch.empty((N, out_samples), dtype=torch.float32, device=Z.device) if out is None else out
    _wpe_call(Z.device, "hipfeat_wpe_istft_run", Z.data_ptr(), N // D, D, *Z.stride(), T, frames.data_ptr(), window.data_ptr(), n_fft, hop, z.data_ptr(),
              D * z.stride(0), z.stride(0), out_samples)
    return z


def _wpe_audio(who: str, audio: torch.Tensor) -> torch.Tensor:
    if not isinstance(audio, torch.Tensor) or audio.device.type != "cuda":
        raise _lib.HipFeatError(_lib.ERR_INVALID, f"{who} runs on an AMD GPU: pass a float32 tensor on a 'cuda' device (there is no CPU fallback)")
    if audio.dtype != torch.float32:
        raise TypeError(f"{who}: expected float32 audio, got {audio.dtype}")
    if audio.ndim not in (2, 3):
        raise ValueError(f"{who} expects (B, T) or (B, D, T) audio")
    audio = audio if audio.ndim == 3 else audio[:, None]
    return audio if audio.stride(-1) == 1 else audio.contiguous()


def wpe_stft_on_device(audio: torch.Tensor, lengths: torch.Tensor, n_fft: int = 512, hop_length: int = 128) -> Tuple[torch.Tensor, torch.Tensor]:
    """Centred STFT of a padded batch with a length per row, for the WPE kernel: row ``b`` is ``audio[b, ..., :lengths[b]]`` and nothing
    behind it is read.  ``audio``: float32 ``(B, T)`` or ``(B, D, T)`` on the device (any row and channel stride); ``lengths``: integer
    ``(B,)``, CPU or device.  Returns ``(Y, frames)``: ``frames[b] = 1 + lengths[b] // hop_length`` (int32, on the device) and ``Y``,
    complex64 ``(B * D, n_fft // 2 + 1, max frames)``, what ``torch.stft(row, n_fft, hop_length, window=blackman_window(n_fft),
    return_complex=True)`` gives for each row alone, with zeros at and behind ``frames[b]``.  Memory layout: contiguous, each bin's
    frames side by side -- what the WPE kernel, one workgroup per bin, reads along time.  ``n_fft`` is 256, 512, 1024 or 2048 and
    ``hop_length`` a quarter or half of it; anything else raises NotImplementedError.  A row with ``lengths[b] <= n_fft // 2`` (torch's
    reflect padding refuses it too) or ``> T`` raises ValueError before anything is launched."""
    a3 = _wpe_audio("wpe_stft_on_device", audio)
    n_fft, hop = _wpe_sizes("wpe_stft_on_device", n_fft, hop_length)
    host, lens = _wpe_counts("wpe_stft_on_device", "lengths", lengths, a3.shape[0], n_fft // 2 + 1, a3.shape[-1], a3.device)
    return _wpe_stft(a3, lens, 1 + max(host, default=-hop) // hop, n_fft, hop, torch.blackman_window(n_fft, device=a3.device))


def wpe_istft_on_device(Z: torch.Tensor, frames: torch.Tensor, n_fft: int = 512, hop_length: int = 128, *,
                        channels: Optional[int] = None, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Inverse of ``wpe_stft_on_device``: ``Z`` complex64 on the device, ``(B, D, F, T)``, or ``(B * D, F, T)`` with ``channels=D``
    (default 1), read in place whatever its strides; ``frames``: integer ``(B,)``, only the first ``frames[b]`` frames of example b
    exist.  Returns ``(z, z_lens)``: ``z`` float32 ``(B, D, n)`` or ``(B * D, n)``, ``n = max z_lens``, row b what ``torch.istft`` gives
    for its own frames (periodic Blackman window) and +0.0 behind ``z_lens[b] = hop_length * (frames[b] - 1)``, all written by the one
    launch (into ``out``, if given: float32 of z's shape, unit sample stride); ``z_lens`` is int64 where ``frames`` lives.  Same sizes as ``wpe_stft_on_device``, NotImplementedError otherwise."""
    if not isinstance(Z, torch.Tensor) or Z.device.type != "cuda":
        raise _lib.HipFeatError(_lib.ERR_INVALID, "wpe_istft_on_device runs on an AMD GPU: pass a complex64 tensor on a 'cuda' device (there is no CPU fallback)")
    n_fft, hop = _wpe_sizes("wpe_istft_on_device", n_fft, hop_length)
    D = Z.shape[1] if Z.ndim == 4 and channels is None else int(channels or 1)
    if Z.dtype != torch.complex64 or Z.ndim not in (3, 4) or Z.shape[-2] != n_fft // 2 + 1 or (Z.ndim == 3 and (D < 1 or Z.shape[0] % D)):
        raise ValueError(f"wpe_istft_on_device: pass complex64 (B, D, {n_fft // 2 + 1}, T), or (B * D, {n_fft // 2 + 1}, T) with channels=D")
    rows = Z if Z.ndim == 3 else Z.reshape(-1, *Z.shape[2:])
    host, counts = _wpe_counts("wpe_istft_on_device", "frames", frames, rows.shape[0] // D, 0, Z.shape[-1], Z.device)
    z_lens = [hop * max(n - 1, 0) for n in host]
    n = max(z_lens, default=0)
    if out is not None:
        flat = out if out.ndim == 2 else out.flatten(0, 1)
        if (out.shape != (*Z.shape[:-2], n) or out.dtype != torch.float32 or out.device != Z.device or (n > 1 and out.stride(-1) != 1)
                or flat.data_ptr() != out.data_ptr()):
            raise ValueError(f"wpe_istft_on_device: `out` is float32 {(*Z.shape[:-2], n)} on Z's device with unit sample stride and one row stride")
        _wpe_istft(rows, counts, D, n_fft, hop, torch.blackman_window(n_fft, device=Z.device), n, flat)
        return out, torch.tensor(z_lens, dtype=torch.int64, device=frames.device)
    z = _wpe_istft(rows, counts, D, n_fft, hop, torch.blackman_window(n_fft, device=Z.device), n)
    return (z if Z.ndim == 3 else z.view(*Z.shape[:2], -1)), torch.tensor(z_lens, dtype=torch.int64, device=frames.device)


class HipDereverbWPE(torch.nn.Module):
    """Dereverberation with Weighted Prediction Error (DereverbWPE, signal_transforms.py:404-447): ``(B, T)`` audio is a batch of mono
    rows, each dereverberated on its own; ``(B, D, T)`` is a batch of D-channel examples, the channels of one example jointly.  The
    keyword-only extras are the arguments the reference leaves at nara_wpe's defaults."""

    def __init__(self, n_fft: int = 512, hop_length: int = 128, *, taps: int = 10, delay: int = 3, iterations: int = 3, statistics_mode: str = "full"):
        super().__init__()
        self.n_fft = n_fft
        self.hop_length = hop_length
        self.taps, self.delay, self.iterations, self.statistics_mode = taps, delay, iterations, statistics_mode

    def forward(self, audio: torch.Tensor, *args, lengths: Optional[torch.Tensor] = None, **kwargs):
        """``lengths=None``: the whole ``(B, [D,] T)`` tensor is dereverberated, padding included, as the reference does; returns ``z``.
        ``lengths``: integer ``(B,)``, CPU or device -- row b is ``audio[b, ..., :lengths[b]]`` and nothing behind it is read; returns
        ``(z, z_lens)``, row b what the module gives for that cut alone, ``z_lens[b] = hop_length * (lengths[b] // hop_length)`` samples
        (an integer tensor where ``lengths`` lives) and +0.0 behind them.  Three launches (``wpe_stft_on_device``, ``wpe_on_device``,
        ``wpe_istft_on_device``; their sizes and refusals apply), no torch.stft / torch.istft."""
        if lengths is not None:
            a3 = _wpe_audio("HipDereverbWPE", audio)
            n_fft, hop = _wpe_sizes("HipDereverbWPE", self.n_fft, self.hop_length)
            host, lens = _wpe_counts("HipDereverbWPE", "lengths", lengths, a3.shape[0], n_fft // 2 + 1, a3.shape[-1], a3.device)
            frames_max = 1 + max(host, default=-hop) // hop
            window = torch.blackman_window(n_fft, device=a3.device)
            Y, frames = _wpe_stft(a3, lens, frames_max, n_fft, hop, window)
            Z = wpe_on_device(Y, self.taps, self.delay, self.iterations, self.statistics_mode, channels=a3.shape[1], frames=frames)
            z = _wpe_istft(Z, frames, a3.shape[1], n_fft, hop, window, hop * max(frames_max - 1, 0))
            return z.view(*audio.shape[:-1], -1), (lengths // hop) * hop
        if not isinstance(audio, torch.Tensor) or audio.device.type != "cuda":
            raise _lib.HipFeatError(_lib.ERR_INVALID, "HipDereverbWPE runs on an AMD GPU: pass a float32 tensor on a 'cuda' device (there is no CPU fallback)")
        if audio.dtype != torch.float32:
            raise TypeError(f"HipDereverbWPE: expected float32 audio, got {audio.dtype}")
        assert audio.ndim in (2, 3), "HipDereverbWPE expects (B, T) or (B, D, T) audio"
        D = 1 if audio.ndim == 2 else audio.shape[1]
        # dereverb_wpe_torch (lhotse/augmentation/wpe.py:111-129): periodic Blackman window, centred frames
        window = torch.blackman_window(self.n_fft, device=audio.device)
        Y = torch.stft(audio.reshape(-1, audio.shape[-1]), n_fft=self.n_fft, hop_length=self.hop_length, return_complex=True, window=window)
        Z = wpe_on_device(Y, self.taps, self.delay, self.iterations, self.statistics_mode, channels=D)
        z = torch.istft(Z, n_fft=self.n_fft, hop_length=self.hop_length, window=window)
        return z.reshape(*audio.shape[:-1], z.shape[-1])


_NOISE_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}  # hipfeat_noise_dtype


def _noise_table(what: str, values, rows: int, dtype: torch.dtype, device) -> torch.Tensor:
    """A float, or one entry per row as a sequence or tensor -> a contiguous ``(rows,)`` table on the device (one small copy at the most)."""
    t = torch.as_tensor(values)
    if t.ndim == 0:
        t = t.expand(rows)
    if t.shape != (rows,) or (not dtype.is_floating_point and (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool)):
        raise ValueError(f"noise_on_device: `{what}` has one {'number' if dtype.is_floating_point else 'integer'} per row, shape ({rows},)")
    return t.to(device=device, dtype=dtype).contiguous()


def noise_on_device(x: torch.Tensor, sigma, *, seed: int, row_keys=None, lengths=None, clip: Optional[Tuple[float, float]] = (-1.0, 1.0),
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[b, t] = clip(x[b, t] + a[b, t] * n(seed, key_b, t))`` with ``a[b, t] = sigma[b]`` in front of ``lengths[b]`` and 0 behind, in one
    launch (the generator and the map to normals are stated in csrc/kernel_noise.hpp and include/hipfeat.h).  ``x``: ``(B, T)`` or
    ``(T,)`` on the device, float32, float16 or bfloat16, any row stride, unit sample stride.  ``sigma``: a float, or one per row
    (sequence or tensor).  ``seed``: an integer, its low 64 bits count.  ``row_keys``: one int64 per row (default: the row index) -- a
    row's noise depends on its key and not on its place in the batch, so a cut keyed by a hash of its id gets the same noise wherever
    it lands.  ``lengths``: integers, one per row, CPU or device; the samples at and behind them are only clipped.  ``clip=None``: no
    clip.  Returns a new tensor, or ``out`` (x's shape and dtype, unit sample stride; ``out=x`` works in place, any other overlap
    with x is an error of the caller).  A sample with amplitude 0 is ``clip(x)`` bit for bit."""
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise _lib.HipFeatError(_lib.ERR_INVALID, "noise_on_device runs on an AMD GPU: pass a float32, float16 or bfloat16 tensor on a 'cuda' device (there is no CPU fallback)")
    if x.dtype not in _NOISE_DTYPES:
        raise TypeError(f"noise_on_device: expected float32, float16 or bfloat16 samples, got {x.dtype}")
    if x.ndim not in (1, 2):
        raise ValueError("noise_on_device expects (B, T) or (T,) samples")
    lo, hi = (-math.inf, math.inf) if clip is None else (float(clip[0]), float(clip[1]))
    if not lo <= hi:
        raise ValueError(f"noise_on_device: clip=(lo, hi) needs lo <= hi, got {clip}")
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    elif not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
        raise ValueError("noise_on_device: `out` must have x's shape, dtype and device")
    B, T = (1, x.shape[0]) if x.ndim == 1 else x.shape

    def row_stride(t: torch.Tensor, who: str) -> int:
        if T > 1 and t.stride(-1) != 1:
            raise ValueError(f"noise_on_device: {who} needs unit stride along the samples")
        stride = T if B == 1 or t.ndim == 1 else t.stride(0)
        if stride < T:
            raise ValueError(f"noise_on_device: the rows of {who} overlap (row stride {stride} < {T} samples)")
        return stride

    if x is not out and x.ndim == 2 and B > 1 and 0 <= x.stride(0) < T and (T == 1 or x.stride(1) == 1):
        x = x.contiguous()  # rows that repeat or overlap (an expanded row) are legal to read
    strides = row_stride(x, "x"), row_stride(out, "`out`")
    table = _noise_table("sigma", sigma, B, torch.float32, x.device)
    keys = None if row_keys is None else _noise_table("row_keys", row_keys, B, torch.int64, x.device)
    lens = None if lengths is None else _noise_table("lengths", lengths, B, torch.int64, x.device)
    seed = int(seed) & (2**64 - 1)
    _wpe_call(x.device, "hipfeat_noise_run", x.data_ptr(), out.data_ptr(), B, T, *strides, _NOISE_DTYPES[x.dtype], table.data_ptr(),
              None if keys is None else keys.data_ptr(), None if lens is None else lens.data_ptr(), seed - 2**64 if seed >= 2**63 else seed, lo, hi)
    return out


def schedule_value_for_step(schedule, step: int):
    """The value of a ``[(first step, value), ...]`` schedule at ``step`` (signal_transforms.py:374-382)."""
    milestones, values = zip(*schedule)
    assert milestones[0] <= step, f"Cannot determine the scheduled value for step {step} with schedule: {schedule}. Did you forget to add the first part of the schedule for steps below {milestones[0]}?"
    return values[bisect.bisect_right(milestones, step) - 1]


def _mix64(a: int, b: int) -> int:
    """splitmix64's finaliser over a + b * golden ratio: the launch seed of call b of a module seeded with a."""
    z = (a + (b + 1) * 0x9E3779B97F4A7C15) & (2**64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    return z ^ (z >> 31)


class HipRandomizedSmoothing(torch.nn.Module):
    """Randomized smoothing (RandomizedSmoothing, signal_transforms.py:63-118): Gaussian noise added to a batch of waveforms, the sum
    clipped to [-1, 1].  ``sigma`` (a float, or a ``[(step, value)]`` schedule read at ``step``, which advances per call as the
    reference's does: under a schedule only), ``sample_sigma`` (a factor ``2 u - 1`` per row) and ``p`` (the probability that a row gets
    noise at all) are the reference's; the two per-row draws come from torch's generator on the host, B numbers each, and fold into one
    sigma table: a masked row gets 0.  The table goes up in one small copy and ``noise_on_device`` does the rest in one launch.
    ``seed``: the noise itself is Philox's (see the module docstring for the difference to the reference); call i of a module uses a
    launch seed mixed from ``seed`` and i, so successive calls differ and a module built again with the same seed replays them;
    ``seed=None`` draws one from torch's generator per call.  ``row_keys`` / ``lengths``: as for ``noise_on_device``.  Audio is
    ``(B, T)`` or ``(B, C, T)`` (the channels of an example share its sigma, its mask and its length; their noise differs)."""

    def __init__(self, sigma=0.1, sample_sigma: bool = True, p: float = 0.3, seed: Optional[int] = None):
        super().__init__()
        self.sigma = sigma
        self.sample_sigma = sample_sigma
        self.p = p
        self.seed = seed
        self.step = 0
        self.calls = 0

    def forward(self, audio: torch.Tensor, *args, lengths=None, row_keys=None, **kwargs) -> torch.Tensor:
        if not isinstance(audio, torch.Tensor) or audio.device.type != "cuda":
            raise _lib.HipFeatError(_lib.ERR_INVALID, "HipRandomizedSmoothing runs on an AMD GPU: pass a float32, float16 or bfloat16 tensor on a 'cuda' device (there is no CPU fallback)")
        if audio.ndim not in (2, 3):
            raise ValueError("HipRandomizedSmoothing expects (B, T) or (B, C, T) audio")
        if isinstance(self.sigma, (int, float)):
            sigma = self.sigma
        else:
            sigma = schedule_value_for_step(self.sigma, self.step)
            self.step += 1
        B = audio.shape[0]
        table = torch.full((B,), float(sigma))
        if self.sample_sigma:
            table = table * (2 * torch.rand(B) - 1)
        table = table * (torch.rand(B) > 1.0 - self.p)  # random_mask_along_batch_axis(p=1 - self.p): a row keeps its noise with probability p
        seed = int(torch.randint(0, 2**62, ()).item()) if self.seed is None else int(self.seed)
        seed, self.calls = _mix64(seed, self.calls), self.calls + 1
        if audio.ndim == 2:
            return noise_on_device(audio, table, seed=seed, row_keys=row_keys, lengths=lengths)
        C = audio.shape[1]
        per_row = lambda t: None if t is None else torch.as_tensor(t).repeat_interleave(C)  # noqa: E731
        keys = torch.as_tensor(row_keys).repeat_interleave(C) * C + torch.arange(C).repeat(B) if row_keys is not None else None
        return noise_on_device(audio.flatten(0, 1), per_row(table), seed=seed, row_keys=keys, lengths=per_row(lengths)).view(audio.shape)
