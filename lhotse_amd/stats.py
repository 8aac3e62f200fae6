"""
Global feature statistics (the estimation half of ``GlobalMVN``) on the HIP path.

* ``HipStatsAccumulator`` -- the surface of ``StatsAccumulator`` (lhotse/features/base.py:990-1033) over ``hipfeat_stats``
  (include/hipfeat.h; csrc/kernel_stats.hpp): ``update`` takes feature matrices that are ALREADY on the device (the packed matrix of
  ``_Plan.run``, the padded batch of ``run_collated`` / ``HipOnTheFlyFeatures`` / ``HipPrecomputedFeatures``), float32 or float16, and
  enqueues two launches; nothing is copied to the host before ``get``.
* ``GlobalStatsPass`` -- the lhotse-free half of a pass over a corpus: batches of waveforms go through the extractor's device path and
  straight into the accumulator, batches of stored matrices are uploaded once.
* ``compute_global_feature_stats`` -- ``CutSet.compute_global_feature_stats`` (lhotse/cut/set.py:2533-2583) with the same arguments
  and the same dict, batched.

There is no CPU fallback.  A cut of 0 frames contributes nothing (the reference's ``np.var`` of an empty matrix turns every bin into NaN).
"""
from __future__ import annotations

import logging
import pickle
import threading
from itertools import islice
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib

__all__ = ["HipStatsAccumulator", "GlobalStatsPass", "compute_global_feature_stats", "get_or_create_stats"]

_DTYPES = {torch.float32: 0, torch.float16: 1}
_DEFAULT_DEVICE = "cuda"  # of a pass that was given neither an extractor nor a device


def _stream(device: torch.device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


class HipStatsAccumulator:
    """``StatsAccumulator`` on the device.  The float64 totals live in HBM; ``total_frames`` is known to the host.  Results are
    bit-identical from run to run and do not depend on how the cuts were grouped into ``update`` calls."""

    def __init__(self, feature_dim: int, device: Union[str, torch.device, None] = "cuda"):
        self.lib = _lib.load()
        self.handle = 0
        self.feature_dim = int(feature_dim)
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise _lib.HipFeatError(_lib.ERR_INVALID, f"HipStatsAccumulator runs on an AMD GPU ('cuda[:i]' device), got device={dev}")
        if not torch.cuda.is_available():
            raise _lib.HipFeatError(_lib.ERR_HIP, "no HIP device is visible (torch.cuda.is_available() is False); there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        out = np.zeros(1, dtype=np.uint64)
        self.lib.check("hipfeat_stats_create", int(self.device.index), self.feature_dim, _lib.addr(out))
        self.handle = int(out[0])

    def close(self):
        if self.handle:
            try:
                self.lib.raw("hipfeat_stats_destroy", self.handle)
            finally:
                self.handle = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- update ---------------------------------------------------------------------------------------------------------------------
    def update(self, features: torch.Tensor, num_frames=None, first_row=None) -> None:
        """``features``: a 2-D ``(T, F)`` device tensor (ONE cut; with ``num_frames``: a packed ``(sum T, F)`` matrix of many cuts), or
        a 3-D padded ``(B, Tmax, F)`` tensor with ``num_frames`` (padding rows are never read).  float32 or float16.  ``first_row``: the
        first row of every cut, counted in rows of the flattened ``(rows, F)`` matrix (default: packed back to back / ``b * Tmax``).
        A view whose rows are further apart than ``F`` elements (``x[:, :F]`` of a wider tensor) is read where it lies."""
        if not isinstance(features, torch.Tensor) or features.device.type != "cuda":
            raise _lib.HipFeatError(_lib.ERR_INVALID, "HipStatsAccumulator runs on an AMD GPU: pass a float32 tensor on a 'cuda' device (there is no CPU fallback)")
        if features.dtype not in _DTYPES:
            raise TypeError(f"HipStatsAccumulator: expected float32 or float16 features, got {features.dtype}")
        if features.ndim not in (2, 3) or features.shape[-1] != self.feature_dim:
            raise ValueError(f"HipStatsAccumulator: expected (T, {self.feature_dim}) or (B, Tmax, {self.feature_dim}) features, got {tuple(features.shape)}")
        x = features
        if x.ndim == 3:
            if num_frames is None:
                raise ValueError("HipStatsAccumulator: a padded (B, Tmax, F) batch needs num_frames")
            B, Tmax, F = x.shape
            if x.numel() and not (x.stride(2) == 1 and x.stride(1) >= F and x.stride(0) == Tmax * x.stride(1)):
                x = x.contiguous()
            stride = int(x.stride(1)) if x.numel() else F
            rows = B * Tmax
            if first_row is None:
                first_row = np.arange(B, dtype=np.int64) * Tmax
        else:
            rows, F = x.shape
            if x.numel() and not (x.stride(1) == 1 and x.stride(0) >= F):
                x = x.contiguous()
            stride = int(x.stride(0)) if rows > 1 else F
            if num_frames is None:
                num_frames = [rows]
        frames = _lib.i64(num_frames.cpu() if isinstance(num_frames, torch.Tensor) else num_frames).reshape(-1)
        first = None if first_row is None else _lib.i64(first_row.cpu() if isinstance(first_row, torch.Tensor) else first_row).reshape(-1)
        if first is not None and len(first) != len(frames):
            raise ValueError("HipStatsAccumulator: one first_row per cut")
        elems = (rows - 1) * stride + F if rows > 0 else 0
        with torch.cuda.device(self.device):
            self.lib.check("hipfeat_stats_update", self.handle, x.data_ptr(), int(elems), _DTYPES[x.dtype], len(frames), _lib.addr(first), _lib.addr(frames),
                           stride, _stream(self.device))

    # -- state ----------------------------------------------------------------------------------------------------------------------
    def state(self) -> Dict[str, object]:
        """-> ``{"total_frames": int, "total_sum": float64 (F,), "total_unnorm_var": float64 (F,)}`` (waits for the stream)."""
        n = np.zeros(1, dtype=np.int64)
        s, v = np.zeros(self.feature_dim, dtype=np.float64), np.zeros(self.feature_dim, dtype=np.float64)
        with torch.cuda.device(self.device):
            self.lib.check("hipfeat_stats_get", self.handle, _lib.addr(n), _lib.addr(s), _lib.addr(v), _stream(self.device))
        return {"total_frames": int(n[0]), "total_sum": s, "total_unnorm_var": v}

    def merge(self, other) -> None:
        """Fold another accumulator (or its ``state()``) in, with the reference's update expression."""
        st = other.state() if hasattr(other, "state") else other
        s = np.ascontiguousarray(st["total_sum"], dtype=np.float64).reshape(-1)
        v = np.ascontiguousarray(st["total_unnorm_var"], dtype=np.float64).reshape(-1)
        if len(s) != self.feature_dim or len(v) != self.feature_dim:
            raise ValueError(f"HipStatsAccumulator.merge: a state of {len(s)} bins into one of {self.feature_dim}")
        with torch.cuda.device(self.device):
            self.lib.check("hipfeat_stats_merge", self.handle, int(st["total_frames"]), _lib.addr(s), _lib.addr(v), _stream(self.device))

    def reset(self) -> None:
        with torch.cuda.device(self.device):
            self.lib.check("hipfeat_stats_reset", self.handle, _stream(self.device))

    @property
    def total_frames(self) -> int:
        return self.state()["total_frames"]

    @property
    def total_sum(self) -> np.ndarray:
        return self.state()["total_sum"]

    @property
    def total_unnorm_var(self) -> np.ndarray:
        return self.state()["total_unnorm_var"]

    @property
    def norm_means(self) -> np.ndarray:
        return self.get()["norm_means"]

    @property
    def norm_stds(self) -> np.ndarray:
        return self.get()["norm_stds"]

    def get(self) -> Dict[str, np.ndarray]:
        st = self.state()
        with np.errstate(divide="ignore", invalid="ignore"):
            return {"norm_means": st["total_sum"] / st["total_frames"], "norm_stds": np.sqrt(st["total_unnorm_var"] / st["total_frames"])}


_accumulators: Dict[tuple, HipStatsAccumulator] = {}
_cache_lock = threading.Lock()


def get_or_create_stats(device: Union[str, torch.device, None], feature_dim: int) -> HipStatsAccumulator:
    """The one accumulator per (device index, feature_dim), kept for the life of the process; ``reset()`` it before a new pass."""
    dev = torch.device("cuda" if device is None else device)
    index = dev.index if dev.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else 0)
    with _cache_lock:
        key = (int(index), int(feature_dim))
        r = _accumulators.get(key)
        if r is None:
            r = _accumulators[key] = HipStatsAccumulator(feature_dim, torch.device(dev.type, index))
        return r


def _is_device_extractor(extractor) -> bool:
    from . import extractors, kaldifeat  # (looked up at the call: the modules may have been reloaded under the real lhotse)

    return isinstance(extractor, (extractors._HipExtractor, kaldifeat._HipKaldifeatExtractor))


class GlobalStatsPass:
    """One pass over a corpus, batch by batch, without a lhotse type in its interface.  ``extractor_or_feature_dim``: one of this
    package's extractors (``add_waveforms``), or the number of bins (``add_features`` only)."""

    def __init__(self, extractor_or_feature_dim, device: Union[str, torch.device, None] = None) -> None:
        if isinstance(extractor_or_feature_dim, (int, np.integer)):
            self.extractor, self.feature_dim = None, int(extractor_or_feature_dim)
        else:
            self.extractor, self.feature_dim = extractor_or_feature_dim, None
            if not _is_device_extractor(self.extractor):
                raise TypeError(f"GlobalStatsPass: {type(self.extractor).__name__} is not one of this package's device extractors")
            if device is None:
                device = self.extractor.device
        self.device = torch.device(_DEFAULT_DEVICE if device is None else device)
        self.accumulator = None
        self._staging: Optional[torch.Tensor] = None  # page-locked where a GPU is there
        self._uploaded = None  # the event behind the upload that read the staging buffer last

    def _acc(self, feature_dim: int):
        if self.accumulator is None:
            self.feature_dim = int(feature_dim)
            self.accumulator = HipStatsAccumulator(self.feature_dim, self.device)
        elif int(feature_dim) != self.feature_dim:
            raise ValueError(f"GlobalStatsPass: features of {feature_dim} bins in a pass over {self.feature_dim}")
        return self.accumulator

    def add_waveforms(self, items: Sequence, sampling_rate: int) -> None:
        """Extract a batch of 1-D waveforms (numpy or torch) on the device, every cut reflected on its own as ``cut.compute_features``
        does, and add the packed device matrix; no feature leaves the device."""
        if self.extractor is None:
            raise ValueError("GlobalStatsPass was created without an extractor")
        ex = self.extractor
        acc = self._acc(ex.feature_dim(sampling_rate))
        if not len(items):
            return
        from . import extractors

        with torch.no_grad():
            if hasattr(ex, "inner"):  # the kaldifeat drop-ins
                assert sampling_rate == ex.config.frame_opts.sampling_rate
                waves = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) if isinstance(x, np.ndarray) else x for x in items]
                packed, frames = ex.inner._extract_items([x.reshape(-1) for x in waves])
                acc.update(ex._post(packed), frames)
            elif type(ex).extract is extractors._HipExtractor.extract:  # the Kaldi-style extractors: one launch for the batch
                ex._check_sr(sampling_rate)
                waves = [extractors._as_1d_float(x.squeeze() if x.ndim > 1 else x, "add_waveforms()") for x in items]
                packed, frames = ex._extract_items(waves)
                acc.update(packed, frames)
            else:  # an extractor with a rule of its own per cut (Whisper's 30 s padding, librosa's centring): its own extract, on the device
                dev = ex.plan.device
                for x in items:
                    t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32) if isinstance(x, np.ndarray) else x).reshape(-1).to(dev)
                    acc.update(ex.extract(t, sampling_rate).to(dev))

    def _stage(self, nbytes: int) -> torch.Tensor:
        if self._uploaded is not None:  # the previous batch's upload has read the buffer
            self._uploaded.synchronize()
            self._uploaded = None
        if self._staging is None or self._staging.numel() < nbytes:
            pin = self.device.type == "cuda" and torch.cuda.is_available()
            self._staging = torch.empty(max(2 * nbytes, 1 << 16), dtype=torch.uint8, pin_memory=pin)
        return self._staging

    def add_features(self, matrices: Sequence[np.ndarray]) -> None:
        """Host ``(T, F)`` matrices, all float32 or all float16 (as a ``hip_archive_f16`` stores them): one upload, one update."""
        mats = [np.ascontiguousarray(m) for m in matrices]
        if not mats:
            return
        dt = mats[0].dtype
        if dt not in (np.float32, np.float16) or any(m.dtype != dt for m in mats):
            raise TypeError("GlobalStatsPass.add_features: float32 or float16 matrices, all of one type")
        F = int(mats[0].shape[1])
        if any(m.ndim != 2 or m.shape[1] != F for m in mats):
            raise ValueError(f"GlobalStatsPass.add_features: every matrix is (T, {F})")
        acc = self._acc(F)
        frames = np.array([m.shape[0] for m in mats], dtype=np.int64)
        rows = int(frames.sum())
        if rows == 0:
            return
        nbytes = rows * F * dt.itemsize
        host = self._stage(nbytes)[:nbytes].numpy().view(dt).reshape(rows, F)
        at = 0
        for m in mats:
            host[at: at + len(m)] = m
            at += len(m)
        with torch.no_grad():
            dev = torch.empty((rows, F), dtype=torch.float32 if dt == np.float32 else torch.float16, device=self.device)
            dev.view(torch.uint8).view(-1).copy_(self._staging[:nbytes], non_blocking=True)
            if self.device.type == "cuda":
                self._uploaded = torch.cuda.Event()
                self._uploaded.record()
            acc.update(dev, frames)

    def result(self) -> Dict[str, np.ndarray]:
        if self.accumulator is None:
            raise ValueError("GlobalStatsPass: nothing was added")
        return self.accumulator.get()


def compute_global_feature_stats(cuts, extractor=None, max_cuts: Optional[int] = None, storage_path=None, batch_duration: float = 600.0) -> Dict[str, np.ndarray]:
    """``cuts.compute_global_feature_stats(storage_path, max_cuts, extractor)`` (lhotse/cut/set.py:2533-2583) on the device.

    With one of this package's extractors the audio is loaded cut by cut, grouped IN CUT ORDER into batches of ``batch_duration``
    seconds and extracted by one launch per batch.  Without an extractor the stored features of the cuts that have some are loaded
    with ``cut.load_features()`` and uploaded batch by batch.  Any other extractor hands the whole call to the reference's method."""
    if extractor is not None and not _is_device_extractor(extractor):
        return cuts.compute_global_feature_stats(storage_path=storage_path, max_cuts=max_cuts, extractor=extractor)
    if extractor is not None:
        selected = cuts
        if max_cuts is not None:
            selected = islice(selected, max_cuts)
        stats = GlobalStatsPass(extractor)
        batch, seconds, rate = [], 0.0, None

        def flush():
            nonlocal batch, seconds
            if batch:
                stats.add_waveforms(batch, rate)
            batch, seconds = [], 0.0

        for cut in selected:
            if rate is not None and cut.sampling_rate != rate:
                flush()
            rate = cut.sampling_rate
            batch.append(np.ascontiguousarray(cut.load_audio(), dtype=np.float32).reshape(-1))
            seconds += float(cut.duration)
            if seconds >= batch_duration:
                flush()
        flush()
    else:
        have_features = [cut.has_features for cut in cuts]
        if not any(have_features):
            raise ValueError("Could not find any features in this CutSet; did you forget to extract them?")
        if not all(have_features):
            logging.warning(f"Computing global stats: only {sum(have_features)}/{len(have_features)} cuts have features.")
        selected = islice((cut for cut in cuts if cut.has_features), max_cuts if max_cuts is not None else len(have_features))
        stats, batch, seconds = None, [], 0.0
        for cut in selected:
            if stats is None:
                stats = GlobalStatsPass(int(cut.num_features))
            # (the cut's own frames; the reference reads cut.features.load(), the whole stored matrix -- the same for an uncut cut)
            batch.append(np.asarray(cut.load_features(), dtype=np.float32))
            seconds += float(cut.duration)
            if seconds >= batch_duration:
                stats.add_features(batch)
                batch, seconds = [], 0.0
        if stats is None:
            raise ValueError("compute_global_feature_stats: max_cuts selects no cut")
        stats.add_features(batch)
    mvn = stats.result()
    if storage_path is not None:
        with open(storage_path, "wb") as f:
            pickle.dump(mvn, f)
    return mvn
