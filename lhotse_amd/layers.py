"""
The Kaldi feature *layers* on the HIP path: ``HipWav2Spec``, ``HipWav2LogSpec``, ``HipWav2LogFilterBank``, ``HipWav2MFCC``.

Drop-ins for the ``torch.nn.Module``s of lhotse/features/kaldi/layers.py (``Wav2Spec`` :336-402, ``Wav2LogSpec`` :405-473,
``Wav2LogFilterBank`` :476-578, ``Wav2MFCC`` :581-724) where they are used for inference: same constructor arguments and
defaults (in the same order), same attributes, ``forward(x)`` maps a ``(B, T)`` (or ``(T,)``) float32 batch of equally long
waveforms on the GPU to ``(B, num_frames, F)`` on the same device -- one fused launch instead of the ~12 tensor ops of
``Wav2Win`` + ``_rfft`` + matmul + log.  Not covered, by design: TorchScript.

Autograd is opt-in: ``layer.differentiable_()`` (all six classes; ``differentiable_(False)`` switches it off, ``layer.differentiable``
reads it) makes ``forward`` backpropagate to the waveform, which is the only gradient the reference layers have (every parameter of
theirs is ``requires_grad=False``).  The forward is the same launch and the same bits; the backward is ``hipfeat_grad_run``
(csrc/kernel_grad.hpp: per frame the recomputed forward, the seeded spectrum cotangent, the adjoint FFT and front end into a workspace,
then a gather without atomics), for the configurations of the streaming kernels.  A default layer refuses inputs that require a gradient
exactly as before, and ``online_inference`` always does.

``HipWav2Win`` (:59-197) and ``HipWav2FFT`` (:227-324) hand out what the four above compute on the way and discard: the preprocessed
frames, ``(B, num_frames, pad_length)`` with the optional ``(B, num_frames)`` log-energies, and their complex STFT,
``(B, num_frames, fft_length / 2 + 1)`` ``complex64`` -- one launch of ``hipfeat_stft_run`` each, under the same restrictions.

All six also take a ragged batch, ``forward(x, lengths, padding_value=0.0)``: ``x`` is the zero-padded ``(B, Smax)`` tensor and row ``b``
is the waveform ``x[b, :lengths[b]]`` and nothing else -- framed as that cut alone, nothing behind its length read -- and the call returns
``(out, out_lens)`` with ``out`` collated to ``(B, max T_b, F)`` and ``padding_value`` behind each row's ``T_b`` frames, every element
written by the launch itself (``hipfeat_stft_run_ragged``; the four feature kinds through the plan's collated launch).  It combines with
``differentiable_()``: ``hipfeat_grad_run_ragged`` gives each row the gradient of the row alone and ``+0.0`` behind its length.
``_HipLayer.forward`` states the contract.

All six have the reference's second public method, ``online_inference(x, context=None)`` (:199-224, :326-333, :775-856): the chunked,
stateless streaming call that frames ``[context | x]``, returns what ``forward`` computes for the complete frames and hands back the
samples they did not consume.  One launch of ``hipfeat_stream_run`` per chunk (csrc/kernel_stream.hpp: the wave-per-frame kernels on a
two-span source), for the FFT sizes 256 / 512 / 1024 / 2048; every frame is computed by one wave from its own samples alone, so the
concatenated outputs of a stream are the same bits under any chunking.  One deliberate difference: where ``[context | x]`` is shorter
than a frame the reference raises; these return zero frames and the whole of ``[context | x]`` as the remainder, so a caller may feed
chunks shorter than a frame.
"""
from __future__ import annotations

import warnings
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, constants
from . import extractors as _E
from .compat import EPSILON, Seconds

__all__ = ["HipWav2Win", "HipWav2FFT", "HipWav2Spec", "HipWav2LogSpec", "HipWav2LogFilterBank", "HipWav2MFCC"]


# --------------------------------------------------------------------------------------
# online_inference: one hipfeat_stream handle per (layer, device, output), one launch per chunk (csrc/kernel_stream.hpp)
# --------------------------------------------------------------------------------------
_STREAM_SIZES = ("online_inference runs on the device for the FFT sizes 256, 512, 1024 and 2048 (round_to_power_of_two=True, 8 to 48 kHz at 25 ms), "
                 "frames of at most 2048 samples, frame_shift <= frame_length and at most 128 mel filters")


class _Stream(_E._DeviceHandle):
    """Owns one ``hipfeat_stream`` handle: the tables of one configuration on one device."""

    _what, _destroy = "layers", "hipfeat_stream_destroy"

    def __init__(self, create: str, args: tuple, n: int, shift: int, snip_edges: bool, width: int, energy_rows: bool, device: torch.device):
        super().__init__(device)
        self.n, self.shift, self.snip_edges, self.width, self.energy_rows = n, shift, bool(snip_edges), width, energy_rows
        self._create(create, *args)
        self._counts = np.zeros(2, dtype=np.int64)
        self._spare = torch.empty(2, dtype=torch.float32, device=self.device)  # a valid address for a context of no samples

    def counts(self, first: bool, context_len: int, chunk_len: int) -> Tuple[int, int]:
        """(frames, remainder length) of one call: hipfeat_stream_counts."""
        c = self._counts
        self.lib.check("hipfeat_stream_counts", self.n, self.shift, int(self.snip_edges), int(first), int(context_len), int(chunk_len), c.ctypes.data,
                       c.ctypes.data + 8)
        return int(c[0]), int(c[1])

    @staticmethod
    def _rows(t: torch.Tensor) -> torch.Tensor:
        B, S = t.shape
        if (S > 1 and t.stride(1) != 1) or (B > 1 and t.stride(0) < S):
            t = t.contiguous()
        return t

    def run(self, x: torch.Tensor, context: Optional[torch.Tensor]) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
        """x (B, S), context (B, R) or None -> (out (B, T, width), log-energies (B, T) or None, remainder (B, L - T shift)): fresh tensors,
        one launch on the current stream."""
        x = self._rows(x)
        B, S = x.shape
        first = context is None
        R = 0
        if not first:
            context = self._rows(context)
            R = int(context.shape[1])
        T, rem = self.counts(first, R, S)
        with torch.cuda.device(self.device):
            out = torch.empty((B, T, self.width), dtype=torch.float32, device=self.device)
            log_e = torch.empty((B, T), dtype=torch.float32, device=self.device) if self.energy_rows else None
            remainder = torch.empty((B, rem), dtype=torch.float32, device=self.device)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self.lib.check("hipfeat_stream_run", self.handle,
                           None if first else (context.data_ptr() or self._spare.data_ptr()), R, R if (first or B <= 1) else int(context.stride(0)),
                           x.data_ptr() or None, S, int(x.stride(0)) if B > 1 else S, B, out.data_ptr() or None, out.numel(),
                           None if log_e is None else (log_e.data_ptr() or None), remainder.data_ptr() or None, remainder.numel(), int(stream))
        return out, log_e, remainder


def _open_stream(layer, *args) -> _Stream:
    """``_Stream(*args)``; a configuration the streaming kernels do not have is ``layer``'s NotImplementedError."""
    try:
        return _Stream(*args)
    except _lib.HipFeatError as e:
        if e.status == _lib.ERR_UNSUPPORTED:
            raise NotImplementedError(f"{type(layer).__name__}.online_inference: {e} -- {_STREAM_SIZES}; forward() still serves this configuration "
                                      "where it did before") from e
        raise


# --------------------------------------------------------------------------------------
# differentiable_(): the waveform gradient, one hipfeat_grad handle per (layer, device, output) (csrc/kernel_grad.hpp)
# --------------------------------------------------------------------------------------
_GRAD_WORKSPACE_BYTES = 128 << 20  # rows are processed in pieces whose per-frame gradients fit this many bytes (half the Infinity Cache)
_GRAD_LIMITS = ("the waveform gradient runs on the device for the FFT sizes 256, 512, 1024 and 2048 (round_to_power_of_two=True, 8 to 48 kHz at 25 ms), "
                "frames of at most 2048 samples, frame_shift <= frame_length and at most 128 mel filters")


class _Grad(_E._DeviceHandle):
    """Owns one ``hipfeat_grad`` handle: the tables of one configuration on one device."""

    _what, _destroy = "layers", "hipfeat_grad_destroy"

    def __init__(self, layer, create: str, args: tuple, device: torch.device):
        super().__init__(device)
        try:
            self._create(create, *args)
        except _lib.HipFeatError as e:
            if e.status == _lib.ERR_UNSUPPORTED:
                raise NotImplementedError(f"{type(layer).__name__} in differentiable mode: {e} -- {_GRAD_LIMITS}; the plain forward() still "
                                          "serves this configuration where it did before") from e
            raise
        self._sizes = np.zeros(2, dtype=np.int64)

    def run(self, x: torch.Tensor, grad_out: Optional[torch.Tensor], grad_log_e: Optional[torch.Tensor]) -> torch.Tensor:
        """x (B, S): the saved waveform; grad_out (B, T, width) / grad_log_e (B, T): the cotangents (either may be None for the frames
        output) -> the (B, S) gradient, a fresh tensor every element of which the launches write; on the current stream."""
        x = _Stream._rows(x)
        B, S = x.shape
        with torch.cuda.device(self.device):
            grad = torch.empty((B, S), dtype=torch.float32, device=self.device)
            if B == 0 or S == 0:
                return grad
            z = self._sizes
            self.lib.check("hipfeat_grad_workspace", self.handle, B, S, int(_GRAD_WORKSPACE_BYTES), z.ctypes.data, z.ctypes.data + 8)
            workspace = torch.empty(max(int(z[1]), 4), dtype=torch.float32, device=self.device)
            cots = [None if g is None else g.to(torch.float32).contiguous() for g in (grad_out, grad_log_e)]
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self.lib.check("hipfeat_grad_run", self.handle, x.data_ptr(), B, S, int(x.stride(0)) if B > 1 else S,
                           None if cots[0] is None else cots[0].data_ptr(), 0 if cots[0] is None else cots[0].numel(),
                           None if cots[1] is None else cots[1].data_ptr(), grad.data_ptr(), S, workspace.data_ptr(), workspace.numel(), int(stream))
        return grad

    def run_ragged(self, x: torch.Tensor, lens: np.ndarray, tmax: int, grad_out: Optional[torch.Tensor], grad_log_e: Optional[torch.Tensor]) -> torch.Tensor:
        """``run`` for rows of ``lens[b]`` samples: the cotangents are (B, tmax, width) / (B, tmax) and their rows from a row's frame count on
        are never read; row ``b`` of the (B, S) gradient is that of ``x[b, :lens[b]]`` alone, followed by +0.0.  ``hipfeat_grad_run_ragged``."""
        x, stride = _rows_in_place(x)
        B, S = x.shape
        with torch.cuda.device(self.device):
            grad = torch.empty((B, S), dtype=torch.float32, device=self.device)
            if B == 0 or S == 0:
                return grad
            z = self._sizes
            self.lib.check("hipfeat_grad_workspace_ragged", self.handle, B, S, _lib.addr(lens), int(_GRAD_WORKSPACE_BYTES), z.ctypes.data, z.ctypes.data + 8)
            workspace = torch.empty(max(int(z[1]), 4), dtype=torch.float32, device=self.device)
            cots = [None if g is None else g.to(torch.float32).contiguous() for g in (grad_out, grad_log_e)]
            assert cots[0] is None or cots[0].shape[:2] == (B, tmax), (tuple(cots[0].shape), B, tmax)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self.lib.check("hipfeat_grad_run_ragged", self.handle, x.data_ptr(), B, S, stride, _lib.addr(lens),
                           None if cots[0] is None else (cots[0].data_ptr() or workspace.data_ptr()), 0 if cots[0] is None else cots[0].numel(),
                           None if cots[1] is None else (cots[1].data_ptr() or workspace.data_ptr()), grad.data_ptr(), S, workspace.data_ptr(),
                           workspace.numel(), int(stream))
        return grad


class _WaveGrad(torch.autograd.Function):
    """``forward``: the launch the plain path makes (``run(x) -> (out, log-energies or None)``); saves only the waveform.  ``backward``:
    ``hipfeat_grad_run`` on the cotangents, either of which may be None.  With ``ragged`` (a ``_Lengths``) the host lengths are kept next
    to the waveform and the backward is ``hipfeat_grad_run_ragged``."""

    @staticmethod
    def forward(ctx, x, run, grad: _Grad, ragged=None):
        out, log_e = run(x.detach())
        ctx.save_for_backward(x)
        ctx.grad = grad
        ctx.ragged = ragged
        ctx.set_materialize_grads(False)
        if log_e is None:
            return out
        return out, log_e

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, grad_log_e=None):
        if grad_out is None and grad_log_e is None:
            return None, None, None, None
        (x,) = ctx.saved_tensors
        r = ctx.ragged
        if r is not None:
            return ctx.grad.run_ragged(x, r.lens, r.tmax, grad_out, grad_log_e), None, None, None
        return ctx.grad.run(x, grad_out, grad_log_e), None, None, None


def _wants_grad(layer, x) -> bool:
    """``layer`` is differentiable and ``x`` asks for a gradient under grad mode."""
    return bool(getattr(layer, "_differentiable", False)) and isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled()


def _check_grad_input(layer, x) -> Tuple[torch.Tensor, bool]:
    """``_check_waveforms`` for an input that keeps its graph: float32, ``(B, T)`` or ``(T,)`` -> (the ``(B, T)`` batch, whether 1-D)."""
    if x.dtype != torch.float32:
        raise TypeError(f"{type(layer).__name__}: expected float32 samples, got {x.dtype}")
    squeeze = x.ndim == 1
    if squeeze:
        x = x.unsqueeze(0)
    assert x.ndim == 2, f"expected a (B, T) batch of waveforms, got shape {tuple(x.shape)}"
    return x, squeeze


class _Differentiable:
    """``differentiable_()`` of the six layers: a private flag, kept by pickling, outside ``state_dict()`` and ``repr``."""

    def differentiable_(self, flag: bool = True):
        """Make ``forward`` backpropagate to the waveform (``flag=False``: refuse inputs that require a gradient again).  Returns self."""
        self._differentiable = bool(flag)
        return self

    @property
    def differentiable(self) -> bool:
        return bool(getattr(self, "_differentiable", False))


def _check_waveforms(layer, x, method: str = "forward") -> Tuple[torch.Tensor, bool]:
    """The argument check of every layer: a float32 ``(B, T)`` or ``(T,)`` tensor that does not ask for a gradient -> (the detached
    ``(B, T)`` batch, whether it was 1-D)."""
    name = type(layer).__name__
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}.{method} expects a torch.Tensor, got {type(x).__name__}")
    if x.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{name} is inference-only (no autograd); call it under torch.no_grad() or detach the input")
    if x.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32 samples, got {x.dtype}")
    squeeze = x.ndim == 1
    if squeeze:
        x = x.unsqueeze(0)
    assert x.ndim == 2, f"expected a (B, T) batch of waveforms, got shape {tuple(x.shape)}"
    return x.detach(), squeeze


# --------------------------------------------------------------------------------------
# forward(x, lengths): a zero-padded (B, Smax) batch whose row b is the waveform x[b, :lengths[b]] and nothing else
# --------------------------------------------------------------------------------------
class _Lengths:
    """The checked row lengths of one ragged call, on the host (int64): ``lens``, the frame counts ``frames`` and their maximum ``tmax``.
    ``out_lens()`` gives the frame counts back as the caller gave the lengths: a tensor of their dtype on their device, else int64 on the
    CPU."""

    def __init__(self, layer, x: torch.Tensor, lengths, n: int, shift: int, snip_edges: bool):
        name = type(layer).__name__
        self._like = lengths if isinstance(lengths, torch.Tensor) else None
        if isinstance(lengths, torch.Tensor):
            if lengths.dtype.is_floating_point or lengths.dtype.is_complex or lengths.dtype == torch.bool:
                raise TypeError(f"{name}: lengths must be integers, got {lengths.dtype}")
            lens = lengths.detach().cpu().numpy()  # (a device tensor: one copy to the host, which waits for the device)
        else:
            lens = np.asarray(lengths)
            if lens.dtype.kind not in "iu":
                raise TypeError(f"{name}: lengths must be integers, got {lens.dtype}")
        B, S = x.shape
        if lens.ndim != 1 or lens.shape[0] != B:
            raise ValueError(f"{name}: {B} rows but lengths of shape {tuple(lens.shape)}")
        lens = np.ascontiguousarray(lens, dtype=np.int64)
        bad = np.flatnonzero((lens < 0) | (lens > S))
        if bad.size:
            b = int(bad[0])
            raise ValueError(f"{name}: row {b}: length {int(lens[b])} is outside [0, {S}], the rows of x")
        if snip_edges:
            frames = np.where(lens < n, 0, 1 + (lens - n) // shift).astype(np.int64)
        else:
            frames = (lens + shift // 2) // shift
            lib = _lib.load()
            for s in np.unique(lens):  # the uniform call's HIPFEAT_ERR_TOO_SHORT, before anything is launched
                if lib.raw("hipfeat_check_length", int(s), n, shift, 0) != 0:
                    raise ValueError(f"{name}: row {int(np.flatnonzero(lens == s)[0])}: {lib.last_error()}")
        self.lens, self.frames, self.tmax = lens, frames, int(frames.max(initial=0))

    def out_lens(self) -> torch.Tensor:
        if self._like is None:
            return torch.from_numpy(self.frames.copy())
        return torch.as_tensor(self.frames, dtype=self._like.dtype, device=self._like.device)


def _rows_in_place(x: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """``x`` (B, S) as the kernels read it in place -- unit column stride, rows that do not overlap -- or its contiguous copy, and the row
    stride in elements."""
    x = _Stream._rows(x)
    B, S = x.shape
    return x, (int(x.stride(0)) if B > 1 else S)


def _check_stream_input(layer, x, context) -> Tuple[torch.Tensor, Optional[torch.Tensor], bool]:
    """``_check_waveforms`` on the chunk, and the reference's assertions on the context (layers.py:832-833): a 2-D tensor with the
    chunk's batch size -- here also float32 and on the chunk's device."""
    x, squeeze = _check_waveforms(layer, x, "online_inference")
    if context is not None:
        assert isinstance(context, torch.Tensor) and context.ndim == 2, "context must be a (B, R) tensor: the remainder of the previous call"
        assert context.shape[0] == x.shape[0], f"context has batch size {context.shape[0]}, the chunk {x.shape[0]}"
        assert context.dtype == torch.float32 and context.device == x.device, (
            f"context must be float32 on the chunk's device ({x.device}), got {context.dtype} on {context.device}")
        context = context.detach()
    return x, context, squeeze


class _HipLayer(_Differentiable, torch.nn.Module):
    kind: int = -1

    def __init__(self, **opts):
        super().__init__()
        for k, v in opts.items():
            setattr(self, k, v)
        self._opts = dict(opts)
        n, shift, fft = constants.frame_sizes(opts["sampling_rate"], opts["frame_length"], opts["frame_shift"], opts["round_to_power_of_two"])
        self.fft_length = fft  # Wav2FFT.fft_length (layers.py:281-286)
        self._n, self._shift = n, shift
        self._plans = {}
        self._streams = {}

    def _plan_config(self) -> SimpleNamespace:
        """The layer's options as ``extractors.plan_inputs`` reads them: those a kind does not have at their neutral values."""
        return SimpleNamespace(**{**dict(num_filters=0, num_ceps=0, cepstral_lifter=0, low_freq=20.0, high_freq=-400.0, norm_filters=False,
                                         torchaudio_compatible_mel_scale=True, use_fft_mag=False), **self._opts})

    def _plan_for(self, device: torch.device, no_dither: bool = False):
        """The layer's plan on ``device``; ``no_dither``: the plan of the same layer with dither 0 (the differentiable path adds the noise
        itself, so that the gradient passes through the addition)."""
        no_dither = no_dither and self._opts["dither"] != 0.0
        key = (device.type, device.index, "no-dither") if no_dither else (device.type, device.index)
        plan = self._plans.get(key)
        if plan is None:
            cfg = self._plan_config()
            if no_dither:
                cfg.dither = 0.0
            plan = _E._Plan(cfg, self.kind, device)  # refuses anything but a 'cuda' device: there is no CPU fallback
            self._plans[key] = plan
        return plan

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_plans"] = {}  # device handles are per process
        st["_streams"] = {}
        st["_grads"] = {}
        return st

    def _grad_for(self, device: torch.device) -> _Grad:
        key = (device.type, device.index)
        g = self.__dict__.setdefault("_grads", {}).get(key)
        if g is None:
            c, window, mel, dct, lifter, _ = _E.plan_inputs(self._plan_config(), self.kind)
            g = self._grads[key] = _Grad(self, "hipfeat_grad_create_features", tuple(_lib.addr(a) for a in (c, window, mel, dct, lifter)), device)
        return g

    def _run_plan(self, plan, x: torch.Tensor) -> torch.Tensor:
        """(B, T) float32 on the plan's device -> (B, num_frames, F): the one launch of ``forward``."""
        B, T = x.shape
        wave = x.contiguous().reshape(-1)
        offs = np.arange(B, dtype=np.int64) * T
        lens = np.full(B, T, dtype=np.int64)
        try:
            packed, frames = plan.run(wave, offs, lens, None)
        except _lib.HipFeatError as e:
            if e.status == _lib.ERR_TOO_SHORT:
                raise ValueError(str(e)) from e
            raise
        return packed.reshape(B, int(frames[0]) if B else 0, plan.feature_dim)

    def _forward_differentiable(self, x: torch.Tensor) -> torch.Tensor:
        x, squeeze = _check_grad_input(self, x)
        grad = self._grad_for(x.device)  # (a configuration without a gradient kernel is refused before anything runs)
        plan = self._plan_for(x.device, no_dither=True)
        dither = self._opts["dither"]
        if dither != 0.0:  # layers.py:191-193
            x = x + dither * torch.randn(x.shape, device=x.device)
        out = _WaveGrad.apply(x, lambda w: (self._run_plan(plan, w), None), grad, None)
        return out[0] if squeeze else out

    def _run_plan_ragged(self, plan, x: torch.Tensor, r: _Lengths, padding_value: float) -> torch.Tensor:
        """(B, Smax) float32 on the plan's device, row ``b`` of ``r.lens[b]`` samples -> (B, Tmax, F) with ``padding_value`` in the rows from
        ``r.frames[b]`` on: the plan's collated launch, the rows read in place as cuts at the offsets ``b * row stride``."""
        B, S = x.shape
        if B == 0 or r.tmax == 0:
            return torch.empty((B, 0, plan.feature_dim), dtype=torch.float32, device=x.device)
        if plan.dither != 0.0:
            x = x.contiguous()  # the plan draws its noise for the tensor it is given: the whole (B, Smax) batch, as the uniform call
        x, stride = _rows_in_place(x)
        wave = torch.as_strided(x, ((B - 1) * stride + S,), (1,))  # the rows and the gaps between them as one 1-D buffer: no copy
        out, frames = plan.run_collated(wave, np.arange(B, dtype=np.int64) * stride, r.lens, None, float(padding_value))
        assert np.array_equal(frames, r.frames) and out.shape == (B, r.tmax, plan.feature_dim)
        return out

    def _forward_ragged(self, x: torch.Tensor, lengths, padding_value: float) -> Tuple[torch.Tensor, torch.Tensor]:
        wants = _wants_grad(self, x)
        x, _ = _check_grad_input(self, x) if wants else _check_waveforms(self, x)
        r = _Lengths(self, x, lengths, self._n, self._shift, self._opts["snip_edges"])
        if not wants:
            return self._run_plan_ragged(self._plan_for(x.device), x, r, padding_value), r.out_lens()
        grad = self._grad_for(x.device)
        plan = self._plan_for(x.device, no_dither=True)
        dither = self._opts["dither"]
        if dither != 0.0:  # layers.py:191-193, for the whole tensor; only each row's first lengths[b] samples of it are read
            x = x + dither * torch.randn(x.shape, device=x.device)
        out = _WaveGrad.apply(x, lambda w: (self._run_plan_ragged(plan, w, r, padding_value), None), grad, r)
        return out, r.out_lens()

    def _stream_for(self, device: torch.device) -> _Stream:
        key = (device.type, device.index)
        s = self.__dict__.setdefault("_streams", {}).get(key)
        if s is None:
            # the tables of hipfeat_plan_create, for the streaming kernel's own handle
            c, window, mel, dct, lifter, (n, shift, fft) = _E.plan_inputs(self._plan_config(), self.kind)
            width = {_E.KIND_FBANK: int(c["num_filters"][0] + c["use_energy"][0]), _E.KIND_MFCC: int(c["num_ceps"][0])}.get(self.kind, fft // 2 + 1)
            args = tuple(_lib.addr(a) for a in (c, window, mel, dct, lifter))
            s = self._streams[key] = _open_stream(self, "hipfeat_stream_create_features", args, n, shift, self._opts["snip_edges"], width, False, device)
        return s

    def online_inference(self, x: torch.Tensor, context: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The reference's chunked, stateless streaming call (layers.py:326-333): ``(output, remainder)`` for the chunk ``x`` and the
        remainder of the previous call (``None`` at the start of a stream; any ``(B, R)`` tensor is accepted).  ``output`` holds the
        frames of ``[context | x]`` that are complete -- what ``forward`` computes per frame, without a reflection on the right --
        and ``remainder`` the ``(B, L - T * shift)`` samples they did not consume.  One launch on the current stream; the concatenated
        outputs of a stream do not depend on how it was cut into chunks, bit for bit.  Unlike the reference, which raises when
        ``[context | x]`` is shorter than a frame, this returns ``(B, 0, F)`` and all of ``[context | x]`` as the remainder.  A 1-D
        chunk gives a 2-D output; the remainder stays ``(1, R)``, ready to be passed back."""
        x, context, squeeze = _check_stream_input(self, x, context)
        s = self._stream_for(x.device)
        dither = self._opts["dither"]
        if dither != 0.0:  # layers.py:209-212: the chunk alone
            x = x + dither * torch.randn(x.shape, device=x.device)
        out, _, remainder = s.run(x, context)
        return (out[0] if squeeze else out), remainder

    def forward(self, x: torch.Tensor, lengths=None, padding_value: float = 0.0):
        """``forward(x)``: a ``(B, T)`` or ``(T,)`` batch of equally long waveforms -> ``(B, num_frames, F)``.

        ``forward(x, lengths, padding_value=0.0)``: the ragged batch.  ``x`` is a zero-padded ``(B, Smax)`` batch read in place (any row
        stride) and row ``b`` is the waveform ``x[b, :lengths[b]]`` and nothing else: its ``T_b`` frames are those of that cut alone, with
        its own reflection at both ends, and ``x[b, lengths[b]:]`` is never read.  Returns ``(out, out_lens)``: ``out`` is
        ``(B, max T_b, F)`` with ``padding_value`` in ``out[b, T_b:]`` (written by the same launch), ``out_lens`` holds the ``T_b`` --
        a tensor of the dtype and on the device of ``lengths`` if that was a tensor, else int64 on the CPU.  ``lengths``: ``B``
        non-negative integers ``<= Smax`` as a sequence, a numpy array or an integer tensor; a DEVICE tensor is copied to the host once,
        which synchronises with the device (the host validates the lengths and computes ``out_lens``).  With ``snip_edges=True`` a row
        shorter than a frame has zero frames; with ``snip_edges=False`` a row too short for its reflection raises the ``ValueError`` of the
        uniform call, naming the row, before anything is launched.  ``dither != 0`` draws ``torch.randn`` for the whole ``(B, Smax)``
        tensor, as the uniform call does; only each row's first ``lengths[b]`` samples of it are read.  A 1-D ``x`` with a one-element
        ``lengths`` is the batch of one row: the outputs keep their leading dimension of 1.  With ``differentiable_()``,
        ``grad[b, :lengths[b]]`` is the gradient of the row alone, ``grad[b, lengths[b]:]`` is ``+0.0`` and the cotangent's padding rows
        are never read."""
        if lengths is not None:
            return self._forward_ragged(x, lengths, padding_value)
        if _wants_grad(self, x):
            return self._forward_differentiable(x)
        x, squeeze = _check_waveforms(self, x)
        out = self._run_plan(self._plan_for(x.device), x)
        return out[0] if squeeze else out


def _common(sampling_rate, frame_length, frame_shift, round_to_power_of_two, remove_dc_offset, preemph_coeff, window_type, dither, snip_edges,
            energy_floor, raw_energy, use_energy):
    return dict(sampling_rate=sampling_rate, frame_length=frame_length, frame_shift=frame_shift, round_to_power_of_two=round_to_power_of_two,
                remove_dc_offset=remove_dc_offset, preemph_coeff=preemph_coeff, window_type=window_type, dither=dither, snip_edges=snip_edges,
                energy_floor=energy_floor, raw_energy=raw_energy, use_energy=use_energy)


class HipWav2Spec(_HipLayer):
    """Power (or magnitude) spectrum; ``use_energy`` (default True, as in the reference) puts the log-energy in bin 0."""

    kind = _E.KIND_SPECTROGRAM

    def __init__(self, sampling_rate: int = 16000, frame_length: Seconds = 0.025, frame_shift: Seconds = 0.01, round_to_power_of_two: bool = True,
                 remove_dc_offset: bool = True, preemph_coeff: float = 0.97, window_type: str = "povey", dither: float = 0.0,
                 snip_edges: bool = False, energy_floor: float = EPSILON, raw_energy: bool = True, use_energy: bool = True,
                 use_fft_mag: bool = False):
        super().__init__(**_common(sampling_rate, frame_length, frame_shift, round_to_power_of_two, remove_dc_offset, preemph_coeff, window_type,
                                   dither, snip_edges, energy_floor, raw_energy, use_energy), use_fft_mag=use_fft_mag)


class HipWav2LogSpec(_HipLayer):
    """``log(spectrum + 1e-15)``; ``use_energy`` (default True) puts the log-energy in bin 0."""

    kind = _E.KIND_LOG_SPECTROGRAM

    def __init__(self, sampling_rate: int = 16000, frame_length: Seconds = 0.025, frame_shift: Seconds = 0.01, round_to_power_of_two: bool = True,
                 remove_dc_offset: bool = True, preemph_coeff: float = 0.97, window_type: str = "povey", dither: float = 0.0,
                 snip_edges: bool = False, energy_floor: float = EPSILON, raw_energy: bool = True, use_energy: bool = True,
                 use_fft_mag: bool = False):
        super().__init__(**_common(sampling_rate, frame_length, frame_shift, round_to_power_of_two, remove_dc_offset, preemph_coeff, window_type,
                                   dither, snip_edges, energy_floor, raw_energy, use_energy), use_fft_mag=use_fft_mag)


class HipWav2LogFilterBank(_HipLayer):
    """Log-mel filterbank energies (``use_energy`` prepends the log-energy column, layers.py:575-576)."""

    kind = _E.KIND_FBANK

    def __init__(self, sampling_rate: int = 16000, frame_length: Seconds = 0.025, frame_shift: Seconds = 0.01, round_to_power_of_two: bool = True,
                 remove_dc_offset: bool = True, preemph_coeff: float = 0.97, window_type: str = "povey", dither: float = 0.0,
                 snip_edges: bool = False, energy_floor: float = EPSILON, raw_energy: bool = True, use_energy: bool = False,
                 use_fft_mag: bool = False, low_freq: float = 20.0, high_freq: float = -400.0, num_filters: int = 80,
                 norm_filters: bool = False, torchaudio_compatible_mel_scale: bool = True):
        super().__init__(**_common(sampling_rate, frame_length, frame_shift, round_to_power_of_two, remove_dc_offset, preemph_coeff, window_type,
                                   dither, snip_edges, energy_floor, raw_energy, use_energy), use_fft_mag=use_fft_mag, low_freq=low_freq,
                         high_freq=high_freq, num_filters=num_filters, norm_filters=norm_filters,
                         torchaudio_compatible_mel_scale=torchaudio_compatible_mel_scale)


class HipWav2MFCC(_HipLayer):
    """MFCCs: log-mel, DCT, lifter.  ``use_energy=True`` replaces C0 by the log-energy (the reference raises a shape error
    there; this is what it documents)."""

    kind = _E.KIND_MFCC

    def __init__(self, sampling_rate: int = 16000, frame_length: Seconds = 0.025, frame_shift: Seconds = 0.01, round_to_power_of_two: bool = True,
                 remove_dc_offset: bool = True, preemph_coeff: float = 0.97, window_type: str = "povey", dither: float = 0.0,
                 snip_edges: bool = False, energy_floor: float = EPSILON, raw_energy: bool = True, use_energy: bool = False,
                 use_fft_mag: bool = False, low_freq: float = 20.0, high_freq: float = -400.0, num_filters: int = 23,
                 norm_filters: bool = False, num_ceps: int = 13, cepstral_lifter: int = 22, torchaudio_compatible_mel_scale: bool = True):
        super().__init__(**_common(sampling_rate, frame_length, frame_shift, round_to_power_of_two, remove_dc_offset, preemph_coeff, window_type,
                                   dither, snip_edges, energy_floor, raw_energy, use_energy), use_fft_mag=use_fft_mag, low_freq=low_freq,
                         high_freq=high_freq, num_filters=num_filters, norm_filters=norm_filters, num_ceps=num_ceps,
                         cepstral_lifter=cepstral_lifter, torchaudio_compatible_mel_scale=torchaudio_compatible_mel_scale)


# --------------------------------------------------------------------------------------
# Wav2Win / Wav2FFT: the two layers whose output is not a real feature matrix (hipfeat_stft_*, csrc/kernel_stft.hpp)
# --------------------------------------------------------------------------------------
def _stft_inputs(win: "HipWav2Win", output: int) -> Tuple[np.ndarray, np.ndarray, int, bool]:
    """What ``hipfeat_stft_create`` and ``hipfeat_stream_create_stft`` take for ``win``: the ``STFT_CONFIG_DTYPE`` record and the window;
    with them the floats of an output row and whether the log-energies come as rows of their own (the spectrum carries its log-energy
    in bin 0: no separate row of them is asked for)."""
    spectrum = output == _lib.STFT_SPECTRUM
    cfg = np.zeros(1, dtype=_lib.STFT_CONFIG_DTYPE)
    cfg["struct_size"] = _lib.STFT_CONFIG_DTYPE.itemsize
    cfg["output"], cfg["frame_length"], cfg["frame_shift"], cfg["pad_length"] = output, win._length, win._shift, win.pad_length
    cfg["snip_edges"], cfg["remove_dc_offset"] = int(bool(win.snip_edges)), int(bool(win.remove_dc_offset))
    cfg["raw_energy"], cfg["want_energy"] = int(bool(win.raw_energy)), int(bool(win.return_log_energy))
    cfg["preemph_coeff"], cfg["energy_floor"] = float(win.preemph_coeff), float(win.energy_floor)
    window = np.ascontiguousarray(win._window.detach().cpu().numpy(), dtype=np.float32)
    assert window.shape == (win._length,)
    return cfg, window, win.pad_length + 2 if spectrum else win.pad_length, bool(win.return_log_energy) and not spectrum


class _Stft(_E._DeviceHandle):
    """Owns one ``hipfeat_stft`` handle: the window (and twiddles) of one configuration on one device."""

    _what, _destroy = "layers", "hipfeat_stft_destroy"

    def __init__(self, win: "HipWav2Win", output: int, device: torch.device):
        super().__init__(device)
        self.n, self.shift, self.snip_edges = win._length, win._shift, bool(win.snip_edges)
        cfg, window, self.width, self.energy_rows = _stft_inputs(win, output)
        self._create("hipfeat_stft_create", _lib.addr(cfg), _lib.addr(window))

    def run(self, x: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """x: (B, S) float32 on the handle's device -> ((B, T, width) float32, (B, T) log-energies or None), on the current stream."""
        B, S = x.shape
        if (S > 1 and x.stride(1) != 1) or (B > 1 and x.stride(0) < S):
            x = x.contiguous()
        frames = int(self.lib.raw("hipfeat_num_frames", S, self.n, self.shift, int(self.snip_edges)))
        with torch.cuda.device(self.device):
            out = torch.empty((B, frames, self.width), dtype=torch.float32, device=self.device)
            log_e = torch.empty((B, frames), dtype=torch.float32, device=self.device) if self.energy_rows else None
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self.lib.check("hipfeat_stft_run", self.handle, x.data_ptr(), B, S, int(x.stride(0)) if B > 1 else S, out.data_ptr(), out.numel(),
                           None if log_e is None else log_e.data_ptr(), int(stream))
        return out, log_e

    def run_ragged(self, x: torch.Tensor, r: _Lengths, padding_value: float) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """``run`` for rows of ``r.lens[b]`` samples, read in place: ((B, Tmax, width), (B, Tmax) or None), every element written by the one
        launch of ``hipfeat_stft_run_ragged`` -- ``padding_value`` from a row's frame count on."""
        x, stride = _rows_in_place(x)
        B, S = x.shape
        with torch.cuda.device(self.device):
            out = torch.empty((B, r.tmax, self.width), dtype=torch.float32, device=self.device)
            log_e = torch.empty((B, r.tmax), dtype=torch.float32, device=self.device) if self.energy_rows else None
            if out.numel():
                stream = torch.cuda.current_stream(self.device).cuda_stream
                self.lib.check("hipfeat_stft_run_ragged", self.handle, x.data_ptr(), B, S, stride, _lib.addr(r.lens), float(padding_value), out.data_ptr(),
                               out.numel(), None if log_e is None else log_e.data_ptr(), int(stream))
        return out, log_e


class HipWav2Win(_Differentiable, torch.nn.Module):
    """Kaldi preprocessing (DC offset, pre-emphasis, window, zero padding to ``pad_length``) of overlapping frames: the reference's
    ``Wav2Win`` (layers.py:59-197).  ``forward(x)`` returns the 2-tuple ``(frames, log_energy or None)`` with ``frames`` of shape
    ``(B, num_frames, pad_length)`` and ``log_energy`` of shape ``(B, num_frames)`` when ``return_log_energy``."""

    _output = _lib.STFT_FRAMES

    def __init__(self, sampling_rate: int = 16000, frame_length: Seconds = 0.025, frame_shift: Seconds = 0.01, pad_length: Optional[int] = None,
                 remove_dc_offset: bool = True, preemph_coeff: float = 0.97, window_type: str = "povey", dither: float = 0.0,
                 snip_edges: bool = False, energy_floor: float = EPSILON, raw_energy: bool = True, return_log_energy: bool = False) -> None:
        super().__init__()
        self.sampling_rate = sampling_rate
        self.frame_length = frame_length
        self.frame_shift = frame_shift
        self.remove_dc_offset = remove_dc_offset
        self.preemph_coeff = preemph_coeff
        self.window_type = window_type
        self.dither = dither
        self.snip_edges = snip_edges
        self.energy_floor = energy_floor
        self.raw_energy = raw_energy
        self.return_log_energy = return_log_energy
        if snip_edges:
            warnings.warn("Setting snip_edges=True is generally incompatible with Lhotse -- "
                          "you might experience mismatched duration/num_frames errors.")
        n, shift, _ = constants.frame_sizes(sampling_rate, frame_length, frame_shift, False)
        self._length = n
        self._shift = shift
        self._window = torch.nn.Parameter(torch.from_numpy(np.array(constants.make_window(n, window_type), dtype=np.float32)), requires_grad=False)
        self.pad_length = n if pad_length is None else pad_length
        assert self.pad_length >= n, f"pad_length (or fft_length) = {pad_length} cannot be smaller than N = {n}"
        self._handles = {}

    def __repr__(self):
        return self.__str__()

    def __str__(self):
        return ("{}(sampling_rate={}, frame_length={}, frame_shift={}, pad_length={}, remove_dc_offset={}, preemph_coeff={}, window_type={} "
                "dither={}, snip_edges={}, energy_floor={}, raw_energy={}, return_log_energy={})").format(
                    self.__class__.__name__, self.sampling_rate, self.frame_length, self.frame_shift, self.pad_length, self.remove_dc_offset,
                    self.preemph_coeff, self.window_type, self.dither, self.snip_edges, self.energy_floor, self.raw_energy, self.return_log_energy)

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_handles"] = {}  # device handles are per process
        return st

    def _handle_for(self, device: torch.device, output: int) -> _Stft:
        key = (device.type, device.index, output)
        h = self._handles.get(key)
        if h is None:
            try:
                h = _Stft(self, output, device)
            except _lib.HipFeatError as e:
                if e.status == _lib.ERR_UNSUPPORTED:
                    raise NotImplementedError(
                        f"{e} -- the device layers have the FFT sizes 256, 512, 1024 and 2048 (round_to_power_of_two=True) and frames of at "
                        f"most 2048 samples; this layer has frame length {self._length} and pad / fft length {self.pad_length}") from e
                raise
            self._handles[key] = h
        return h

    def _grad_for(self, device: torch.device, output: int, layer) -> _Grad:
        key = (device.type, device.index, output, "grad")
        g = self._handles.get(key)
        if g is None:
            cfg, window, _, _ = _stft_inputs(self, output)
            g = self._handles[key] = _Grad(layer, "hipfeat_grad_create_stft", (_lib.addr(cfg), _lib.addr(window)), device)
        return g

    @staticmethod
    def _launch(handle: _Stft, x: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        try:
            return handle.run(x)
        except _lib.HipFeatError as e:
            if e.status == _lib.ERR_TOO_SHORT:
                raise ValueError(str(e)) from e
            raise

    def _run(self, x: torch.Tensor, output: int, layer=None) -> Tuple[torch.Tensor, Optional[torch.Tensor], bool]:
        """``layer``: the layer whose call this is (``HipWav2FFT`` runs its ``wav2win``), whose flag decides and whose name refusals carry."""
        layer = self if layer is None else layer
        if _wants_grad(layer, x):
            x, squeeze = _check_grad_input(layer, x)
            grad = self._grad_for(x.device, output, layer)  # (a configuration without a gradient kernel is refused before anything runs)
            handle = self._handle_for(x.device, output)
            if self.dither != 0.0:  # layers.py:191-193
                x = x + self.dither * torch.randn(x.shape, device=x.device)
            res = _WaveGrad.apply(x, lambda w: self._launch(handle, w), grad, None)
            out, log_e = res if isinstance(res, tuple) else (res, None)
            return out, log_e, squeeze
        x, squeeze = _check_waveforms(layer, x)
        handle = self._handle_for(x.device, output)
        if self.dither != 0.0:  # layers.py:191-193
            x = x + self.dither * torch.randn(x.shape, device=x.device)
        out, log_e = self._launch(handle, x)
        return out, log_e, squeeze

    def _run_ragged(self, x: torch.Tensor, lengths, padding_value: float, output: int,
                    layer=None) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
        """``_run`` for the rows ``x[b, :lengths[b]]`` (``_HipLayer.forward`` states the contract): (out (B, Tmax, width), log-energies
        (B, Tmax) or None, out_lens)."""
        layer = self if layer is None else layer
        wants = _wants_grad(layer, x)
        x, _ = _check_grad_input(layer, x) if wants else _check_waveforms(layer, x)
        r = _Lengths(layer, x, lengths, self._length, self._shift, self.snip_edges)
        grad = self._grad_for(x.device, output, layer) if wants else None  # (refused before anything runs)
        handle = self._handle_for(x.device, output)
        if self.dither != 0.0:  # layers.py:191-193, for the whole tensor; only each row's first lengths[b] samples of it are read
            x = x + self.dither * torch.randn(x.shape, device=x.device)
        if not wants:
            out, log_e = handle.run_ragged(x, r, padding_value)
            return out, log_e, r.out_lens()
        res = _WaveGrad.apply(x, lambda w: handle.run_ragged(w, r, padding_value), grad, r)
        out, log_e = res if isinstance(res, tuple) else (res, None)
        return out, log_e, r.out_lens()

    def forward(self, x: torch.Tensor, lengths=None, padding_value: float = 0.0):
        """``forward(x)``: ``(frames, log_energy or None)`` of equally long rows.  ``forward(x, lengths, padding_value=0.0)``: the ragged
        batch of ``_HipLayer.forward`` -- ``((frames, log_energy or None), out_lens)``, the shape of ``online_inference``'s pair, with
        ``frames[b, T_b:]`` and ``log_energy[b, T_b:]`` equal to ``padding_value``; a device ``lengths`` tensor is copied to the host once
        (a synchronisation); ``dither`` is drawn for the whole ``(B, Smax)`` tensor and only each row's first ``lengths[b]`` samples of it
        are read."""
        if lengths is not None:
            out, log_e, out_lens = self._run_ragged(x, lengths, padding_value, self._output)
            return (out, log_e), out_lens
        out, log_e, squeeze = self._run(x, self._output)
        if squeeze:
            return out[0], (None if log_e is None else log_e[0])
        return out, log_e

    def _stream_for(self, device: torch.device, output: int, layer) -> _Stream:
        key = (device.type, device.index, output, "stream")
        s = self._handles.get(key)
        if s is None:
            cfg, window, width, energy_rows = _stft_inputs(self, output)
            s = self._handles[key] = _open_stream(layer, "hipfeat_stream_create_stft", (_lib.addr(cfg), _lib.addr(window)), self._length, self._shift,
                                                  self.snip_edges, width, energy_rows, device)
        return s

    def _online(self, x: torch.Tensor, context: Optional[torch.Tensor], output: int, layer):
        x, context, squeeze = _check_stream_input(layer, x, context)
        s = self._stream_for(x.device, output, layer)
        if self.dither != 0.0:  # layers.py:209-212: the chunk alone, before the concatenation
            x = x + self.dither * torch.randn(x.shape, device=x.device)
        out, log_e, remainder = s.run(x, context)
        return out, log_e, remainder, squeeze

    def online_inference(self, x: torch.Tensor, context: Optional[torch.Tensor] = None
                         ) -> Tuple[Tuple[torch.Tensor, Optional[torch.Tensor]], torch.Tensor]:
        """The reference's chunked, stateless streaming call (layers.py:199-224): ``((frames, log_energy), remainder)`` for the chunk
        ``x`` and the remainder of the previous call (``None`` at the start of a stream, where without ``snip_edges`` the first
        ``min((N - shift) // 2, S)`` samples are reflected in front; any ``(B, R)`` tensor is accepted as a context).  The frames are
        those of ``[context | x]`` that are complete, ``T = 1 + (L - N) // shift`` of them, never reflected on the right; ``remainder``
        is ``[context | x][:, T * shift:]``, fresh and contiguous.  One launch on the current stream; the concatenated outputs of a
        stream do not depend on how it was cut into chunks, bit for bit.  Unlike the reference, which raises when ``[context | x]``
        is shorter than a frame, this returns ``(B, 0, pad_length)`` frames (and ``(B, 0)`` log-energies) and all of ``[context | x]``
        as the remainder.  A 1-D chunk gives 2-D frames; the remainder stays ``(1, R)``, ready to be passed back."""
        out, log_e, remainder, squeeze = self._online(x, context, self._output, self)
        if squeeze:
            return (out[0], (None if log_e is None else log_e[0])), remainder
        return (out, log_e), remainder


class HipWav2FFT(_Differentiable, torch.nn.Module):
    """The complex STFT of the Kaldi-preprocessed frames: the reference's ``Wav2FFT`` (layers.py:227-324).  ``forward(x)`` returns a
    ``complex64`` tensor of shape ``(B, num_frames, fft_length / 2 + 1)``; ``use_energy`` (default True) puts the log-energy in bin 0."""

    def __init__(self, sampling_rate: int = 16000, frame_length: Seconds = 0.025, frame_shift: Seconds = 0.01, round_to_power_of_two: bool = True,
                 remove_dc_offset: bool = True, preemph_coeff: float = 0.97, window_type: str = "povey", dither: float = 0.0,
                 snip_edges: bool = False, energy_floor: float = EPSILON, raw_energy: bool = True, use_energy: bool = True) -> None:
        super().__init__()
        self.use_energy = use_energy
        _, _, self.fft_length = constants.frame_sizes(sampling_rate, frame_length, frame_shift, round_to_power_of_two)
        self.wav2win = HipWav2Win(sampling_rate, frame_length, frame_shift, pad_length=self.fft_length, remove_dc_offset=remove_dc_offset,
                                  preemph_coeff=preemph_coeff, window_type=window_type, dither=dither, snip_edges=snip_edges,
                                  energy_floor=energy_floor, raw_energy=raw_energy, return_log_energy=use_energy)

    @property
    def sampling_rate(self) -> int:
        return self.wav2win.sampling_rate

    @property
    def frame_length(self) -> Seconds:
        return self.wav2win.frame_length

    @property
    def frame_shift(self) -> Seconds:
        return self.wav2win.frame_shift

    @property
    def remove_dc_offset(self) -> bool:
        return self.wav2win.remove_dc_offset

    @property
    def preemph_coeff(self) -> float:
        return self.wav2win.preemph_coeff

    @property
    def window_type(self) -> str:
        return self.wav2win.window_type

    @property
    def dither(self) -> float:
        return self.wav2win.dither

    def _complex(self, out: torch.Tensor, squeeze: bool) -> torch.Tensor:
        """Rows of ``fft_length + 2`` floats as ``fft_length / 2 + 1`` complex bins."""
        spec = torch.view_as_complex(out.view(out.shape[0], out.shape[1], self.fft_length // 2 + 1, 2))
        return spec[0] if squeeze else spec

    def forward(self, x: torch.Tensor, lengths=None, padding_value: float = 0.0):
        """``forward(x)``: the ``complex64`` STFT of equally long rows.  ``forward(x, lengths, padding_value=0.0)``: the ragged batch of
        ``_HipLayer.forward`` -- ``(spectrum, out_lens)`` with ``spectrum[b, T_b:]`` equal to ``padding_value + 0j``; a device ``lengths``
        tensor is copied to the host once (a synchronisation); ``dither`` is drawn for the whole ``(B, Smax)`` tensor and only each row's
        first ``lengths[b]`` samples of it are read."""
        if lengths is not None:
            out, _, out_lens = self.wav2win._run_ragged(x, lengths, padding_value, _lib.STFT_SPECTRUM, self)
            return self._complex(out, False), out_lens
        out, _, squeeze = self.wav2win._run(x, _lib.STFT_SPECTRUM, self)  # (refusals name this layer)
        return self._complex(out, squeeze)

    def online_inference(self, x: torch.Tensor, context: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The reference's chunked, stateless streaming call (layers.py:326-333): ``(spectrum, remainder)``, the ``complex64`` STFT of the
        complete frames of ``[context | x]`` and the samples they did not consume; see ``HipWav2Win.online_inference``, whose framing,
        remainder and zero-frame rule (``(B, 0, fft_length / 2 + 1)`` where the reference raises) this shares."""
        out, _, remainder, squeeze = self.wav2win._online(x, context, _lib.STFT_SPECTRUM, self)
        return self._complex(out, squeeze), remainder
