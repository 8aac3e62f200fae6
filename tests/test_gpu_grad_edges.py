"""GPU: the launch edges of the waveform gradient (csrc/kernel_grad.hpp, ``hipfeat_grad_run``) that tests/test_gpu_grad.py leaves out.

1. the scalar head and tail of ``grad_overlap_add_kernel``: rows that start 0 to 3 floats past a 16-byte boundary, bit for bit against the
   row alone, also under piecewise launches on a strided view of a leaf (``row_stride != S``);
2. nothing is written outside the gradient rows and the reported workspace, with ``grad_wave_stride != S``;
3. rows one frame longer than one and two workgroups' 32 frames in the spectral modes;
4. the refusals of the layers in differentiable mode.
"""
import warnings

import numpy as np
import pytest
import torch

import _grad_ref as GR
import lhotse_amd as LA
from lhotse_amd import _lib
from lhotse_amd import layers as LY
from test_gpu_grad import cotangents, held_to_autograd, signal

pytestmark = pytest.mark.gpu


def shapes_of(cls, kw, x):
    return [tuple(o.shape) for o in GR.outputs(GR.forward(cls, kw, torch.from_numpy(x)))]


# ---- 1. head and tail bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["Wav2LogFilterBank", "Wav2FFT"])
@pytest.mark.parametrize("S", [1501, 1502, 1503])
def test_rows_that_start_off_a_16_byte_boundary_have_the_bits_of_the_row_alone(cls, S, monkeypatch):
    B, kw = 5, dict(use_energy=True)
    heads = {(b * S) % 4 for b in range(B)}
    assert heads == ({0, 2} if S % 2 == 0 else {0, 1, 2, 3})  # where a row of the (B, S) gradient starts, in floats past a 16-byte boundary
    x = signal(100 + S, B, S)
    cots = cotangents(9, cls, shapes_of(cls, kw, x))
    layer = GR.hip_layer(cls, kw)
    whole = GR.device_gradient(layer, x, cots)
    assert np.isfinite(whole).all()
    for b in range(B):
        alone = GR.device_gradient(layer, x[b:b + 1], [c[b:b + 1] for c in cots])
        assert np.array_equal(alone[0], whole[b]), (b, (b * S) % 4)
    # piecewise launches on a strided row view of a leaf: row_stride = S + 7, rows_per_piece 1 and 2 (a last piece of one row)
    T, nr = cots[0].shape[1], 400
    wide = np.zeros((B, S + 7), dtype=np.float32)
    wide[:, 3:3 + S] = x
    for budget, pieces in ((T * nr * 4, 5), (2 * T * nr * 4 + 4, 3)):
        monkeypatch.setattr(LY, "_GRAD_WORKSPACE_BYTES", budget)
        assert -(-B // max(1, budget // (T * nr * 4))) == pieces
        leaf = torch.from_numpy(wide).cuda().requires_grad_(True)
        view = leaf[:, 3:3 + S]
        assert view.stride(0) == S + 7
        outs = GR.outputs(layer(view))
        torch.autograd.backward(list(outs), [torch.from_numpy(c).cuda() for c in cots])
        g = leaf.grad.cpu().numpy()
        assert np.array_equal(g[:, 3:3 + S], whole), budget
        assert not g[:, :3].any() and not g[:, 3 + S:].any()


# ---- 2. nothing outside the outputs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["fbank", "spectrum", "frames-401"])
def test_nothing_is_written_outside_the_gradient_rows_and_the_reported_workspace(which):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    B, S, n, shift = 3, 1100, 400, 160
    if which == "fbank":
        cls, kw = "Wav2LogFilterBank", dict()
        layer = GR.hip_layer(cls, kw)
        grad, width = layer._grad_for(dev), 80
    elif which == "spectrum":
        cls, kw = "Wav2FFT", dict()
        layer = GR.hip_layer(cls, kw)
        grad, width = layer.wav2win._grad_for(dev, _lib.STFT_SPECTRUM, layer), 514
    else:
        cls, kw = "Wav2Win", dict(pad_length=401, return_log_energy=True)
        layer = GR.hip_layer(cls, kw)
        grad, width = layer._grad_for(dev, _lib.STFT_FRAMES, layer), 401
    T = GR.num_frames(S, n, shift, False)
    x = signal(61, B, S)
    cots = cotangents(6, cls, shapes_of(cls, kw, x))
    want = GR.device_gradient(layer, x, cots)
    assert np.isfinite(want).all() and want.all()

    sizes = np.zeros(2, dtype=np.int64)
    assert lib.raw("hipfeat_grad_workspace", grad.handle, B, S, 1 << 30, sizes.ctypes.data, sizes.ctypes.data + 8) == 0
    assert (int(sizes[0]), int(sizes[1])) == (B, B * T * n)  # Nr == N == 400
    assert lib.raw("hipfeat_grad_workspace", grad.handle, B, S, 1, sizes.ctypes.data, sizes.ctypes.data + 8) == 0
    assert (int(sizes[0]), int(sizes[1])) == (1, T * n)

    xt = torch.from_numpy(x).cuda()
    c0 = torch.from_numpy(cots[0]).cuda()
    c0 = (torch.view_as_real(c0) if c0.is_complex() else c0).contiguous()  # the spectrum's cotangent: interleaved (re, im) pairs
    assert c0.numel() == B * T * width
    c1 = torch.from_numpy(cots[1]).cuda() if len(cots) > 1 else None
    stream = int(torch.cuda.current_stream().cuda_stream)
    guard, stride, behind = 1027, S + 3, 1024  # an odd guard and an odd stride: the rows start 3, 2 and 1 floats past a 16-byte boundary
    for ws_floats in (B * T * n, T * n):  # all rows in one piece; one row per piece
        gbuf = torch.full((guard + B * stride + behind,), float("nan"), device="cuda")
        ws = torch.full((ws_floats + behind,), float("nan"), device="cuda")
        assert ws.data_ptr() % 16 == 0 and {((gbuf.data_ptr() // 4) + guard + b * stride) % 4 for b in range(B)} == {3, 2, 1}
        status = lib.raw("hipfeat_grad_run", grad.handle, xt.data_ptr(), B, S, S, c0.data_ptr(), c0.numel(), None if c1 is None else c1.data_ptr(),
                         gbuf.data_ptr() + 4 * guard, stride, ws.data_ptr(), ws_floats, stream)
        assert status == 0, lib.last_error()
        torch.cuda.synchronize()
        assert gbuf[:guard].isnan().all() and gbuf[guard + B * stride:].isnan().all()
        rows = gbuf[guard:guard + B * stride].view(B, stride)
        assert rows[:, S:].isnan().all() and not rows[:, :S].isnan().any()
        assert np.array_equal(rows[:, :S].cpu().numpy(), want), ws_floats
        assert ws[ws_floats:].isnan().all() and not ws[:ws_floats].isnan().any()


# ---- 3. rows longer than a workgroup's frames, spectral modes ----------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["Wav2FFT", "Wav2MFCC"])
@pytest.mark.parametrize("T", [33, 65])
def test_rows_one_frame_past_one_and_two_workgroups_at_8k(cls, T):
    kw = dict(sampling_rate=8000)
    n, shift, fft = GR.sizes(kw, cls)
    S = T * shift
    assert (n, shift, fft) == (200, 80, 256) and GR.num_frames(S, n, shift, False) == T and T % 32 == 1
    held_to_autograd(f"{cls} T={T}", cls, kw, signal(T, 2, S))


# ---- 4. refusals at the layer ------------------------------------------------------------------------------------------------------------
def make(cls, differentiable, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return getattr(LA, "Hip" + cls)(**kw).differentiable_(differentiable)


@pytest.mark.parametrize("cls", ["Wav2Win", "Wav2FFT", "Wav2LogFilterBank"])
def test_a_shift_longer_than_the_frame_is_refused_by_the_first_differentiable_call(cls):
    kw = dict(frame_length=0.025, frame_shift=0.03, snip_edges=True)
    x = torch.from_numpy(signal(2, 2, 1500)).cuda()
    layer = make(cls, True, **kw)
    with pytest.raises(NotImplementedError, match=r"frame_shift \(480\) > frame_length \(400\).*frame_shift <= frame_length"):
        layer(x.clone().requires_grad_(True))
    if cls != "Wav2LogFilterBank":  # (the feature plans never had such a shift; the frames and the spectrum go on serving it)
        out = GR.outputs(layer(x))[0]
        assert out.shape == (2, 3, 400 if cls == "Wav2Win" else 257) and not out.requires_grad


@pytest.mark.parametrize("cls", ["Wav2LogFilterBank", "Wav2MFCC"])
def test_more_than_128_filters_are_refused_by_the_first_differentiable_call(cls):
    layer = make(cls, True, num_filters=129)
    x = torch.from_numpy(signal(3, 2, 1000)).cuda()
    with pytest.raises(NotImplementedError, match="num_filters = 129.*at most 128 mel filters"):
        layer(x.clone().requires_grad_(True))
    assert layer(x).shape == (2, 6, 129 if cls == "Wav2LogFilterBank" else 13)


def test_a_frame_of_2049_samples_is_refused_by_the_first_differentiable_call():
    kw = dict(sampling_rate=2049, frame_length=1.0, frame_shift=0.5)
    layer = make("Wav2Win", True, **kw)
    assert (layer._length, layer._shift) == (2049, 1024)
    x = torch.from_numpy(signal(4, 2, 5000)).cuda()
    with pytest.raises(NotImplementedError, match="frame_length = 2049.*frames of at most 2048 samples"):
        layer(x.clone().requires_grad_(True))
    ok = make("Wav2Win", True, sampling_rate=2048, frame_length=1.0, frame_shift=0.5)  # 2048 samples: the largest frame there is
    held_to_autograd("Wav2Win N=2048", "Wav2Win", dict(sampling_rate=2048, frame_length=1.0, frame_shift=0.5), signal(5, 2, 5000))
    assert GR.outputs(ok(x))[0].shape == (2, 5, 2048)
