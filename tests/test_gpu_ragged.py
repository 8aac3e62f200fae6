"""GPU: ``forward(x, lengths, padding_value)`` of the six ``HipWav2*`` layers and its waveform gradient (hipfeat_stft_run_ragged,
hipfeat_grad_run_ragged, the plans' collated launch; csrc/kernel_stft.hpp ``RaggedRowSource``).

Row ``b`` of a ragged batch is the waveform ``x[b, :lengths[b]]`` and nothing else.  The lengths sit at the launch's edges: ``Smax``,
``Smax - 1``, the length whose frame count is exactly one workgroup's (4 waves x 8 frames), that length plus one shift, and the shortest
legal row.  Each row is held (1) bit for bit to the uniform call on the row alone, forward and gradient, and (2) to the float64
restatement ``_grad_ref.forward`` directly, with the bars of tests/test_gpu_layers.py (the four feature kinds), tests/_stft_ref.py (frames,
spectrum) and tests/_grad_ref.py (the gradient); then padding, reads outside the row, zero-frame rows, layout, determinism and the
argument checks."""
import functools
import warnings

import numpy as np
import pytest
import torch

import _grad_ref as G
import _stft_ref as R
import lhotse_amd as LA
from lhotse_amd import layers as LY
from lhotse_amd.compat import LOG_EPSILON

pytestmark = pytest.mark.gpu

BLOCK_FRAMES = 32  # 4 waves x kStftFramesPerWave = 8 frames per workgroup
KW = {"Wav2Win": dict(return_log_energy=True)}  # (every other class at its defaults; Wav2FFT / Spec / LogSpec carry the log-energy in bin 0)
RATES = {256: 8000, 512: 16000, 1024: 22050, 2048: 44100}


def config(cls, snip, fft=512):
    kw = dict(KW.get(cls, {}), snip_edges=snip)
    if fft != 512:
        kw["sampling_rate"] = RATES[fft]
    if cls == "Wav2Win" and fft != 512:
        kw["pad_length"] = fft
    return kw


def edge_lengths(n, shift, snip):
    """(Smax, the five lengths of the module docstring)."""
    if snip:
        block, short = n + (BLOCK_FRAMES - 1) * shift, n
    else:
        block, short = BLOCK_FRAMES * shift, R.shortest_reflectable(n, shift)
        lib = LA._lib.load()  # ... which is the smallest length hipfeat_check_length passes
        assert lib.raw("hipfeat_check_length", short, n, shift, 0) == 0 and lib.raw("hipfeat_check_length", short - 1, n, shift, 0) != 0
    smax = block + 3 * shift + shift // 2 + 7
    lens = [smax, smax - 1, block, block + shift, short]
    assert G.num_frames(block, n, shift, snip) == BLOCK_FRAMES and G.num_frames(block + shift, n, shift, snip) == BLOCK_FRAMES + 1
    return smax, lens


def signal(seed, B, S, rate):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-0.5, 0.5, size=(B, S)) + 0.25 * np.sin(2 * np.pi * 440.0 * np.arange(S) / rate + rng.rand(B, 1))
    return x.astype(np.float32)


def cotangents(seed, cls, shapes):
    rng = np.random.RandomState(seed)
    out = []
    for shape in shapes:
        c = rng.randint(-8, 9, size=shape).astype(np.float32) / 8.0
        if cls == "Wav2FFT":
            c = (c + 1j * (rng.randint(-8, 9, size=shape).astype(np.float32) / 8.0)).astype(np.complex64)
        out.append(c)
    return out


def run_ragged(layer, x, lens, cots=None, padding_value=0.0, xt=None):
    """(outputs as a tuple of device tensors, out_lens, x.grad or None).  ``xt``: the device tensor to feed instead of a copy of ``x``."""
    xt = torch.from_numpy(x).cuda() if xt is None else xt
    if cots is not None:
        xt.requires_grad_(True)
    res, out_lens = layer(xt, lens, padding_value)
    outs = G.outputs(res)
    if cots is None:
        return outs, out_lens, None
    torch.autograd.backward(list(outs), [torch.as_tensor(c).cuda() for c in cots])
    return tuple(o.detach() for o in outs), out_lens, xt.grad


def run_alone(layer, row, cots=None):
    """The uniform call on one row alone, (1, S_b)."""
    xt = torch.from_numpy(np.ascontiguousarray(row)).cuda()
    if cots is not None:
        xt.requires_grad_(True)
    outs = G.outputs(layer(xt))
    if cots is None:
        return outs, None
    torch.autograd.backward(list(outs), [torch.as_tensor(np.ascontiguousarray(c)).cuda() for c in cots])
    return tuple(o.detach() for o in outs), xt.grad


@functools.lru_cache(maxsize=None)
def case(cls, snip, fft=512):
    """One ragged batch at the edge lengths, computed once and shared: the layer, x, the lengths, the cotangents, and the device's outputs
    and gradient."""
    kw = config(cls, snip, fft)
    n, shift, _ = G.sizes(kw, cls)
    smax, lens = edge_lengths(n, shift, snip)
    x = signal(fft + 7 * len(cls) + snip, len(lens), smax, kw.get("sampling_rate", 16000))
    layer = G.hip_layer(cls, kw)
    outs, out_lens, _ = run_ragged(layer, x, lens)
    cots = cotangents(11 + fft + snip, cls, [tuple(o.shape) for o in outs])
    outs2, _, grad = run_ragged(layer, x, lens, cots)
    for a, b in zip(outs, outs2):
        assert torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b)  # the same launch, with or without a graph
    T = [G.num_frames(s, n, shift, snip) for s in lens]
    assert out_lens.dtype == torch.int64 and out_lens.device.type == "cpu" and out_lens.tolist() == T
    assert all(o.shape[:2] == (len(lens), max(T)) for o in outs)
    return dict(kw=kw, layer=layer, x=x, lens=lens, T=T, cots=cots, outs=outs, grad=grad, n=n, shift=shift)


def bits(t):
    t = t.detach()
    return torch.view_as_real(t).contiguous() if t.is_complex() else t.contiguous()


SIX = [(cls, snip, 512) for cls in G.CLASSES for snip in (False, True)]
SIZES = [(cls, False, fft) for fft in (256, 1024, 2048) for cls in ("Wav2Win", "Wav2FFT", "Wav2LogFilterBank")]
IDS = [f"{c}-snip{int(s)}-fft{f}" for c, s, f in SIX + SIZES]


@pytest.mark.parametrize("cls,snip,fft", SIX + SIZES, ids=IDS)
def test_a_row_equals_the_row_alone_bit_for_bit(cls, snip, fft):
    c = case(cls, snip, fft)
    for b, (s, t) in enumerate(zip(c["lens"], c["T"])):
        outs, grad = run_alone(c["layer"], c["x"][b: b + 1, :s], [k[b: b + 1, :t] for k in c["cots"]])
        for got, want in zip(c["outs"], outs):
            assert torch.equal(bits(got[b, :t]), bits(want[0])), (cls, snip, fft, b, "forward")
        assert torch.equal(c["grad"][b, :s], grad[0]), (cls, snip, fft, b, "gradient")


def hold_features(cls, kw, got, want):
    """The bars of tests/test_gpu_layers.py for one row of a feature kind (got float32, want float64, both (T, F))."""
    assert got.shape == want.shape
    if cls == "Wav2Spec":
        tol = np.broadcast_to(1e-4 * np.abs(want[:, 1:]).max(axis=1, keepdims=True) + 1e-7, want.shape).copy()
        if kw.get("use_energy", True):
            tol[:, 0] = 1e-4
        assert np.all(np.abs(got - want) <= tol)
    elif cls == "Wav2MFCC":
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-4
    else:
        err = np.abs(got - want)
        loud = want >= want.max(axis=1, keepdims=True) - 14.0
        assert err[loud].max() <= 2e-4, err[loud].max()
        assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-4


@pytest.mark.parametrize("cls,snip,fft", SIX + SIZES, ids=IDS)
def test_every_row_is_held_to_the_float64_restatement(cls, snip, fft):
    c = case(cls, snip, fft)
    kw = c["kw"]
    for b, (s, t) in enumerate(zip(c["lens"], c["T"])):
        row = c["x"][b: b + 1, :s]
        label = f"ragged {cls} snip {int(snip)} fft {fft} row {b} (S {s}, T {t})"
        t64 = G.outputs(G.forward(cls, kw, torch.from_numpy(row).double()))
        r32 = G.outputs(G.forward(cls, kw, torch.from_numpy(row)))
        for i, (got, want, ref) in enumerate(zip(c["outs"], t64, r32)):
            got, want, ref = got[b: b + 1, :t].cpu().numpy(), want.numpy(), ref.numpy()
            if cls in ("Wav2Win", "Wav2FFT"):
                if i == 1:
                    R.hold_energy(label + " log-energy", got, want)
                else:
                    R.hold(label, got, ref, want, energy_bin=(cls == "Wav2FFT"))
            else:
                hold_features(cls, kw, got[0], want[0])
        cots = [k[b: b + 1, :t] for k in c["cots"]]
        g64, g32 = G.gradient(cls, kw, row, cots, torch.float64), G.gradient(cls, kw, row, cots, torch.float32)
        G.hold(label, c["grad"][b: b + 1, :s].cpu().numpy(), g32, g64)


@pytest.mark.parametrize("padding_value", [0.0, LOG_EPSILON, -1.5])
@pytest.mark.parametrize("cls", G.CLASSES)
def test_padding_rows_hold_the_padding_value_and_the_gradient_tail_is_plus_zero(cls, padding_value):
    c = case(cls, False)
    shapes = [tuple(o.shape) for o in c["outs"]]
    poison = [torch.full(s, float("nan"), device="cuda", dtype=o.dtype) for s, o in zip(shapes, c["outs"])]  # what the allocator hands out next
    del poison
    outs, _, grad = run_ragged(c["layer"], c["x"], c["lens"], c["cots"], padding_value)
    pv = np.float32(padding_value)
    for o, clean in zip(outs, c["outs"]):
        o = bits(o)
        assert torch.isfinite(o).all()
        for b, t in enumerate(c["T"]):
            assert torch.equal(o[b, :t], bits(clean)[b, :t])
            pad = o[b, t:]
            if pad.numel() and c["outs"][0].is_complex():
                assert (pad[..., 0] == float(pv)).all() and (pad[..., 1].view(torch.int32) == 0).all()
            else:
                assert (pad == float(pv)).all()
    assert torch.equal(grad, c["grad"])  # the padding value is not part of the gradient
    for b, s in enumerate(c["lens"]):
        assert (grad[b, s:].view(torch.int32) == 0).all()  # +0.0: the sign bit clear


@pytest.mark.parametrize("cls", G.CLASSES)
def test_nothing_outside_the_row_is_read(cls):
    c = case(cls, False)
    x = c["x"].copy()
    cots = [k.copy() for k in c["cots"]]
    for b, (s, t) in enumerate(zip(c["lens"], c["T"])):
        x[b, s:] = np.nan
        for k in cots:
            k[b, t:] = np.nan
    outs, _, grad = run_ragged(c["layer"], x, c["lens"], cots)
    for o, clean in zip(outs, c["outs"]):
        assert torch.equal(bits(o), bits(clean))
    assert torch.equal(grad, c["grad"])


@pytest.mark.parametrize("cls", G.CLASSES)
def test_zero_frame_rows_and_layout(cls):
    kw = config(cls, True)
    n, shift, _ = G.sizes(kw, cls)
    layer = G.hip_layer(cls, kw)
    smax = n + 40 * shift + 3
    lens = [0, smax, n - 1, n, smax - shift]
    x = signal(5, len(lens), smax, 16000)
    outs, out_lens, _ = run_ragged(layer, x, lens)
    T = [G.num_frames(s, n, shift, True) for s in lens]
    assert out_lens.tolist() == T and T[0] == T[2] == 0 and T[3] == 1
    cots = cotangents(3, cls, [tuple(o.shape) for o in outs])
    outs, _, grad = run_ragged(layer, x, lens, cots, -1.5)
    for o in outs:
        o = bits(o)
        assert (o[0] == -1.5).all() or o.shape[-1] == 2 and (o[0][..., 0] == -1.5).all() and (o[0][..., 1] == 0).all()
        assert torch.equal(o[0], o[2])
    assert (grad[0].view(torch.int32) == 0).all() and (grad[2].view(torch.int32) == 0).all()
    alone, g1 = run_alone(layer, x[1:2], [k[1:2] for k in cots])
    assert torch.equal(bits(outs[0][1]), bits(alone[0][0])) and torch.equal(grad[1], g1[0])
    # a batch of only such rows: (B, 0, width), nothing launched, an all-zero gradient
    none, lens0, _ = run_ragged(layer, x[:3], [0, n - 1, 5])
    assert lens0.tolist() == [0, 0, 0] and all(tuple(o.shape[:2]) == (3, 0) for o in none) and none[0].shape[-1] == outs[0].shape[-1]
    xt = torch.from_numpy(x[:3]).cuda().requires_grad_(True)
    res, _ = layer(xt, [0, n - 1, 5])
    torch.autograd.backward(list(G.outputs(res)), [torch.zeros_like(o) for o in G.outputs(res)])
    assert xt.grad.shape == (3, smax) and (xt.grad.view(torch.int32) == 0).all()
    # a non-contiguous x (row stride > Smax, base offset of one float) gives the bits of the contiguous one
    base = torch.zeros(len(lens) * (smax + 5) + 1, device="cuda")
    view = base[1:].view(len(lens), smax + 5)[:, :smax]
    view.copy_(torch.from_numpy(x))
    assert not view.is_contiguous() and view.storage_offset() == 1 and view.stride(0) == smax + 5
    leaf = base.requires_grad_(True)
    view = leaf[1:].view(len(lens), smax + 5)[:, :smax]
    res, _ = layer(view, lens, -1.5)
    strided = G.outputs(res)
    torch.autograd.backward(list(strided), [torch.as_tensor(k).cuda() for k in cots])
    for a, b in zip(strided, outs):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(leaf.grad[1:].view(len(lens), smax + 5)[:, :smax], grad)
    # a 1-D x with a one-element lengths is the batch of one row
    one, one_lens, _ = run_ragged(layer, x[1], [smax - shift], xt=torch.from_numpy(x[1]).cuda())
    two, _, _ = run_ragged(layer, x[1:2], [smax - shift])
    assert one_lens.tolist() == [T[4]] and all(torch.equal(bits(a), bits(b)) for a, b in zip(one, two))


@pytest.mark.parametrize("cls", G.CLASSES)
def test_pieces_and_row_order_do_not_change_a_bit(cls, monkeypatch):
    c = case(cls, False)
    nr = (c["n"] + 3) & ~3
    perm = [3, 0, 4, 2, 1]
    x, lens, cots = c["x"][perm], [c["lens"][i] for i in perm], [k[perm] for k in c["cots"]]
    with monkeypatch.context() as m:
        m.setattr(LY, "_GRAD_WORKSPACE_BYTES", max(c["T"]) * nr * 4)  # one row per piece: five pieces
        _, _, pieces = run_ragged(c["layer"], c["x"], c["lens"], c["cots"])
        outs, out_lens, grad = run_ragged(c["layer"], x, lens, cots)
    assert torch.equal(pieces, c["grad"])
    assert out_lens.tolist() == [c["T"][i] for i in perm]
    for o, clean in zip(outs, c["outs"]):
        assert torch.equal(bits(o), bits(clean)[perm])
    assert torch.equal(grad, c["grad"][perm])


@pytest.mark.parametrize("cls", G.CLASSES)
def test_argument_checks(cls):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        layer = getattr(LA, "Hip" + cls)(**KW.get(cls, {}))
    x = torch.from_numpy(signal(1, 3, 4000, 16000)).cuda()
    for bad in ([4000, 4000], [4000, 4000, 4000, 4000], [[4000, 4000, 4000]], [4000, -1, 4000], [4000, 4001, 4000]):
        with pytest.raises(ValueError):
            layer(x, bad)
    for bad in (torch.tensor([4000.0, 3000.0, 2000.0]), np.array([4000.0, 3000.0, 2000.0]), [4000.0, 3000, 2000], torch.tensor([True, True, False])):
        with pytest.raises(TypeError):
            layer(x, bad)
    with pytest.raises(ValueError, match="row 1"):
        layer(x, [4000, 50, 4000])  # too short for its reflection (snip_edges=False)
    with pytest.raises(ValueError, match="row 2"):
        layer(x, [4000, 4000, 0])
    dev = torch.tensor([4000, 3999, 1600], dtype=torch.int32, device="cuda")
    res, out_lens = layer(x, dev)
    assert out_lens.dtype == torch.int32 and out_lens.device == dev.device and out_lens.tolist() == [25, 25, 10]
    host, host_lens = layer(x, np.array([4000, 3999, 1600], dtype=np.int16), 0.0)
    assert host_lens.dtype == torch.int64 and host_lens.device.type == "cpu" and host_lens.tolist() == [25, 25, 10]
    for a, b in zip(G.outputs(res), G.outputs(host)):
        assert torch.equal(bits(a), bits(b))
    if cls == "Wav2Win":
        assert isinstance(res, tuple) and len(res) == 2 and res[0].shape == (3, 25, 400) and res[1].shape == (3, 25)
    plain = layer(x)  # lengths=None returns what it returned before
    assert isinstance(plain, tuple) == (cls == "Wav2Win") and G.outputs(plain)[0].shape[:2] == (3, 25)
    assert not isinstance(layer(x, None), tuple) or cls == "Wav2Win"
    for a, b in zip(G.outputs(plain), G.outputs(layer(x, [4000, 4000, 4000])[0])):
        assert torch.equal(bits(a), bits(b))
    layer.differentiable_()
    with pytest.raises(NotImplementedError, match="inference-only"):
        layer.online_inference(x.clone().requires_grad_(True))
