"""GPU: ``differentiable_()`` of the six ``HipWav2*`` layers -- the waveform gradient of csrc/kernel_grad.hpp.

The goldens (tests/golden/grad.npz) are the live reference's autograd in float32 and float64; everywhere else the device is held to the
autograd of ``_grad_ref.forward`` (tests/test_grad_reference.py holds that restatement to the same goldens) with the same bar:
per row E(device) <= max(2 E(float32 autograd), 1e-6) against the float64 gradient, and exact zeros where the float64 gradient is zero.
"""
import warnings

import numpy as np
import pytest
import torch

import _grad_ref as GR
import _stft_ref as SR
import lhotse_amd as LA
from lhotse_amd import layers as LY

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return GR.load_golden()


def cotangents(seed, cls, shapes):
    rng = np.random.RandomState(seed)
    out = []
    for shape in shapes:
        c = rng.standard_normal(shape).astype(np.float32)
        if cls == "Wav2FFT":
            c = (c + 1j * rng.standard_normal(shape).astype(np.float32)).astype(np.complex64)
        out.append(c)
    return out


def signal(seed, B, S):
    rng = np.random.RandomState(seed)
    t = np.arange(S)
    return (rng.uniform(-0.5, 0.5, size=(B, S)) + 0.25 * np.sin(2 * np.pi * t / 37.0 + rng.rand(B, 1))).astype(np.float32)


def poison(shape):
    """Allocate and free a NaN-filled tensor of the gradient's size, so that an element the launches do not write shows."""
    t = torch.full(shape, float("nan"), device="cuda")
    del t


def held_to_autograd(label, cls, kw, x, seed=3):
    """The device gradient of one layer on ``x`` under the bar, against the autograd of the restatement; returns it."""
    shapes = [tuple(o.shape) for o in GR.outputs(GR.forward(cls, kw, torch.from_numpy(x)))]
    cots = cotangents(seed, cls, shapes)
    g64, g32 = GR.gradient(cls, kw, x, cots, torch.float64), GR.gradient(cls, kw, x, cots, torch.float32)
    poison(x.shape)
    g = GR.device_gradient(GR.hip_layer(cls, kw), x, cots)
    GR.hold(label, g, g32, g64)
    return g


# ---- 1. goldens ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GR.CASES))
def test_goldens(gold, name):
    cls, kw = GR.CASES[name]
    x, g32, g64 = gold[f"{name}/x"], gold[f"{name}/g32"], gold[f"{name}/g64"]
    assert np.array_equal(x, GR.case_input(name)) and not x[1].any()
    poison(x.shape)
    g = GR.device_gradient(GR.hip_layer(cls, kw), x, GR.golden_cotangents(gold, name))
    worst = GR.hold(name, g, g32, g64)
    print(f"[grad] {name}: worst E(device) / E(g32) where the reference's error sets the bar: {worst:.3g}")
    if cls not in ("Wav2Win", "Wav2FFT"):  # the silent row of every non-linear kind
        assert not g64[1].any() and not g[1].any()


# ---- 2. forward unchanged ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", GR.CLASSES)
def test_the_differentiable_forward_is_the_plain_forward(cls):
    kw = dict(return_log_energy=True) if cls == "Wav2Win" else {}
    x = torch.from_numpy(signal(5, 2, 1000)).cuda()
    plain = getattr(LA, "Hip" + cls)(**kw)
    with pytest.raises(NotImplementedError, match="inference-only"):
        plain(x.clone().requires_grad_(True))
    layer = GR.hip_layer(cls, kw)
    assert layer.differentiable and not plain.differentiable
    want = GR.outputs(plain(x))
    got = GR.outputs(layer(x.clone().requires_grad_(True)))
    assert all(g.requires_grad for g in got)
    for a, b in zip(want, got):
        assert torch.equal(a, b.detach())
    # the flag on and no gradient asked for, or no_grad: the plain path
    for res in (layer(x), ):
        assert all(not o.requires_grad and torch.equal(o, w) for o, w in zip(GR.outputs(res), want))
    with torch.no_grad():
        assert all(not o.requires_grad and torch.equal(o, w) for o, w in zip(GR.outputs(layer(x.clone().requires_grad_(True))), want))
    # online_inference keeps refusing, and differentiable_(False) restores the refusal of forward
    with pytest.raises(NotImplementedError, match="inference-only"):
        layer.online_inference(x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="inference-only"):
        layer.differentiable_(False)(x.clone().requires_grad_(True))


# ---- 3. adjoint identity on the linear kinds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GR.LINEAR)
def test_adjoint_identity(gold, name):
    cls, kw = GR.CASES[name]
    x, cots = gold[f"{name}/x"], GR.golden_cotangents(gold, name)
    layer = GR.hip_layer(cls, kw)
    with torch.no_grad():
        outs = [o.cpu() for o in GR.outputs(layer(torch.from_numpy(x).cuda()))]
    fwd = float(GR.pairing(outs, cots, torch.float64))
    g = GR.device_gradient(layer, x, cots)
    back = float((x.astype(np.float64) * g.astype(np.float64)).sum())
    gap, ref = abs(fwd - back) / abs(fwd), float(gold[f"{name}/gap32"])
    print(f"[grad] {name}: <forward(x), c> {fwd:.9g}  <x, backward(c)> {back:.9g}  gap {gap:.3g}  reference's float32 gap {ref:.3g}")
    assert gap <= max(2.0 * ref, 1e-6)


# ---- 4. edge lengths ---------------------------------------------------------------------------------------------------------------------
N16, SHIFT16 = 400, 160
EDGE_LENGTHS = sorted({SR.shortest_reflectable(N16, SHIFT16), N16, N16 + 1})


@pytest.mark.parametrize("cls", ["Wav2LogFilterBank", "Wav2FFT", "Wav2Win"])
@pytest.mark.parametrize("S", EDGE_LENGTHS)
def test_edge_lengths_at_16k(cls, S):
    """The shortest row whose single frame reflects at both ends onto the same samples, S = N and S = N + 1."""
    kw = dict(use_energy=True) if cls == "Wav2LogFilterBank" else (dict(return_log_energy=True) if cls == "Wav2Win" else dict(use_energy=False))
    held_to_autograd(f"{cls} S={S}", cls, kw, signal(S, 2, S))


@pytest.mark.parametrize("S,sign", [(5 * 320 + 100, -1), (5 * 320 + 40, 0), (5 * 320 + 10, 1)])
def test_the_sign_of_the_right_reflection(S, sign):
    """npad_right = (T - 1) shift + N - S - npad_left below, at and above zero.  (At the default shift of 160 it is always positive: a 20 ms
    shift, npad_left = 40, has all three.)"""
    n, shift = 400, 320
    T = (S + shift // 2) // shift
    right = (T - 1) * shift + n - S - (n - shift) // 2
    assert np.sign(right) == sign
    g = held_to_autograd(f"npad_right={right}", "Wav2LogFilterBank", dict(frame_shift=0.02), signal(S, 2, S))
    if right < 0:  # the last -npad_right samples are read by no frame
        assert not g[:, S + right:].any() and g[:, : S + right].all()


def test_snip_edges_leaves_the_unused_tail_at_exactly_zero():
    S = N16 + 3 * SHIFT16 + 57
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g = held_to_autograd("snip tail", "Wav2LogFilterBank", dict(snip_edges=True), signal(9, 2, S))
    tail = g[:, S - 57:]
    assert tail.shape[1] == 57 and not tail.any() and not np.signbit(tail).any() and g[:, : S - 57].all()


# ---- 5. overlap multiplicity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift_s,contributors", [(0.001, 25), (0.025, 1), (0.01, 3)])
def test_overlap_multiplicity(shift_s, contributors):
    assert -(-N16 // int(shift_s * 16000)) == contributors
    held_to_autograd(f"shift {shift_s}", "Wav2LogFilterBank", dict(frame_shift=shift_s), signal(21, 2, 1234))
    held_to_autograd(f"shift {shift_s} frames", "Wav2Win", dict(frame_shift=shift_s), signal(22, 2, 1234))


# ---- 6. FFT sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,fft", [(8000, 256), (16000, 512), (22050, 1024), (44100, 2048)])
def test_fft_sizes(rate, fft):
    S = 700 * rate // 16000
    for cls, kw in (("Wav2Spec", dict(sampling_rate=rate)), ("Wav2MFCC", dict(sampling_rate=rate, use_energy=True))):
        assert GR.sizes(kw, cls)[2] == fft
        held_to_autograd(f"{cls} fft {fft}", cls, kw, signal(fft, 2, S))


@pytest.mark.parametrize("cls", ["Wav2FFT", "Wav2Spec", "Wav2LogSpec", "Wav2LogFilterBank", "Wav2MFCC"])
def test_a_size_without_a_gradient_kernel_is_refused_by_the_first_differentiable_call(cls):
    layer = GR.hip_layer(cls, dict(round_to_power_of_two=False))
    x = torch.from_numpy(signal(1, 2, 1000)).cuda()
    with pytest.raises(NotImplementedError, match="256, 512, 1024 and 2048"):
        layer(x.clone().requires_grad_(True))
    if cls not in ("Wav2FFT",):
        assert layer(x).shape[0] == 2  # the plain forward goes on serving it


# ---- 7. bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["Wav2LogFilterBank", "Wav2FFT"])
def test_the_gradient_of_a_row_is_the_same_bits_in_any_batch_run_and_piece_size(cls, monkeypatch):
    kw = dict(use_energy=True)
    x = signal(77, 5, 1500)
    shapes = [tuple(o.shape) for o in GR.outputs(GR.forward(cls, kw, torch.from_numpy(x)))]
    cots = cotangents(8, cls, shapes)
    layer = GR.hip_layer(cls, kw)
    whole = GR.device_gradient(layer, x, cots)
    assert np.array_equal(whole, GR.device_gradient(layer, x, cots))  # two runs
    alone = GR.device_gradient(layer, x[2:3], [c[2:3] for c in cots])
    assert np.array_equal(alone[0], whole[2])  # a row alone and in a batch of 5
    T, nr = shapes[0][1], 400
    for budget in (T * nr * 4, 2 * T * nr * 4 + 4, 16):  # one row per piece, two (a last piece of one), less than a single row
        monkeypatch.setattr(LY, "_GRAD_WORKSPACE_BYTES", budget)
        assert np.array_equal(whole, GR.device_gradient(layer, x, cots)), budget


# ---- 8. call shapes ----------------------------------------------------------------------------------------------------------------
def test_call_shapes():
    kw = dict()
    layer = GR.hip_layer("Wav2LogFilterBank", kw)
    base = torch.from_numpy(signal(31, 3, 2400)).cuda()

    def grad_of(x, pick=lambda y: y):
        x = x.detach().requires_grad_(True)
        y = pick(layer(x))
        w = torch.linspace(-1.0, 1.0, y.numel(), device="cuda").reshape(y.shape)
        (y * w).sum().backward()
        return x.grad

    dense = base[:, ::2].contiguous()
    want = grad_of(dense)
    leaf = base.clone().requires_grad_(True)  # a non-contiguous view of a leaf: the gradient arrives in the leaf's even samples
    y = layer(leaf[:, ::2])
    (y * torch.linspace(-1.0, 1.0, y.numel(), device="cuda").reshape(y.shape)).sum().backward()
    assert torch.equal(leaf.grad[:, ::2], want) and not leaf.grad[:, 1::2].any()
    leaf = base.clone().requires_grad_(True)  # a strided row view
    y = layer(leaf[:, 100:1300])
    (y * torch.linspace(-1.0, 1.0, y.numel(), device="cuda").reshape(y.shape)).sum().backward()
    assert torch.equal(leaf.grad[:, 100:1300], grad_of(base[:, 100:1300].contiguous())) and not leaf.grad[:, :100].any() and not leaf.grad[:, 1300:].any()
    # 1-D
    one = grad_of(dense[1])
    assert one.shape == dense[1].shape and torch.equal(one, grad_of(dense[1:2])[0])
    # B = 0
    empty = torch.zeros((0, 1200), device="cuda", requires_grad=True)
    y = layer(empty)
    y.sum().backward()
    assert y.shape[0] == 0 and empty.grad.shape == (0, 1200)
    # a non-contiguous cotangent: a loss on y[..., ::2]
    g = grad_of(dense, lambda y: y[..., ::2])
    x64 = dense.cpu().numpy()
    shapes = [tuple(o.shape) for o in GR.outputs(GR.forward("Wav2LogFilterBank", kw, torch.from_numpy(x64)))]
    cot = np.zeros(shapes[0], dtype=np.float32)
    cot[..., ::2] = np.linspace(-1.0, 1.0, cot[..., ::2].size, dtype=np.float32).reshape(cot[..., ::2].shape)
    GR.hold("loss on y[..., ::2]", g.cpu().numpy(), GR.gradient("Wav2LogFilterBank", kw, x64, [cot], torch.float32), GR.gradient("Wav2LogFilterBank", kw, x64, [cot]))


def test_either_cotangent_of_the_frames_may_be_none():
    kw = dict(return_log_energy=True)
    layer = GR.hip_layer("Wav2Win", kw)
    x = signal(41, 2, 1100)
    shapes = [tuple(o.shape) for o in GR.outputs(GR.forward("Wav2Win", kw, torch.from_numpy(x)))]
    both = cotangents(4, "Wav2Win", shapes)
    for cots in ([both[0], None], [None, both[1]], both):
        g = GR.device_gradient(layer, x, cots)
        GR.hold(f"frames cotangents {[c is not None for c in cots]}", g, GR.gradient("Wav2Win", kw, x, cots, torch.float32), GR.gradient("Wav2Win", kw, x, cots))
    # an output that does not reach the loss at all
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    frames, log_e = layer(xt)
    (log_e * 2.0).sum().backward()
    assert torch.isfinite(xt.grad).all() and xt.grad.any()


def test_a_complex_loss_on_the_spectrum():
    kw = dict(use_energy=False)
    layer = GR.hip_layer("Wav2FFT", kw)
    x = signal(43, 2, 1100)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    (layer(xt).abs() ** 2).sum().backward()  # the power spectrum through torch's own complex autograd
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    (GR.forward("Wav2FFT", kw, x64).abs() ** 2).sum().backward()
    x32 = torch.from_numpy(x).requires_grad_(True)
    (GR.forward("Wav2FFT", kw, x32).abs() ** 2).sum().backward()
    GR.hold("sum |X|^2", xt.grad.cpu().numpy(), x32.grad.numpy(), x64.grad.numpy())


# ---- 9. dither ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["Wav2LogFilterBank", "Wav2Win", "Wav2FFT"])
def test_dither_is_added_in_front_and_the_gradient_passes_through_it(cls):
    x = torch.from_numpy(signal(51, 2, 1000)).cuda()
    dithered, plain = GR.hip_layer(cls, dict(dither=0.25)), GR.hip_layer(cls, dict())

    def run(layer, inp):
        inp = inp.detach().requires_grad_(True)
        outs = GR.outputs(layer(inp))
        sum((o.abs() ** 2).sum() for o in outs).backward()
        return [o.detach() for o in outs], inp.grad

    torch.manual_seed(7)
    outs, g = run(dithered, x)
    torch.manual_seed(7)
    noise = torch.randn(x.shape, device=x.device)
    outs0, g0 = run(plain, x + 0.25 * noise)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs0)) and torch.equal(g, g0)
