"""GPU: ``HipWav2Win`` / ``HipWav2FFT`` (hipfeat_stft_*, csrc/kernel_stft.hpp) against the reference's float32 call sequence (``ref32``) and the
float64 truth on the same samples (tests/_stft_ref.py, where the two bars are stated), at the smallest shapes that can go wrong."""
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

import _stft_ref as R
import lhotse_amd as LA
from lhotse_amd import _lib

pytestmark = pytest.mark.gpu
RATE_IDS = [str(r[0]) for r in R.RATES]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stft.npz")


def win_layer(cfg, pad):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the snip_edges warning has its own test)
        return LA.HipWav2Win(pad_length=pad, return_log_energy=cfg.use_energy, **R.layer_kwargs(cfg))


def fft_layer(cfg):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LA.HipWav2FFT(use_energy=cfg.use_energy, **R.layer_kwargs(cfg))


def check(label, cfg, x, pads, xt=None, worst=None):
    """Both layers on x (xt: the device tensor to feed, default a fresh copy of x) against ref32 and the truth, to both bars."""
    xt = torch.from_numpy(x).cuda() if xt is None else xt
    n, shift, fft = R.K.window_sizes(cfg)
    T = R.K.num_frames(x.shape[1], n, shift, cfg.snip_edges)
    y = fft_layer(cfg)(xt)
    assert y.is_cuda and y.dtype == torch.complex64 and tuple(y.shape) == (x.shape[0], T, fft // 2 + 1)
    _, _, r_spec = R.ref32(x, cfg)
    _, _, t_spec = R.truth(x, cfg)
    errs = [R.hold(f"{label} spectrum", y.cpu().numpy(), r_spec, t_spec, energy_bin=cfg.use_energy)]
    for pad in pads:
        frames, log_e = win_layer(cfg, pad)(xt)
        assert frames.is_cuda and frames.dtype == torch.float32 and tuple(frames.shape) == (x.shape[0], T, pad)
        r_frames, _, _ = R.ref32(x, cfg, pad)
        t_frames, t_log_e, _ = R.truth(x, cfg, pad)
        errs.append(R.hold(f"{label} frames pad {pad}", frames.cpu().numpy(), r_frames, t_frames))
        assert (log_e is None) == (not cfg.use_energy)
        if log_e is not None:
            assert log_e.dtype == torch.float32 and tuple(log_e.shape) == (x.shape[0], T)
            R.hold_energy(f"{label} log-energy pad {pad}", log_e.cpu().numpy(), t_log_e)
    if worst is not None:
        worst.extend(ey / er for ey, er in errs if er > 0)
    return y


@pytest.mark.parametrize("rate,n,fft", R.RATES, ids=RATE_IDS)
def test_every_option_against_the_reference_and_the_truth(rate, n, fft):
    worst = []
    for i, cfg in enumerate(R.option_grid(rate)):
        _, shift, _ = R.K.window_sizes(cfg)
        all_lengths = R.lengths(n, shift, cfg.snip_edges)
        x = R.signal(i, 1 + 2 * (i % 2), all_lengths[i % len(all_lengths)])
        check(f"{rate} #{i} {cfg.window_type} snip {int(cfg.snip_edges)} dc {int(cfg.remove_dc_offset)} pre {cfg.preemph_coeff} raw {int(cfg.raw_energy)} "
              f"energy {int(cfg.use_energy)} x{x.shape}", cfg, x, (n, n + 1, fft), worst=worst)
    print(f"[stft] {rate}: worst E(device) / E(ref32) over the option grid: {max(worst):.3g}")


@pytest.mark.parametrize("rate,n,fft", R.RATES, ids=RATE_IDS)
def test_every_edge_length_and_batch_size(rate, n, fft):
    for k, snip in enumerate((False, True)):
        cfg = R.config(rate, snip_edges=snip, raw_energy=not snip)
        _, shift, _ = R.K.window_sizes(cfg)
        for j, S in enumerate(R.lengths(n, shift, snip)):
            for B in (1, 3):
                check(f"{rate} snip {int(snip)} S {S} B {B}", cfg, R.signal(100 * k + j, B, S), (n + 1,))


@pytest.mark.parametrize("rate,n,fft", R.RATES, ids=RATE_IDS)
def test_the_shortest_row_one_below_it_no_frames_and_no_rows(rate, n, fft):
    cfg = R.config(rate)
    _, shift, _ = R.K.window_sizes(cfg)
    shortest = R.shortest_reflectable(n, shift)
    check(f"{rate} shortest S {shortest}", cfg, R.signal(1, 2, shortest), (n, n + 1))
    below = torch.from_numpy(R.signal(2, 2, shortest - 1)).cuda()
    with pytest.raises(ValueError):
        R.truth(below.cpu().numpy(), cfg)
    for layer in (fft_layer(cfg), win_layer(cfg, n + 1)):
        with pytest.raises(ValueError, match="TOO_SHORT"):
            layer(below)
    # snip_edges with fewer samples than a frame: no frames, (B, 0, width)
    snip = R.config(rate, snip_edges=True)
    short = torch.from_numpy(R.signal(3, 3, n - 1)).cuda()
    assert tuple(fft_layer(snip)(short).shape) == (3, 0, fft // 2 + 1)
    frames, log_e = win_layer(snip, n + 1)(short)
    assert tuple(frames.shape) == (3, 0, n + 1) and tuple(log_e.shape) == (3, 0)
    # B = 0
    none = torch.zeros((0, 5 * shift), device="cuda")
    assert tuple(fft_layer(cfg)(none).shape) == (0, 5, fft // 2 + 1)
    frames, log_e = win_layer(cfg, n)(none)
    assert tuple(frames.shape) == (0, 5, n) and tuple(log_e.shape) == (0, 5)


@pytest.mark.parametrize("rate,n,fft", R.RATES, ids=RATE_IDS)
def test_an_offset_view_a_strided_batch_and_a_non_contiguous_input(rate, n, fft):
    cfg = R.config(rate)
    _, shift, _ = R.K.window_sizes(cfg)
    B, S = 3, 3 * shift + shift // 2 - 1
    x = R.signal(7, B, S)
    # a batch that starts one element into its storage: a 4-byte-aligned base
    store = torch.zeros(B * S + 1, device="cuda")
    store[1:] = torch.from_numpy(x.reshape(-1)).cuda()
    view = store[1:].view(B, S)
    assert view.data_ptr() % 8 == 4
    a = check(f"{rate} offset view", cfg, x, (n + 1,), xt=view)
    # rows with a stride of their own (read in place), and every second column of a wider tensor (copied)
    wide = torch.full((B, S + 5), 9.0, device="cuda")
    wide[:, 2:S + 2] = torch.from_numpy(x).cuda()
    b = check(f"{rate} row stride", cfg, x, (n + 1,), xt=wide[:, 2:S + 2])
    twice = torch.full((B, 2 * S), 9.0, device="cuda")
    twice[:, ::2] = torch.from_numpy(x).cuda()
    assert not twice[:, ::2].is_contiguous()
    c = check(f"{rate} non-contiguous", cfg, x, (n + 1,), xt=twice[:, ::2])
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)) and torch.equal(torch.view_as_real(a), torch.view_as_real(c))


@pytest.mark.parametrize("rate,n,fft", R.RATES, ids=RATE_IDS)
def test_an_all_zero_row_gives_zeros_and_the_floor(rate, n, fft):
    for raw in (True, False):
        cfg = R.config(rate, raw_energy=raw)
        _, shift, _ = R.K.window_sizes(cfg)
        x = R.signal(9, 3, 5 * shift)
        x[1] = 0.0
        xt = torch.from_numpy(x).cuda()
        y = check(f"{rate} zero row raw {int(raw)}", cfg, x, (n, n + 1, fft), xt=xt)
        frames, log_e = win_layer(cfg, n + 1)(xt)
        r_frames, r_log_e, _ = R.ref32(x, cfg, n + 1)
        assert not frames[1].any() and not r_frames[1].any()
        spec = torch.view_as_real(y[1])
        assert not spec[:, 1:].any() and not spec[:, 0, 1].any()  # bin 0 holds (log-energy, 0)
        floor = np.float32(np.log(cfg.energy_floor))
        assert (r_log_e[1] == floor).all()  # the floor the reference gives
        assert np.abs(log_e[1].cpu().numpy().astype(np.float64) - float(floor)).max() <= 1e-4
        assert np.abs(spec[:, 0, 0].cpu().numpy().astype(np.float64) - float(floor)).max() <= 1e-4
        cfg0 = R.config(rate, raw_energy=raw, want_energy=False)
        assert not torch.view_as_real(fft_layer(cfg0)(xt)[1]).any()


@pytest.mark.parametrize("rate,n,fft", R.RATES, ids=RATE_IDS)
def test_one_row_equals_its_row_of_the_batch_and_runs_repeat_bit_for_bit(rate, n, fft):
    cfg = R.config(rate)
    _, shift, _ = R.K.window_sizes(cfg)
    xt = torch.from_numpy(R.signal(13, 3, 37 * shift + 5)).cuda()  # (more than one workgroup per row)
    for layer in (fft_layer(cfg), win_layer(cfg, n + 1), win_layer(cfg, fft)):
        first, again, one = layer(xt), layer(xt), layer(xt[0])
        for a, b, c in zip(*[(o if isinstance(o, tuple) else (o,)) for o in (first, again, one)]):
            a, b, c = [torch.view_as_real(v) if v.is_complex() else v for v in (a, b, c)]
            assert torch.equal(a, b) and torch.equal(c, a[0]) and c.shape == a.shape[1:]


@pytest.mark.parametrize("rate,n,fft", R.RATES, ids=RATE_IDS)
def test_the_power_of_the_spectrum_is_the_spectrogram_layer(rate, n, fft):
    for kw in ({}, {"use_energy": False, "window_type": "hamming", "snip_edges": True}):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            stft, spec = LA.HipWav2FFT(sampling_rate=rate, **kw), LA.HipWav2Spec(sampling_rate=rate, **kw)
        x = R.signal(17, 2, 5 * n)
        xt = torch.from_numpy(x).cuda()
        X, P = stft(xt), spec(xt).cpu().numpy().astype(np.float64)
        mine = (X.abs() ** 2).cpu().numpy().astype(np.float64)
        cfg = R.config(rate, want_energy=kw.get("use_energy", True), **{k: v for k, v in kw.items() if k != "use_energy"})
        t = np.abs(R.truth(x, cfg)[2]) ** 2
        first = 1 if cfg.use_energy else 0  # bin 0 holds the log-energy in both
        if first:
            assert np.abs(X[:, :, 0].real.cpu().numpy() - P[:, :, 0]).max() <= 1e-4 and not X[:, :, 0].imag.any()
        tol = 1e-4 * t[:, :, first:].max(axis=2, keepdims=True) + 1e-7
        assert (np.abs(mine[:, :, first:] - t[:, :, first:]) <= tol).all() and (np.abs(P[:, :, first:] - t[:, :, first:]) <= tol).all()
        assert (np.abs(mine[:, :, first:] - P[:, :, first:]) <= 2 * tol).all()


SENTINEL = 12345.0


@pytest.mark.parametrize("rate,n,fft", R.RATES, ids=RATE_IDS)
def test_nothing_is_written_next_to_the_output_and_run_refuses_before_launching(rate, n, fft):
    lib = _lib.load()
    cfg = R.config(rate)
    _, shift, _ = R.K.window_sizes(cfg)
    B, S, T = 2, 3 * shift, 3
    x = R.signal(19, B, S)
    xt = torch.from_numpy(x).cuda()
    stream = int(torch.cuda.current_stream().cuda_stream)
    # (output, pad, guard floats in front): odd rows behind an odd guard, so that no row of the frames starts on a 16-byte boundary twice
    for output, pad, guard in ((_lib.STFT_SPECTRUM, fft, 1026), (_lib.STFT_FRAMES, n + 1, 1027), (_lib.STFT_FRAMES, n, 1025), (_lib.STFT_FRAMES, fft, 1026)):
        layer = win_layer(cfg, pad)
        handle = layer._handle_for(xt.device, output)
        width = pad + 2 if output == _lib.STFT_SPECTRUM else pad
        need = B * T * width
        buf = torch.full((guard + need + 1024,), SENTINEL, device="cuda")
        energies = torch.full((64 + B * T + 64,), SENTINEL, device="cuda")
        out_ptr, e_ptr = buf.data_ptr() + 4 * guard, energies.data_ptr() + 4 * 64
        # refusals: nothing is launched
        assert lib.raw("hipfeat_stft_run", handle.handle, xt.data_ptr(), B, S, S, out_ptr, need - 1, e_ptr, stream) == _lib.ERR_INVALID
        assert lib.raw("hipfeat_stft_run", handle.handle, xt.data_ptr(), B, S, S - 1, out_ptr, need, e_ptr, stream) == _lib.ERR_INVALID
        assert lib.raw("hipfeat_stft_run", handle.handle, xt.data_ptr(), B, S, S, None, need, e_ptr, stream) == _lib.ERR_INVALID
        assert lib.raw("hipfeat_stft_run", handle.handle, xt.data_ptr(), -1, S, S, out_ptr, need, e_ptr, stream) == _lib.ERR_INVALID
        assert lib.raw("hipfeat_stft_run", handle.handle, xt.data_ptr(), B, S, S, out_ptr + 2, need, e_ptr, stream) == _lib.ERR_INVALID
        if output == _lib.STFT_SPECTRUM:
            assert lib.raw("hipfeat_stft_run", handle.handle, xt.data_ptr(), B, S, S, out_ptr + 4, need, e_ptr, stream) == _lib.ERR_INVALID
        assert lib.raw("hipfeat_stft_run", handle.handle, xt.data_ptr(), B, 20, 20, out_ptr, need, e_ptr, stream) == _lib.ERR_TOO_SHORT
        assert lib.raw("hipfeat_stft_run", handle.handle, xt.data_ptr(), 0, S, S, out_ptr, 0, e_ptr, stream) == 0
        torch.cuda.synchronize()
        assert (buf == SENTINEL).all() and (energies == SENTINEL).all()
        lib.check("hipfeat_stft_run", handle.handle, xt.data_ptr(), B, S, S, out_ptr, need, e_ptr, stream)
        torch.cuda.synchronize()
        assert (buf[:guard] == SENTINEL).all() and (buf[guard + need:] == SENTINEL).all()
        assert (energies[:64] == SENTINEL).all() and (energies[64 + B * T:] == SENTINEL).all()
        got = buf[guard: guard + need].view(B, T, width).cpu()
        if output == _lib.STFT_SPECTRUM:
            want = torch.view_as_real(fft_layer(cfg)(xt)).reshape(B, T, width).cpu()
            assert torch.equal(got, want) and torch.equal(energies[64: 64 + B * T].view(B, T).cpu()[:, :], want[:, :, 0])
        else:
            frames, log_e = layer(xt)
            assert torch.equal(got, frames.cpu()) and torch.equal(energies[64: 64 + B * T].view(B, T).cpu(), log_e.cpu())
        # d_log_energy may be NULL
        buf.fill_(SENTINEL)
        lib.check("hipfeat_stft_run", handle.handle, xt.data_ptr(), B, S, S, out_ptr, need, None, stream)
        torch.cuda.synchronize()
        assert torch.equal(buf[guard: guard + need].view(B, T, width).cpu(), got) and (buf[:guard] == SENTINEL).all() and (buf[guard + need:] == SENTINEL).all()


def test_a_run_on_another_stream():
    cfg = R.config(16000)
    x = R.signal(23, 3, 20 * 160 + 3)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        xt = torch.from_numpy(x).cuda()
        y = check("side stream", cfg, x, (401,), xt=xt)
    side.synchronize()
    assert torch.equal(torch.view_as_real(y), torch.view_as_real(fft_layer(cfg)(xt)))


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_the_goldens_of_the_live_layers(name):
    arrays = np.load(GOLDEN)
    cfg, pad, x = R.golden_case(name)
    assert np.array_equal(arrays[f"{name}/x"], x)
    xt = torch.from_numpy(arrays[f"{name}/x"]).cuda()
    t_frames, t_log_e, _ = R.truth(x, cfg, pad)
    _, _, t_spec = R.truth(x, cfg)
    R.hold(f"golden {name} spectrum", fft_layer(cfg)(xt).cpu().numpy(), arrays[f"{name}/spectrum"], t_spec, energy_bin=cfg.use_energy)
    frames, log_e = win_layer(cfg, pad)(xt)
    R.hold(f"golden {name} frames", frames.cpu().numpy(), arrays[f"{name}/frames"], t_frames)
    if cfg.use_energy:
        R.hold_energy(f"golden {name} log-energy", log_e.cpu().numpy(), t_log_e)
        R.hold_energy(f"golden {name} stored log-energy", arrays[f"{name}/log_energy"], t_log_e)
    else:
        assert log_e is None and f"{name}/log_energy" not in arrays


def test_argument_checks_unsupported_sizes_dither_and_pickle():
    x = torch.from_numpy(R.signal(29, 2, 16000)).cuda()
    for layer in (LA.HipWav2Win(), LA.HipWav2FFT()):
        with pytest.raises(_lib.HipFeatError, match="no CPU fallback|'cuda"):
            layer(x.cpu())
        with pytest.raises(NotImplementedError, match="inference-only"):
            layer(x.clone().requires_grad_(True))
        with torch.no_grad():
            layer(x.clone().requires_grad_(True))
        with pytest.raises(ValueError):
            layer(torch.zeros(1, 50, device="cuda"))
    # sizes without a device FFT: refused, naming the switch and the size; the frames of the same sizes are served
    for kw, size in (({"round_to_power_of_two": False}, 400), ({"sampling_rate": 4000}, 128), ({"frame_length": 0.05, "sampling_rate": 48000}, 4096)):
        with pytest.raises(NotImplementedError, match=f"round_to_power_of_two(.|\n)*{size}"):
            LA.HipWav2FFT(**kw)(x)
    with pytest.raises(NotImplementedError, match="2400"):
        LA.HipWav2Win(sampling_rate=48000, frame_length=0.05)(x)
    frames, log_e = LA.HipWav2Win(sampling_rate=4000)(x)
    assert tuple(frames.shape) == (2, 400, 100) and log_e is None
    # dither: torch.randn on the device in front of the launch
    quiet, noisy = LA.HipWav2FFT(dither=0.0), LA.HipWav2FFT(dither=1.0)
    torch.manual_seed(3)
    a = noisy(x)
    torch.manual_seed(3)
    b = noisy(x)
    torch.manual_seed(3)
    want = quiet(x + 1.0 * torch.randn(x.shape, device=x.device))
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)) and torch.equal(torch.view_as_real(a), torch.view_as_real(want))
    assert not torch.equal(torch.view_as_real(a), torch.view_as_real(quiet(x)))
    # handles are per device and lazy, and dropped on pickle
    fresh = LA.HipWav2FFT()
    assert fresh.wav2win._handles == {}
    first = fresh(x)
    assert len(fresh.wav2win._handles) == 1
    again = pickle.loads(pickle.dumps(fresh))
    assert again.wav2win._handles == {} and torch.equal(torch.view_as_real(again(x)), torch.view_as_real(first))
    win = pickle.loads(pickle.dumps(LA.HipWav2Win(return_log_energy=True)))
    frames, log_e = win(x[0])
    assert tuple(frames.shape) == (100, 400) and tuple(log_e.shape) == (100,)
