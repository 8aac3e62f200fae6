"""GPU: ``online_inference`` of the six layers (hipfeat_stream_*, csrc/kernel_stream.hpp) against the statements of tests/_stream_ref.py on the
virtual waveform ``V = [A | x]`` of every call, at the smallest shapes that can go wrong.

Chunking invariance and the start of a stream.  Without ``snip_edges`` the first call reflects ``min(P, S)`` samples, so a stream whose first
chunk is shorter than P has ANOTHER V than the same samples fed as one chunk, in the reference as here: the three chunkings of the
invariance test can agree bit for bit only where they frame the same V.  They are therefore run as stated -- a first chunk shorter than P
included -- on the ``snip_edges=True`` layers, and on the default layers with a first chunk of exactly P samples (the shortest that
reflects what one chunk reflects); the default layers' stream with a first chunk shorter than P is held, bit for bit, to one call on its own
V with the flipped head passed as a caller-made context.
"""
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

import _stft_ref as R
import _stream_ref as SR
import lhotse_amd as LA
from lhotse_amd import _lib
from test_gpu_layers import CASES

pytestmark = pytest.mark.gpu
RATE_IDS = [str(r[0]) for r in R.RATES]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream.npz")


def make(name, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the snip_edges warning has its own test)
        return getattr(LA, "Hip" + name)(**kw)


def win_layer(cfg, pad):
    return make("Wav2Win", pad_length=pad, return_log_energy=cfg.use_energy, **R.layer_kwargs(cfg))


def fft_layer(cfg):
    return make("Wav2FFT", use_energy=cfg.use_energy, **R.layer_kwargs(cfg))


def real(t):
    return torch.view_as_real(t) if t.is_complex() else t


def sizes_of(layer):
    w = layer if isinstance(layer, LA.HipWav2Win) else getattr(layer, "wav2win", None)
    return (w._length, w._shift) if w is not None else (layer._n, layer._shift)


def run_stream(layer, x, sizes, context=None):
    """Feeds the chunks of x (a device tensor) through online_inference -> (per call outputs, per call remainders); Wav2Win outputs are tuples."""
    outs, rems, at = [], [], 0
    for s in sizes:
        out, context = layer.online_inference(x[:, at:at + s], context)
        outs.append(out)
        rems.append(context)
        at += s
    assert at == x.shape[1]
    return outs, rems


def joined(outs):
    """Concatenated along the frames; Wav2Win: (frames, log-energies or None)."""
    if isinstance(outs[0], tuple):
        return torch.cat([o[0] for o in outs], dim=1), (None if outs[0][1] is None else torch.cat([o[1] for o in outs], dim=1))
    return torch.cat([real(o) for o in outs], dim=1), None


def chunk_plan(n, shift, first_head, frames=(1, 31, 0, 32, 33)):
    """Chunk lengths that give the calls `frames` frames: L = N + (k - 1) s + d for k frames (d < s varies), L = N - 1 for none."""
    sizes, rem = [], None
    for i, k in enumerate(frames):
        L = n - 1 if k == 0 else n + (k - 1) * shift + (5 + 37 * i) % shift
        have = first_head if rem is None else rem
        assert L - have >= (first_head if rem is None else 0)
        sizes.append(L - have)
        rem = L - k * shift
    return sizes


@pytest.mark.parametrize("rate,n,fft", R.RATES, ids=RATE_IDS)
def test_win_and_fft_every_option_at_the_workgroup_edges_and_without_frames(rate, n, fft):
    grid = list(R.option_grid(rate))[::11]
    assert {c.snip_edges for c in grid} == {False, True} and {c.remove_dc_offset for c in grid} == {False, True}
    assert {c.preemph_coeff for c in grid} == {0.0, 0.97} and len({c.window_type for c in grid}) >= 3
    assert {c.raw_energy for c in grid} == {False, True} and {c.use_energy for c in grid} == {False, True}
    worst = []
    for i, cfg in enumerate(grid):
        _, shift, _ = R.K.window_sizes(cfg)
        head = 0 if cfg.snip_edges else (n - shift) // 2
        sizes = chunk_plan(n, shift, head)
        x = R.signal(i, 3, sum(sizes))
        xt = torch.from_numpy(x).cuda()
        pad = (n, n + 1, fft)[i % 3]
        calls = SR.walk(x, sizes, n, shift, cfg.snip_edges)
        assert [c[3] for c in calls] == [1, 31, 0, 32, 33]
        spectra, rems_f = run_stream(fft_layer(cfg), xt, sizes)
        windows, rems_w = run_stream(win_layer(cfg, pad), xt, sizes)
        for j, (chunk, _, V, T, remainder) in enumerate(calls):
            label = f"{rate} #{i} call {j} T {T} {cfg.window_type} snip {int(cfg.snip_edges)} dc {int(cfg.remove_dc_offset)} pre {cfg.preemph_coeff}"
            y, (frames, log_e) = spectra[j], windows[j]
            assert y.is_cuda and y.dtype == torch.complex64 and tuple(y.shape) == (3, T, fft // 2 + 1)
            assert frames.dtype == torch.float32 and tuple(frames.shape) == (3, T, pad)
            assert (log_e is None) == (not cfg.use_energy) and (log_e is None or tuple(log_e.shape) == (3, T))
            for rem in (rems_f[j], rems_w[j]):
                assert rem.is_contiguous() and torch.equal(rem.cpu(), torch.from_numpy(remainder)), label
            if T == 0:
                continue
            worst.append(R.hold(f"{label} spectrum", y.cpu().numpy(), SR.ref32(V, cfg)[2], SR.truth(V, cfg)[2], energy_bin=cfg.use_energy))
            t_frames, t_log_e, _ = SR.truth(V, cfg, pad)
            worst.append(R.hold(f"{label} frames pad {pad}", frames.cpu().numpy(), SR.ref32(V, cfg, pad)[0], t_frames))
            if log_e is not None:
                R.hold_energy(f"{label} log-energy", log_e.cpu().numpy(), t_log_e)
    print(f"[stream] {rate}: worst E(device) / E(ref32): {max(ey / er for ey, er in worst if er > 0):.3g}")


@pytest.mark.parametrize("cls,kind,kw", CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(CASES)])
def test_feature_layers_streamed_in_three_chunks_match_the_oracle(cls, kind, kw):
    layer = make(cls[3:], **kw)
    cfg, kind_ = SR.feature_config(layer)
    assert kind_ == kind
    n, shift = sizes_of(layer)
    sizes = (n + 7 * shift + 3, 13 * shift + 1, 17 * shift + 5)
    x = R.signal(len(cls) + len(kw), 2, sum(sizes))
    outs, rems = run_stream(layer, torch.from_numpy(x).cuda(), sizes)
    calls = SR.walk(x, sizes, n, shift, cfg.snip_edges)
    for out, rem, (_, _, V, T, remainder) in zip(outs, rems, calls):
        assert torch.equal(rem.cpu(), torch.from_numpy(remainder))
        assert out.is_cuda and out.dtype == torch.float32 and T >= 7
        want = SR.features_truth(V, cfg)
        got = out.cpu().numpy().astype(np.float64)
        assert got.shape == want.shape
        for b in range(2):
            SR.hold_features(kind, cfg.use_energy, got[b], want[b])


INVARIANCE = [("Wav2Win", dict(pad_length=401, return_log_energy=True)), ("Wav2FFT", {}), ("Wav2Spec", {}), ("Wav2LogSpec", {}),
              ("Wav2LogFilterBank", {}), ("Wav2MFCC", {})]


def irregular(total, first, shift):
    """A fixed irregular chunking: `first`, a 1-sample chunk, small and large chunks, a 0-sample chunk in the middle."""
    sizes = [first, 1, 37, 0, 3 * shift + 11, shift - 1, 1, 0, 7 * shift]
    rest = total - sum(sizes)
    assert rest > 0
    return sizes + [rest]


@pytest.mark.parametrize("snip", (False, True), ids=("reflect", "snip"))
@pytest.mark.parametrize("name,kw", INVARIANCE, ids=[c[0] for c in INVARIANCE])
def test_the_output_of_a_stream_does_not_depend_on_the_chunking(name, kw, snip):
    layer = make(name, snip_edges=snip, **kw)
    n, shift = sizes_of(layer)
    p = (n - shift) // 2
    total = 70 * shift + 77
    x = torch.from_numpy(R.signal(31, 2, total)).cuda()
    # snip_edges: a first chunk shorter than P; without it exactly P, so that the three chunkings frame the same V (module docstring)
    chunkings = [[total], [shift] * 70 + [77], irregular(total, p - 9 if snip else p, shift)]
    results = [run_stream(layer, x, sizes) for sizes in chunkings]
    (a, ea), ra = joined(results[0][0]), results[0][1][-1]
    assert 68 <= a.shape[1] <= 70  # 1 + (L - N) // shift with L = 70 shifts + 77 (+ P when the head is reflected)
    for outs, rems in results[1:]:
        b, eb = joined(outs)
        assert torch.equal(a, b) and torch.equal(ra, rems[-1]) and ((ea is None and eb is None) or torch.equal(ea, eb))
    if name in ("Wav2Win", "Wav2FFT"):  # ... and they are `forward` of the snip_edges twin on V
        V = x if snip else torch.cat((torch.flip(x[:, :p], (1,)), x), dim=1)
        twin = make(name, snip_edges=True, **kw)(V)
        frames, log_e = twin if isinstance(twin, tuple) else (real(twin), None)
        assert torch.equal(a, frames) and (log_e is None or torch.equal(ea, log_e))
    if not snip:
        # a first chunk shorter than P reflects only what it has: the same bits as one call on that V, the head given as a context
        short = p - 9
        outs, rems = run_stream(layer, x, irregular(total, short, shift))
        one, rem1 = layer.online_inference(x, torch.flip(x[:, :short], (1,)).contiguous())
        (b, eb), (c, ec) = joined(outs), joined([one])
        assert torch.equal(b, c) and torch.equal(rems[-1], rem1) and ((eb is None and ec is None) or torch.equal(eb, ec))
        assert b.shape[1] == a.shape[1] and not torch.equal(a[:, 0], b[:, 0])  # (another head: another first frame)


@pytest.mark.parametrize("name,kw", INVARIANCE, ids=[c[0] for c in INVARIANCE])
def test_seams_a_long_caller_made_context_and_strided_views(name, kw):
    layer = make(name, **kw)
    n, shift = sizes_of(layer)
    R_, S = 2 * n + 3, n + 2 * shift + 1  # frames wholly in the context, across the seam, wholly in the chunk
    context, x = R.signal(41, 3, R_), R.signal(42, 3, S)
    V = np.concatenate([context, x], axis=1)
    T, remainder = SR.split(V, n, shift)
    starts = np.arange(T) * shift
    assert (starts + n <= R_).sum() >= 2 and ((starts < R_) & (starts + n > R_)).sum() >= 2 and (starts >= R_).sum() >= 1
    ct, xt = torch.from_numpy(context).cuda(), torch.from_numpy(x).cuda()
    out, rem = layer.online_inference(xt, ct)
    assert torch.equal(rem.cpu(), torch.from_numpy(remainder))
    if name == "Wav2Win":
        cfg = R.config(16000, True)
        R.hold("seam frames", out[0].cpu().numpy(), SR.ref32(V, cfg, 401)[0], SR.truth(V, cfg, 401)[0])
        R.hold_energy("seam log-energy", out[1].cpu().numpy(), SR.truth(V, cfg, 401)[1])
    elif name == "Wav2FFT":
        cfg = R.config(16000, True)
        R.hold("seam spectrum", out.cpu().numpy(), SR.ref32(V, cfg)[2], SR.truth(V, cfg)[2], energy_bin=True)
    else:
        cfg, kind = SR.feature_config(layer)
        want = SR.features_truth(V, cfg)
        for b in range(3):
            SR.hold_features(kind, cfg.use_energy, out[b].cpu().numpy().astype(np.float64), want[b])
    a, ea = joined([out])
    # the same V with the seam elsewhere (odd and even offsets, an empty context, an empty chunk): the same bits
    Vt = torch.from_numpy(V).cuda()
    for cut in (0, 1, n - 1, n, R_ + 1, R_ + 2, V.shape[1] - 1, V.shape[1]):
        o2, r2 = layer.online_inference(Vt[:, cut:].contiguous(), Vt[:, :cut].contiguous())
        b, eb = joined([o2])
        assert torch.equal(a, b) and torch.equal(rem, r2) and ((ea is None and eb is None) or torch.equal(ea, eb)), cut
    # column slices of wider tensors: row stride > length, first element at an odd float offset
    wide_c = torch.full((3, R_ + 8), 9.0, device="cuda")
    wide_x = torch.full((3, S + 6), 9.0, device="cuda")
    wide_c[:, 3:R_ + 3], wide_x[:, 1:S + 1] = ct, xt
    vc, vx = wide_c[:, 3:R_ + 3], wide_x[:, 1:S + 1]
    assert vc.data_ptr() % 8 == 4 and vx.data_ptr() % 8 == 4 and vc.stride(0) > R_ and vx.stride(0) > S
    o3, r3 = layer.online_inference(vx, vc)
    b, eb = joined([o3])
    assert torch.equal(a, b) and torch.equal(rem, r3) and ((ea is None and eb is None) or torch.equal(ea, eb))
    # every second column of a wider tensor (copied before the launch)
    twice = torch.full((3, 2 * S), 9.0, device="cuda")
    twice[:, ::2] = xt
    o4, r4 = layer.online_inference(twice[:, ::2], ct)
    assert torch.equal(a, joined([o4])[0]) and torch.equal(rem, r4)


@pytest.mark.parametrize("which", ("frames-401", "spectrum", "fbank"))
def test_nothing_is_written_outside_the_three_outputs_and_run_refuses_before_launching(which):
    lib = _lib.load()
    n, shift, B = 400, 160, 2
    if which == "frames-401":
        layer = make("Wav2Win", pad_length=401, return_log_energy=True)
        handle, width, energies = layer._stream_for(torch.device("cuda", 0), _lib.STFT_FRAMES, layer), 401, True
    elif which == "spectrum":
        layer = make("Wav2FFT")
        handle, width, energies = layer.wav2win._stream_for(torch.device("cuda", 0), _lib.STFT_SPECTRUM, layer), 514, False
    else:
        layer = make("Wav2LogFilterBank")
        handle, width, energies = layer._stream_for(torch.device("cuda", 0)), 80, False
    R_, S = n - shift + 7, 2 * shift + 30
    T, rem = SR.counts(R_ + S, n, shift)
    assert handle.counts(False, R_, S) == (T, rem) and T == 2
    ct, xt = torch.from_numpy(R.signal(51, B, R_)).cuda(), torch.from_numpy(R.signal(52, B, S)).cuda()
    stream = int(torch.cuda.current_stream().cuda_stream)
    guard = 1027 if which == "frames-401" else 1026  # odd rows behind an odd guard: no row of the frames starts on a 16-byte boundary twice
    need, need_r = B * T * width, B * rem
    buf = torch.full((guard + need + 1024,), float("nan"), device="cuda")
    en = torch.full((64 + B * T + 64,), float("nan"), device="cuda")
    rm = torch.full((65 + need_r + 64,), float("nan"), device="cuda")
    out_ptr, e_ptr, r_ptr = buf.data_ptr() + 4 * guard, en.data_ptr() + 4 * 64, rm.data_ptr() + 4 * 65

    def run(c=ct.data_ptr(), cl=R_, cs=R_, x=xt.data_ptr(), xl=S, xs=S, b=B, o=out_ptr, of=need, e=e_ptr, r=r_ptr, rf=need_r):
        return lib.raw("hipfeat_stream_run", handle.handle, c, cl, cs, x, xl, xs, b, o, of, e, r, rf, stream)

    # refusals: nothing is launched
    for bad in (dict(of=need - 1), dict(rf=need_r - 1), dict(cs=R_ - 1), dict(xs=S - 1), dict(o=None), dict(r=None), dict(x=None), dict(b=-1), dict(cl=-1),
                dict(xl=-1), dict(c=None), dict(o=out_ptr + 2), dict(r=r_ptr + 1), dict(x=xt.data_ptr() + 2), dict(c=ct.data_ptr() + 1)):
        assert run(**bad) == _lib.ERR_INVALID, bad
    if which == "spectrum":
        assert run(o=out_ptr + 4, of=need) == _lib.ERR_INVALID
    assert run(b=0, of=0, rf=0) == 0
    torch.cuda.synchronize()
    assert buf.isnan().all() and en.isnan().all() and rm.isnan().all()
    assert run() == 0
    torch.cuda.synchronize()
    assert buf[:guard].isnan().all() and buf[guard + need:].isnan().all() and not buf[guard:guard + need].isnan().any()
    assert rm[:65].isnan().all() and rm[65 + need_r:].isnan().all()
    assert en[:64].isnan().all() and en[64 + B * T:].isnan().all() and en[64:64 + B * T].isnan().any() != energies
    out, remainder = layer.online_inference(xt, ct)
    frames, log_e = out if isinstance(out, tuple) else (real(out), None)
    assert torch.equal(buf[guard:guard + need].view(B, T, width), frames.reshape(B, T, width))
    assert torch.equal(rm[65:65 + need_r].view(B, rem), remainder)
    if energies:
        assert torch.equal(en[64:64 + B * T].view(B, T), log_e)
        buf.fill_(float("nan"))  # d_log_energy may be NULL
        assert run(e=None) == 0
        torch.cuda.synchronize()
        assert torch.equal(buf[guard:guard + need].view(B, T, width), frames) and buf[:guard].isnan().all() and buf[guard + need:].isnan().all()
    # a call without frames writes its remainder and nothing else
    buf.fill_(float("nan")), rm.fill_(float("nan")), en.fill_(float("nan"))
    assert run(cl=100, xl=50, of=0, rf=B * 150) == 0  # (the rows keep their strides)
    torch.cuda.synchronize()
    assert buf.isnan().all() and en.isnan().all() and rm[:65].isnan().all() and rm[65 + B * 150:].isnan().all()
    assert torch.equal(rm[65:65 + B * 150].view(B, 150), torch.cat((ct[:, :100], xt[:, :50]), dim=1))


@pytest.mark.parametrize("name,kw", INVARIANCE, ids=[c[0] for c in INVARIANCE])
def test_the_zero_frame_rule_no_rows_and_one_dimensional_chunks(name, kw):
    for snip in (False, True):
        layer = make(name, snip_edges=snip, **kw)
        n, shift = sizes_of(layer)
        width = joined([layer.online_inference(torch.zeros(1, 2 * n, device="cuda"))[0]])[0].shape[2:]
        # L < N at the start of a stream (S < P, S >= P), behind a context, with an empty chunk, with nothing at all
        x = torch.from_numpy(R.signal(61, 3, n)).cuda()
        p = (n - shift) // 2
        for context, s in ((None, p - 1), (None, n - p - 1 if not snip else n - 1), (x[:, :n - 10].contiguous(), 9), (x[:, :n - 1].contiguous(), 0),
                           (x[:, :0].contiguous(), 0), (None, 0)):
            chunk = x[:, :s]
            out, rem = layer.online_inference(chunk, context)
            frames, log_e = joined([out])
            V = SR.virtual(chunk.cpu().numpy(), None if context is None else context.cpu().numpy(), n, shift, snip)
            assert V.shape[1] < n and tuple(frames.shape) == (3, 0) + tuple(width) and torch.equal(rem.cpu(), torch.from_numpy(V))
            if name == "Wav2Win":
                assert tuple(log_e.shape) == (3, 0)
        # ... and the stream goes on from there: chunks shorter than a frame add up to the one-chunk output
        xs = torch.from_numpy(R.signal(62, 2, 3 * n)).cuda()
        small = [n // 3] * 9
        a, ea = joined(run_stream(layer, xs, [p] + [3 * n - p])[0])
        b, eb = joined(run_stream(layer, xs, [p] + [small[0] - p] + small[1:] + [3 * n - sum(small)])[0])
        assert torch.equal(a, b) and a.shape[1] >= 5
        # B = 0
        out, rem = layer.online_inference(torch.zeros((0, 5 * shift + n), device="cuda"))
        frames, log_e = joined([out])
        assert frames.shape[0] == 0 and frames.shape[1] in (5, 6) and rem.shape[0] == 0
        out, rem = layer.online_inference(torch.zeros((0, shift), device="cuda"), torch.zeros((0, n), device="cuda"))
        assert joined([out])[0].shape[:2] == (0, 2) and tuple(rem.shape) == (0, n + shift - 2 * shift)
        # a 1-D chunk: 2-D output, the remainder stays (1, R) and is accepted back
        o2, r2 = layer.online_inference(xs[:1, :2 * n])
        o1, r1 = layer.online_inference(xs[0, :2 * n])
        f2, e2 = joined([o2])
        f1, e1 = (o1[0], o1[1]) if isinstance(o1, tuple) else (real(o1), None)
        assert torch.equal(f1, f2[0]) and torch.equal(r1, r2) and r1.ndim == 2 and (e1 is None or torch.equal(e1, e2[0]))
        o3, _ = layer.online_inference(xs[0, 2 * n:], r1)
        o4, _ = layer.online_inference(xs[:1, 2 * n:], r2)
        assert torch.equal(o3[0] if isinstance(o3, tuple) else real(o3), joined([o4])[0][0])


def test_argument_checks_unsupported_sizes_dither_streams_and_pickle():
    x = torch.from_numpy(R.signal(71, 2, 4000)).cuda()
    ctx = x[:, :240].contiguous()
    for name, kw in INVARIANCE:
        layer = make(name, **kw)
        with pytest.raises(_lib.HipFeatError, match="no CPU fallback|'cuda"):
            layer.online_inference(x.cpu())
        with pytest.raises(TypeError, match="float32"):
            layer.online_inference(x.double())
        with pytest.raises(NotImplementedError, match="inference-only"):
            layer.online_inference(x.clone().requires_grad_(True))
        with torch.no_grad():
            layer.online_inference(x.clone().requires_grad_(True))
        for bad in (ctx[0], ctx[:1], ctx.double(), ctx.cpu(), ctx.cpu().numpy(), ctx.unsqueeze(0)):
            with pytest.raises(AssertionError):
                layer.online_inference(x, bad)
        # handles are lazy, per device, and dropped on pickle; a pickled layer streams the same bits
        a, ra = layer.online_inference(x, ctx)
        again = pickle.loads(pickle.dumps(layer))
        holder = again if name == "Wav2Win" else getattr(again, "wav2win", again)
        assert not getattr(holder, "_handles", {}) and not getattr(again, "_streams", {})
        b, rb = again.online_inference(x, ctx)
        assert torch.equal(joined([a])[0], joined([b])[0]) and torch.equal(ra, rb)
    # sizes the stream kernel does not serve: refused, naming the supported sizes and that forward goes on
    for name, kw in (("Wav2FFT", {"round_to_power_of_two": False}), ("Wav2LogFilterBank", {"round_to_power_of_two": False}), ("Wav2MFCC", {"sampling_rate": 4000}),
                     ("Wav2Spec", {"frame_length": 0.05, "sampling_rate": 48000}), ("Wav2LogFilterBank", {"num_filters": 129}),
                     ("Wav2Win", {"sampling_rate": 48000, "frame_length": 0.05})):
        with pytest.raises(NotImplementedError, match="256, 512, 1024 and 2048(.|\n)*forward\\(\\) still serves"):
            make(name, **kw).online_inference(x)
    assert make("Wav2LogFilterBank", round_to_power_of_two=False)(x).shape == (2, 25, 80)  # (forward does)
    frames, _ = make("Wav2Win", sampling_rate=4000).online_inference(x)[0]  # frames of any length up to 2048 are served
    assert frames.shape[2] == 100
    # dither: torch.randn on the chunk alone, in front of the launch
    for name in ("Wav2FFT", "Wav2LogFilterBank"):
        quiet, noisy = make(name, dither=0.0), make(name, dither=1.0)
        torch.manual_seed(3)
        a, ra = noisy.online_inference(x, ctx)
        torch.manual_seed(3)
        noise = torch.randn(x.shape, device=x.device)
        b, rb = quiet.online_inference(x + 1.0 * noise, ctx)
        assert torch.equal(real(a), real(b)) and torch.equal(ra, rb) and not torch.equal(real(a), real(quiet.online_inference(x, ctx)[0]))
    # another stream
    side = torch.cuda.Stream()
    layer = make("Wav2LogFilterBank")
    want, rw = layer.online_inference(x, ctx)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got, rg = layer.online_inference(x, ctx)
    side.synchronize()
    assert torch.equal(got, want) and torch.equal(rg, rw)


@pytest.mark.parametrize("name", sorted(SR.GOLDEN_CASES))
def test_the_goldens_of_the_live_layers(name):
    arrays = np.load(GOLDEN)
    cls, kw, batch, sizes = SR.GOLDEN_CASES[name]
    x = SR.golden_input(name)
    assert np.array_equal(arrays[f"{name}/x"], x)
    layer = make(cls, **kw)
    n, shift = sizes_of(layer)
    outs, _ = run_stream(layer, torch.from_numpy(x).cuda(), sizes)
    for i, (out, (_, _, V, T, remainder)) in enumerate(zip(outs, SR.walk(x, sizes, n, shift, kw.get("snip_edges", False)))):
        frames, log_e = out if isinstance(out, tuple) else (out, None)
        got = frames.cpu().numpy()
        stored = arrays[f"{name}/{i}/out"]
        assert got.shape == stored.shape and got.dtype == stored.dtype
        # the bars the stored values themselves are held to (tests/test_stream_golden.py), with the stored values as the float32 reference
        if cls == "Wav2Win":
            cfg = SR.stft_config(kw, "return_log_energy")
            t_frames, t_log_e, _ = SR.truth(V, cfg, kw.get("pad_length", n))
            R.hold(f"golden {name}/{i} frames", got, stored, t_frames)
            assert (log_e is not None) == cfg.use_energy
            if log_e is not None:
                R.hold_energy(f"golden {name}/{i} log-energy", log_e.cpu().numpy(), t_log_e)
        elif cls == "Wav2FFT":
            cfg = SR.stft_config(kw, "use_energy")
            R.hold(f"golden {name}/{i} spectrum", got, stored, SR.truth(V, cfg)[2], energy_bin=cfg.use_energy)
        else:
            cfg = SR.golden_feature_config(name)
            want = SR.features_truth(V, cfg)
            for b in range(batch):
                SR.hold_features(SR.KINDS[cls], cfg.use_energy, got[b].astype(np.float64), want[b])
