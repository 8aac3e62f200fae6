"""GPU: the six ``HipWav2*`` layers behind a stalled stream (the scenario: tests/_stalled_stream.py::run_scenario):
``forward(x)``, ``forward(x, lengths, padding_value)``, the backward of both after ``differentiable_()`` and ``online_inference``.

P and Q are two calls of ONE layer object (its plan, its STFT handle, its gradient handle and its streaming handle are the shared
handles).  The ragged lengths are those of tests/test_gpu_ragged.py: rows at ``Smax``, one workgroup's 32 frames, the shortest legal row
and, with ``snip_edges``, a row of no samples; Q's are P's permuted and shortened.  The graph of a backward case is built under the stalled
stream and ``backward`` is called there, with cotangents that arrive by a copy on that stream; the ragged backward runs with
``_GRAD_WORKSPACE_BYTES`` set as tests/test_gpu_ragged.py sets it, one row per piece, so several workspace pieces are in flight behind
the stall.  The reference of step 1 is the float64 restatement ``_grad_ref.forward`` / ``_grad_ref.gradient`` with the bars of
tests/test_gpu_ragged.py::test_every_row_is_held_to_the_float64_restatement (imported); ``online_inference`` is held to the same
restatement on the virtual waveform ``[context | x]`` of tests/_stream_ref.py, framed without reflection.  All of these are claimed to
repeat bit for bit (tests/test_gpu_ragged.py: "determinism"; tests/test_gpu_stream.py: chunking invariance), so the stalled results are
held to the bits of the synchronised run."""
import pytest
import torch

import _grad_ref as G
import _stft_ref as R
import _stream_ref as SR
import test_gpu_ragged as TR
from _stalled_stream import Call, run_scenario

from lhotse_amd import layers as LY

pytestmark = pytest.mark.gpu
WARM_ROUNDS = 8  # x (P, Q) = 16 calls: more than any ring a layer's handles have
MODES = ("forward", "ragged", "backward", "ragged-backward", "online")


def _hold_rows(label, cls, kw, rows, outs, cots=None, grad=None):
    """rows: per row b its waveform (1, S_b) float32; outs: the device's outputs on the host, row b's first T_b frames being the row's;
    the loop of test_every_row_is_held_to_the_float64_restatement."""
    n, shift, _ = G.sizes(kw, cls)
    for b, row in enumerate(rows):
        t = G.num_frames(row.shape[1], n, shift, kw["snip_edges"])
        if t == 0:
            if grad is not None:
                assert not grad[b].view(torch.int32).any(), (label, b, "the gradient of a row without frames is +0.0")
            continue
        t64 = G.outputs(G.forward(cls, kw, torch.from_numpy(row).double()))
        r32 = G.outputs(G.forward(cls, kw, torch.from_numpy(row)))
        for i, (got, want, ref) in enumerate(zip(outs, t64, r32)):
            got, want, ref = got[b: b + 1, :t].numpy(), want.numpy(), ref.numpy()
            if cls in ("Wav2Win", "Wav2FFT"):
                if i == 1:
                    R.hold_energy(f"{label} row {b} log-energy", got, want)
                else:
                    R.hold(f"{label} row {b}", got, ref, want, energy_bin=(cls == "Wav2FFT"))
            else:
                TR.hold_features(cls, kw, got[0], want[0])
        if grad is not None:
            c = [k[b: b + 1, :t] for k in cots]
            g64, g32 = G.gradient(cls, kw, row, c, torch.float64), G.gradient(cls, kw, row, c, torch.float32)
            G.hold(f"{label} row {b}", grad[b: b + 1, : row.shape[1]].numpy(), g32, g64)
            assert not grad[b, row.shape[1]:].view(torch.int32).any(), (label, b, "the gradient behind the row is +0.0")


def _shapes(cls, kw, lens):
    """The shapes of the layer's outputs for rows of ``lens`` samples, (B, Tmax, ...)."""
    n, shift, _ = G.sizes(kw, cls)
    tmax = max(G.num_frames(s, n, shift, kw["snip_edges"]) for s in lens)
    one = G.outputs(G.forward(cls, kw, torch.zeros((1, max(max(lens), n + shift)), dtype=torch.float32)))
    return [(len(lens), tmax) + tuple(o.shape[2:]) for o in one]


def _layer_call(layer, cls, kw, mode, seed, smax, lens, padding_value):
    """lens: the row lengths (uniform modes: all equal to smax)"""
    ragged, backward = mode.startswith("ragged"), mode.endswith("backward")
    x = TR.signal(seed, len(lens), smax, kw.get("sampling_rate", 16000))
    host = {"x": torch.from_numpy(x)}
    cots = TR.cotangents(seed + 1, cls, _shapes(cls, kw, lens)) if backward else None
    if backward:
        host.update({f"cot{i}": torch.from_numpy(c) for i, c in enumerate(cots)})

    def run(bufs):
        xt = bufs["x"].detach().requires_grad_(True) if backward else bufs["x"]
        res = layer(xt, lens, padding_value)[0] if ragged else layer(xt)
        outs = G.outputs(res)
        if not backward:
            return list(outs)
        torch.autograd.backward(list(outs), [bufs[f"cot{i}"] for i in range(len(outs))])
        return [o.detach() for o in outs] + [xt.grad]

    def check(got):
        rows = [x[b: b + 1, :s] for b, s in enumerate(lens)]
        outs = got[: len(got) - backward]
        _hold_rows(f"stalled stream {cls} {mode}", cls, kw, rows, outs, cots, got[-1] if backward else None)
        if ragged:  # the padding rows hold the padding value
            n, shift, _ = G.sizes(kw, cls)
            for b, s in enumerate(lens):
                t = G.num_frames(s, n, shift, kw["snip_edges"])
                for o in outs:
                    pad = torch.view_as_real(o[b, t:]) if o.is_complex() else o[b, t:]
                    assert bool((pad[..., 0] == padding_value).all() if o.is_complex() else (pad == padding_value).all()), (cls, mode, b)

    return Call(host, {}, run, check)


def _online_call(layer, cls, kw, seed, B, chunk, context_len):
    n, shift, _ = G.sizes(kw, cls)
    x = TR.signal(seed, B, chunk, kw.get("sampling_rate", 16000))
    context = None if context_len is None else TR.signal(seed + 1, B, context_len, kw.get("sampling_rate", 16000))
    host = {"x": torch.from_numpy(x)}
    if context is not None:
        host["context"] = torch.from_numpy(context)
    V = SR.virtual(x, context, n, shift, kw["snip_edges"])
    T, remainder = SR.split(V, n, shift)
    assert T > 0

    def run(bufs):
        res, rem = layer.online_inference(bufs["x"], bufs.get("context"))
        return list(G.outputs(res)) + [rem]

    def check(got):
        assert torch.equal(got[-1], torch.from_numpy(remainder))
        _hold_rows(f"stalled stream {cls} online", cls, dict(kw, snip_edges=True), [V[b: b + 1] for b in range(B)], got[:-1])

    return Call(host, {}, run, check)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cls", G.CLASSES)
def test_layer(cls, mode, monkeypatch):
    snip = mode.startswith("ragged")  # (the ragged cases carry a row of no samples, which only snip_edges allows)
    kw = TR.config(cls, snip)
    n, shift, _ = G.sizes(kw, cls)
    smax, edge = TR.edge_lengths(n, shift, snip)  # [Smax, Smax - 1, one workgroup's 32 frames, that plus a shift, the shortest legal row]
    layer = G.hip_layer(cls, kw)  # (in differentiable mode: an input that asks for no gradient takes the plain path)
    if mode == "online":
        head = 0 if snip else (n - shift) // 2
        P = _online_call(layer, cls, kw, 91, 2, n + 31 * shift + 5 - head, None)       # the start of a stream: 32 frames
        Q = _online_call(layer, cls, kw, 93, 3, 3 * shift + 1, n - shift + 7)          # a chunk behind a remainder: 4 frames
    elif mode.startswith("ragged"):
        p_lens = [smax, edge[2], edge[4], 0, edge[3]]
        q_lens = [0, edge[4], edge[2] - shift, smax - shift - 3]  # P's permuted and shortened, in a batch of another size
        if mode == "ragged-backward":
            nr = (n + 3) & ~3
            monkeypatch.setattr(LY, "_GRAD_WORKSPACE_BYTES", G.num_frames(smax, n, shift, snip) * nr * 4)  # one row per piece
        P = _layer_call(layer, cls, kw, mode, 95, smax, p_lens, -1.5)
        Q = _layer_call(layer, cls, kw, mode, 97, smax - shift, q_lens, 0.25)
    else:
        P = _layer_call(layer, cls, kw, mode, 95, smax, [smax] * 3, 0.0)
        Q = _layer_call(layer, cls, kw, mode, 97, edge[2], [edge[2]] * 2, 0.0)
    run_scenario(f"{cls} {mode}", P, Q, WARM_ROUNDS)
