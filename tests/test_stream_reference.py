"""CPU, under the real lhotse (authoring container only): the six layers' ``online_inference`` has the reference's signature, and
tests/_stream_ref.py -- the framing the GPU tests hold the device to -- equals the live ``online_inference`` with torch.equal: the
remainder for all six layers, the outputs for ``Wav2Win`` / ``Wav2FFT``.  Where ``[context | x]`` is shorter than a frame the reference
raises; the device layers document that they do not."""
import inspect
import warnings

import numpy as np
import pytest
import torch

import _stft_ref as R
import _stream_ref as SR

pytestmark = pytest.mark.reference


@pytest.fixture(scope="module")
def ref():
    from _dropin_support import import_lhotse

    import_lhotse()
    import lhotse.features.kaldi.layers as L

    import lhotse_amd as LA

    return LA, L


@pytest.mark.parametrize("name", SR.LAYERS)
def test_the_signature_of_online_inference_is_the_references(ref, name):
    LA, L = ref
    mine, theirs = getattr(LA, "Hip" + name), getattr(L, name)
    assert inspect.signature(mine.online_inference, eval_str=True) == inspect.signature(theirs.online_inference, eval_str=True)


def live_layer(L, name, kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return getattr(L, name)(**kw)


# chunk sequences (16 kHz: N 400, s 160, P 120): a first call and continued calls, chunks of one shift, an irregular sequence.  Every call has
# a frame under both snip_edges values: the first chunk holds one and every later chunk is at least one shift long.
SEQUENCES = [(560, 333, 487), (400, 160, 160, 160), (1234, 161, 160, 1000), (2000,)]


@pytest.mark.parametrize("snip", (False, True), ids=("reflect", "snip"))
@pytest.mark.parametrize("name", SR.LAYERS)
def test_the_restated_framing_is_the_live_framing(ref, name, snip):
    LA, L = ref
    for k, sizes in enumerate(SEQUENCES):
        kw = dict(snip_edges=snip)
        layer = live_layer(L, name, kw)
        n, shift = (layer._length, layer._shift) if name == "Wav2Win" else (layer.wav2win._length, layer.wav2win._shift)
        x = R.signal(60 + k, 2, sum(sizes))
        context = None
        for chunk, ctx, V, T, remainder in SR.walk(x, sizes, n, shift, snip):
            assert T >= 1
            assert (context is None) == (ctx is None) and (ctx is None or np.array_equal(context.numpy(), ctx))
            with torch.no_grad():
                out, context = layer.online_inference(torch.from_numpy(chunk), context)
            assert torch.equal(context, torch.from_numpy(remainder)), (name, sizes)
            frames = out[0] if name == "Wav2Win" else out
            assert frames.shape[:2] == (2, T)
            if name == "Wav2Win":
                cfg = R.config(16000, False, snip_edges=snip)
                r_frames, _, _ = SR.ref32(V, cfg, n)
                assert torch.equal(out[0], torch.from_numpy(r_frames)) and out[1] is None
            elif name == "Wav2FFT":
                cfg = R.config(16000, True, snip_edges=snip)
                assert torch.equal(out, torch.from_numpy(SR.ref32(V, cfg)[2]))


@pytest.mark.parametrize("rate,n,fft", R.RATES, ids=[str(r[0]) for r in R.RATES])
def test_win_and_fft_outputs_over_options_short_first_chunks_and_made_up_contexts(ref, rate, n, fft):
    LA, L = ref
    grid = list(R.option_grid(rate))[::7]  # both snip_edges values, DC, pre-emphasis, the windows, raw energy, energy on / off
    assert {c.snip_edges for c in grid} == {False, True} and {c.use_energy for c in grid} == {False, True}
    for i, cfg in enumerate(grid):
        _, shift, _ = R.K.window_sizes(cfg)
        p = (n - shift) // 2
        kw = R.layer_kwargs(cfg)
        win = live_layer(L, "Wav2Win", dict(pad_length=n + 1, return_log_energy=cfg.use_energy, **kw))
        fftl = live_layer(L, "Wav2FFT", dict(use_energy=cfg.use_energy, **kw))
        # (context, chunk) pairs with a frame: the start of a stream; a remainder-like context; a caller-made context longer than a frame
        # (frames wholly in the context, across the seam, wholly in the chunk); a chunk shorter than P behind a context
        pairs = [(None, n + 3 * shift + 5), (n - shift + 7, 2 * shift), (2 * n + 3, n + shift), (n, max(p - 1, 1))]
        for j, (r, s) in enumerate(pairs):
            x = R.signal(100 * i + j, 2, s)
            context = None if r is None else R.signal(100 * i + j + 50, 2, r)
            V = SR.virtual(x, context, n, shift, cfg.snip_edges)
            T, remainder = SR.split(V, n, shift)
            assert T >= 1
            ct = None if context is None else torch.from_numpy(context)
            with torch.no_grad():
                (frames, log_e), rem_w = win.online_inference(torch.from_numpy(x), ct)
                spec, rem_f = fftl.online_inference(torch.from_numpy(x), ct)
            r_frames, r_log_e, _ = SR.ref32(V, cfg, n + 1)
            assert torch.equal(rem_w, torch.from_numpy(remainder)) and torch.equal(rem_f, torch.from_numpy(remainder))
            assert torch.equal(frames, torch.from_numpy(r_frames)), (i, j, cfg)
            assert (log_e is None) == (r_log_e is None) and (log_e is None or torch.equal(log_e, torch.from_numpy(r_log_e)))
            assert torch.equal(spec, torch.from_numpy(SR.ref32(V, cfg)[2])), (i, j, cfg)


def test_a_first_chunk_shorter_than_p_reflects_only_what_it_has(ref):
    LA, L = ref
    # (a first chunk shorter than P never completes a frame, 2 S < 2 P < N, so the layers raise there: the framing function alone is asked)
    x = torch.from_numpy(R.signal(7, 2, 50))  # N 100, s 80, P 10 < S: L = 60, no frame, everything is handed back
    frames, remainder = L._get_strided_batch_streaming(x, window_length=100, window_shift=80, snip_edges=False)
    V = SR.virtual(x.numpy(), None, 100, 80, False)
    assert frames.shape[1] == 0 and V.shape[1] == 60 and SR.counts(60, 100, 80) == (0, 60) and torch.equal(remainder, torch.from_numpy(V))
    x5 = torch.from_numpy(R.signal(8, 2, 95))  # L = 105: a frame
    frames, remainder = L._get_strided_batch_streaming(x5, window_length=100, window_shift=80, snip_edges=False)
    V = SR.virtual(x5.numpy(), None, 100, 80, False)
    T, rem = SR.split(V, 100, 80)
    assert T == 1 and torch.equal(remainder, torch.from_numpy(rem)) and torch.equal(frames[:, 0], torch.from_numpy(V[:, :100].copy()))
    # S < P: the flipped head is the whole chunk
    x3 = R.signal(9, 1, 30)
    V = SR.virtual(x3, None, 400, 160, False)
    assert V.shape[1] == 60 and np.array_equal(V[:, :30], x3[:, ::-1]) and np.array_equal(V[:, 30:], x3)
    pad_left = torch.flip(torch.from_numpy(x3)[:, :120], (1,))  # layers.py:828-830 on a chunk shorter than P
    assert torch.equal(torch.cat((pad_left, torch.from_numpy(x3)), dim=1), torch.from_numpy(V))


@pytest.mark.parametrize("snip", (False, True), ids=("reflect", "snip"))
@pytest.mark.parametrize("name", SR.LAYERS)
def test_the_reference_raises_where_there_is_no_frame(ref, name, snip):
    """The documented difference: ``[context | x]`` shorter than a frame gives zero frames on the device, an error in the reference."""
    LA, L = ref
    layer = live_layer(L, name, dict(snip_edges=snip))
    for context, s in ((None, 100), (None, 279), (R.signal(1, 2, 200), 150), (R.signal(2, 2, 0), 399)):
        x = R.signal(3, 2, s)
        V = SR.virtual(x, context, 400, 160, snip)
        assert SR.counts(V.shape[1], 400, 160)[0] == 0
        with pytest.raises(RuntimeError), torch.no_grad():
            layer.online_inference(torch.from_numpy(x), None if context is None else torch.from_numpy(context))
