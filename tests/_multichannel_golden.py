"""Golden of the multi-channel collation: int16 inputs and what the reference's LIVE ``collate_audio``
(lhotse/dataset/collation.py:148-247) returns for them in its three ``mono_downmix`` modes.

``python tests/_multichannel_golden.py`` (authoring container only: needs the real lhotse) writes tests/golden/multichannel.npz:

    in/<i>            int16 (C_i, T_i): cut i as its WAV holds it (the stdlib backend reads sample / 32768 as float32)
    true              ``collate_audio(cuts, mono_downmix=True)[0]``: (B, Tmax) float32
    none              ``mono_downmix=None`` on the whole batch (it holds a mono cut: the downmix, (B, Tmax))
    false/<C>         ``mono_downmix=False`` on the cuts FALSE_BATCHES[C] -- the cuts of C channels and the mono cut; the reference
                      collates (B, C, T) only where every multi-channel cut of the batch has the same C --: (B', C, Tmax')
    none_multi        ``mono_downmix=None`` on the two 3-channel cuts alone (NONE_MULTI): (2, 3, Tmax')
    lens              the int32 ``audio_lens`` of the whole batch

The cuts have 2, 3, 1, 8 and 3 channels and unequal lengths of about two thousand samples.  ``write_cuts`` builds the same cuts on disk for
the tests that run under the real lhotse; ``load`` is what the GPU test reads."""
import os
import wave

import numpy as np

SR = 16000
SHAPES = [(2, 2100), (3, 1700), (1, 1900), (8, 1500), (3, 1300)]  # (channels, samples) per cut
FALSE_BATCHES = {2: [0, 2], 3: [1, 2, 4], 8: [3, 2]}  # channels -> the cuts of its (B, C, T) batch
NONE_MULTI = [1, 4]
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multichannel.npz")


def make_inputs(shapes=SHAPES, seed=2024):
    rs = np.random.RandomState(seed)
    out = []
    for c, t in shapes:
        gain = rs.uniform(2000.0, 30000.0, size=(c, 1))  # channels of unequal level, as microphones at unequal distances
        out.append(np.round((rs.rand(c, t) * 2.0 - 1.0) * gain).astype(np.int16))
    return out


def write_cuts(directory, inputs, sampling_rate=SR, prefix="mc"):
    """One int16 WAV per cut (interleaved channels) + a ``MultiCut`` over all its channels (a ``MonoCut`` for one channel)."""
    from lhotse import MonoCut, MultiCut, Recording
    from lhotse.audio import AudioSource

    cuts = []
    for i, pcm in enumerate(inputs):
        c, t = pcm.shape
        p = os.path.join(str(directory), f"{prefix}{i}.wav")
        with wave.open(p, "wb") as f:
            f.setnchannels(c), f.setsampwidth(2), f.setframerate(sampling_rate)
            f.writeframes(np.ascontiguousarray(pcm.T).tobytes())
        rec = Recording(id=f"{prefix}rec{i}", sources=[AudioSource(type="file", channels=list(range(c)), source=p)], sampling_rate=sampling_rate,
                        num_samples=t, duration=t / sampling_rate)
        if c == 1:
            cuts.append(MonoCut(id=f"{prefix}cut{i}", start=0, duration=rec.duration, channel=0, recording=rec))
        else:
            cuts.append(MultiCut(id=f"{prefix}cut{i}", start=0, duration=rec.duration, channel=list(range(c)), recording=rec))
    return cuts


def load():
    with np.load(PATH) as z:
        g = {k: z[k] for k in z.files}
    g["inputs"] = [g[f"in/{i}"] for i in range(len(SHAPES))]
    return g


def main():
    import sys
    import tempfile

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from _dropin_support import import_lhotse, install_wave_backend

    import_lhotse()
    from lhotse import CutSet
    from lhotse.dataset.collation import collate_audio

    install_wave_backend()
    inputs = make_inputs()
    with tempfile.TemporaryDirectory() as d:
        cuts = write_cuts(d, inputs)
        batch = CutSet.from_cuts(cuts)
        out = {f"in/{i}": x for i, x in enumerate(inputs)}
        for name, mode in (("true", True), ("none", None)):
            audio, lens = collate_audio(batch, mono_downmix=mode)
            out[name] = audio.numpy()
        out["lens"] = lens.numpy()
        for c, ids in FALSE_BATCHES.items():
            out[f"false/{c}"] = collate_audio(CutSet.from_cuts([cuts[i] for i in ids]), mono_downmix=False)[0].numpy()
            assert out[f"false/{c}"].shape == (len(ids), c, max(SHAPES[i][1] for i in ids))
        out["none_multi"] = collate_audio(CutSet.from_cuts([cuts[i] for i in NONE_MULTI]), mono_downmix=None)[0].numpy()
    assert out["true"].shape == (5, 2100) and out["none"].shape == (5, 2100) and out["none_multi"].shape == (2, 3, 1700)
    np.savez_compressed(PATH, **out)
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
