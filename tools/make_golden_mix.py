#!/usr/bin/env python3
"""
TEST INFRASTRUCTURE -- generates tests/golden/mix.npz + mix.json: what the REFERENCE returns for mixed cuts (CutMix, CutSet.mix / .pad)
over the corpus of oracle/driver_corpus.py, together with the track tables of those cuts in plain numbers.

Needs the real lhotse (authoring container only):

    python tools/make_golden_mix.py

Groups (fixed seeds):
  1 cutmix        CutMix(p=1, snr=(10, 20), pad_to_longest=True, random_mix_offset=True) over plain cuts
  2 speed_cutmix  the same behind PerturbSpeed([0.9, 1.1], p=1)
  3 pad           cuts.pad(duration=...) with direction right and left (a PaddingCut track)
  4 fixed         a fixed-SNR mix: one cut with snr=None (gain 1), one with an all-zero noise file (E_t = 0), one at 15 dB
  5 k2            one K2SpeechRecognitionDataset(OnTheFlyFeatures(Fbank()), cut_transforms=[PerturbSpeed(p=2/3), CutMix(p=0.5)]) batch
                  (no pad_to_longest: mixed, speed-only and plain cuts share the mini-batch)

Per cut: the track table -- file id (None = padding track; "zero" = the all-zero file), first sample and sample count of the read in
front of a pending Speed, factor, offset in samples, SNR, reference flag, samples the track ends up with -- and the wanted sample count
(cut ids are uuid4 and lhotse is absent where the GPU tests run); the reference's Fbank features (groups 1-4: every cut framed on its
own; group 5: the zero-padded batch the dataset returned); for some cuts of groups 1-4 `load_audio()`, and for groups 1, 3, 4 the exact
float64 mix of the same float32 tracks (stored as its float32 difference from `load_audio()`) with the reference's own rel-L2 distance
from it.  The track tables are taken from the product's own classifier and reader (`deferred_mix`, `_read_tracks`) with the audio backend
logging which samples of which file each track read; that the numpy rule of tests/_mix_ref.py over these tables equals `load_audio()`
is asserted here and again in tests/test_mix_reference.py.
"""
from __future__ import annotations

import json
import os
import random
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.driver_corpus import SAMPLING_RATE, write_corpus, write_wav  # noqa: E402

AUDIO_MAX = 9000  # cuts up to this many samples keep their audio (the fixtures stay under 1 MB)
ZERO_SAMPLES = 6000


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    from _dropin_support import import_lhotse, install_wave_backend
    from _mix_ref import mix_tracks

    import_lhotse()
    install_wave_backend()
    from lhotse import CutSet, MonoCut, Recording, SupervisionSegment
    from lhotse.audio import AudioSource
    from lhotse.audio.backend import get_current_audio_backend
    from lhotse.dataset import K2SpeechRecognitionDataset
    from lhotse.dataset.cut_transforms import CutMix, PerturbSpeed
    from lhotse.dataset.input_strategies import OnTheFlyFeatures
    from lhotse.features.kaldi.extractors import Fbank

    import lhotse_amd.input_strategies as IS

    backend = get_current_audio_backend()
    reads = []
    inner = backend.read_audio

    def logging_read(path_or_fd, offset=0.0, duration=None, force_opus_sampling_rate=None):
        audio, sr = inner(path_or_fd, offset=offset, duration=duration, force_opus_sampling_rate=force_opus_sampling_rate)
        reads.append((Path(str(path_or_fd)).stem, int(round(offset * sr)), int(audio.shape[1])))
        return audio, sr

    backend.read_audio = logging_read

    def cutset(files, ids, supervised=True):
        cuts = []
        for f in files:
            if f["id"] not in ids:
                continue
            dur = f["num_samples"] / SAMPLING_RATE
            rec = Recording(id=f"rec-{f['id']}", sources=[AudioSource(type="file", channels=[0], source=f["path"])], sampling_rate=SAMPLING_RATE,
                            num_samples=f["num_samples"], duration=dur)
            sup = SupervisionSegment(id=f"sup-{f['id']}", recording_id=rec.id, start=0.0, duration=dur, channel=0, text=f"text of {f['id']}")
            cuts.append(MonoCut(id=f["id"], start=0, duration=dur, channel=0, recording=rec, supervisions=[sup] if supervised else []))
        return CutSet.from_cuts(sorted(cuts, key=lambda c: ids.index(c.id)))

    def table_of(cut):
        """-> (rows of the track table, loaded tracks) through the product's classifier and reader; a plain cut is a cut of one track."""
        if type(cut).__name__ == "MixedCut":
            tracks = IS.deferred_mix(cut)
            assert tracks is not None, cut
        else:
            chain = IS.parse_chain(cut, gpu_reverb=False, gpu_resample=False, gpu_level=False)  # a Speed, or the cut as load_audio() gives it
            tracks = [IS.PendingTrack(cut, 0, None, True, chain or IS.Chain())]
        rows, loaded = [], []
        for tr in tracks:
            del reads[:]
            res = IS._read_tracks(cut, [tr])
            assert res is not None
            x, factor, off, snr, is_ref, n = res[0][0][:6]
            if isinstance(x, int):
                assert not reads
                rows.append({"file": None, "first": 0, "count": int(x), "factor": 1.0, "offset": int(off), "snr": None, "ref": False, "num_samples": int(n)})
            else:
                assert len(reads) == 1 and reads[0][2] == len(x), (reads, len(x))
                rows.append({"file": reads[0][0], "first": reads[0][1], "count": len(x), "factor": float(factor), "offset": int(off),
                             "snr": None if snr is None else float(snr), "ref": bool(is_ref), "num_samples": int(n)})
            loaded.append(x)
        return rows, loaded

    def rel_l2(a, b):
        return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b))

    arrays, meta = {}, {"sampling_rate": SAMPLING_RATE, "zero_samples": ZERO_SAMPLES, "groups": {}}
    fb = Fbank()
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        files = write_corpus(td / "wav")
        meta["files"] = [{k: v for k, v in f.items() if k != "path"} for f in files]
        write_wav(td / "wav" / "zero.wav", np.zeros(ZERO_SAMPLES, dtype=np.int16))
        zero = {"id": "zero", "num_samples": ZERO_SAMPLES, "path": str(td / "wav" / "zero.wav")}
        speech = cutset(files, ["utt6", "utt4", "utt2"])
        speech = CutSet.from_cuts([c if c.id != "utt2" else c.truncate(offset=0.1, duration=0.45) for c in speech])  # (short cuts: small fixtures)
        noise = cutset(files, ["utt1", "utt7"], supervised=False)

        def record(group, cuts, audio=True, exact=True):
            out = []
            for i, cut in enumerate(cuts):
                rows, loaded = table_of(cut)
                want = int(cut.num_samples)
                ref_audio = cut.load_audio()[0]
                assert ref_audio.dtype == np.float32 and len(ref_audio) == want
                key = f"{group}/{i}"
                entry = {"tracks": rows, "want": want, "audio": False, "exact": False}
                arrays[f"{key}/feats"] = fb.extract(ref_audio, SAMPLING_RATE)
                if all(r["factor"] == 1.0 for r in rows):  # the rule, bit for bit, with the reference's own float32 energies
                    tr = [(r["count"] if r["file"] is None else x, r["offset"], r["snr"]) for r, x in zip(rows, loaded)]
                    ref = next((k for k, r in enumerate(rows) if r["ref"]), -1)
                    assert np.array_equal(mix_tracks(tr, ref, want, energy="float32"), ref_audio), (group, i)
                    if exact and audio and want <= AUDIO_MAX:
                        m64 = mix_tracks(tr, ref, want, accumulate=np.float64)
                        arrays[f"{key}/exact_minus_audio"] = (m64 - ref_audio.astype(np.float64)).astype(np.float32)
                        entry["exact"], entry["reference_rel_l2"] = True, rel_l2(ref_audio, m64)
                if audio and want <= AUDIO_MAX:
                    arrays[f"{key}/audio"] = ref_audio
                    entry["audio"] = True
                out.append(entry)
            meta["groups"][group] = out

        mix = CutMix(noise, snr=(10, 20), p=1.0, pad_to_longest=True, random_mix_offset=True, seed=7)
        record("cutmix", list(mix(speech)))
        sp = PerturbSpeed(factors=[0.9, 1.1], p=1.0, randgen=random.Random(3))
        record("speed_cutmix", list(CutMix(noise, snr=(10, 20), p=1.0, pad_to_longest=True, random_mix_offset=True, seed=11)(sp(speech))), exact=False)
        short = cutset(files, ["utt6", "utt4"])
        record("pad", list(short.pad(duration=0.55, direction="right")) + list(short.pad(duration=0.55, direction="left")))
        one_noise = list(cutset(files, ["utt4"]))[0]
        zrec = Recording(id="rec-zero", sources=[AudioSource(type="file", channels=[0], source=zero["path"])], sampling_rate=SAMPLING_RATE,
                         num_samples=ZERO_SAMPLES, duration=ZERO_SAMPLES / SAMPLING_RATE)
        zcut = MonoCut(id="zero", start=0, duration=zrec.duration, channel=0, recording=zrec)
        u6, u4 = list(short)
        record("fixed", [u6.mix(one_noise.truncate(duration=0.25), snr=None, offset_other_by=0.0301875),
                         u6.mix(zcut.truncate(duration=0.3), snr=15), u4.mix(zcut, snr=15),
                         u6.pad(duration=0.4, direction="both").mix(one_noise.truncate(duration=0.35), snr=15)])

        k2cuts = cutset(files, ["utt0", "utt2", "utt4", "utt6", "utt1", "utt7"])
        tf = [PerturbSpeed(factors=[0.9, 1.1], p=2 / 3, randgen=random.Random(1)),
              CutMix(noise, snr=(10, 20), p=0.5, pad_to_longest=False, random_mix_offset=True, seed=13)]
        ds = K2SpeechRecognitionDataset(input_strategy=OnTheFlyFeatures(Fbank()), cut_transforms=tf, return_cuts=True)
        batch = ds[k2cuts]
        bc = batch["supervisions"]["cut"]
        record("k2", bc, audio=False)
        kinds = [("mixed" if type(c).__name__ == "MixedCut" else "speed" if c.recording.transforms else "plain") for c in bc]
        assert {"mixed", "speed", "plain"} <= set(kinds), kinds
        meta["k2_kinds"] = kinds
        nf = batch["supervisions"]["num_frames"].numpy()
        inputs = batch["inputs"].numpy()
        for i in range(len(bc)):
            arrays[f"k2/{i}/feats"] = inputs[i, : int(nf[i])]  # (the batch's rows replace the per-cut matrix: zero-padded framing)
        arrays["k2/num_frames"] = nf
        arrays["k2/shape"] = np.array(inputs.shape, dtype=np.int32)

    out_dir = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(out_dir, "mix.npz"), **arrays)
    with open(os.path.join(out_dir, "mix.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("mix.npz", os.path.getsize(os.path.join(out_dir, "mix.npz")), "bytes;", {g: len(v) for g, v in meta["groups"].items()}, "k2:", meta["k2_kinds"])
    for g, v in meta["groups"].items():
        for i, e in enumerate(v):
            if e["exact"]:
                print(g, i, "reference rel-L2 from the exact mix:", e["reference_rel_l2"])


if __name__ == "__main__":
    main()
