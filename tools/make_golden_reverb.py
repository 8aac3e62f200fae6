#!/usr/bin/env python3
"""
TEST INFRASTRUCTURE -- generates tests/golden/reverb.npz + reverb.json: what the REFERENCE returns for cuts reverberated with a recorded
impulse response (``cut.reverb_rir``, the ``ReverbWithImpulseResponse`` cut transform) over the corpus of oracle/driver_corpus.py, together
with the track tables of those cuts in plain numbers.

Needs the real lhotse (authoring container only):

    python tools/make_golden_reverb.py

RIRs: synthetic int16 WAVs (decaying noise with one dominant peak), their samples stored in the npz:
  rir257   257 taps, the peak at tap 0          rir4000  4000 taps, used with early_only (its first 800 taps), the peak at tap 37
  rir3001  3001 taps, the peak at the LAST tap  rir8003  8003 taps, the peak at tap 120

Groups (fixed seeds):
  1 reverb          plain cuts, reverberated (normalised)
  2 speed_reverb    PerturbSpeed([0.9, 1.1], p=1), then the reverb
  3 reverb_cutmix   speed, then reverb, then CutMix: the speech is reverberated, the noise is not
  4 options         early_only=True and normalize_output=False
  5 k2              one K2SpeechRecognitionDataset(OnTheFlyFeatures(Fbank()), cut_transforms=[PerturbSpeed(p=2/3),
                    ReverbWithImpulseResponse(p=0.5), CutMix(p=0.5)]) batch: reverberated, speed-only, mixed and plain cuts share it

Per cut: the track table as in mix.json, a reverberated track with ``"reverb": {"rir", "early_only", "normalize"}`` -- taken from the
product's own classifier and reader (``deferred_mix``, ``parse_chain``, ``_read_tracks``) with the audio backend logging which
samples of which file each track read --, the wanted sample count and the reference's Fbank features.  For the single-track cuts of groups
1, 2 and 4 up to AUDIO_MAX samples, over RIRs of 800 taps or more: ``load_audio()``; the exact float64 convolution (tests/_reverb_ref.py) of
the float32 samples the reference had in front of the reverb, scaled by the float64 gain, stored as its float32 difference from
``load_audio()``; the reference's own rel-L2 and max-abs distance from it; the float64 gain.

Asserted for every such case (other inputs are to be picked if one fails): the numpy statement of the device's summation order stays within
the audio bars (2 x the reference's own distances + 2^-24 [x peak]) and ONE serial float32 chain over all taps does not; for every
single-track cut: the reference's Fbank over the numpy model's audio meets the feature bar (rel-L2 <= 1e-4, max abs <= 2e-3) against the
reference's features.
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
RIRS = {"rir257": (257, 0, 1), "rir4000": (4000, 37, 2), "rir3001": (3001, 3000, 3), "rir8003": (8003, 120, 4)}  # taps, peak, seed


def rir_pcm16(taps: int, peak: int, seed: int) -> np.ndarray:
    rs = np.random.RandomState(seed)
    h = rs.randn(taps) * np.exp(-5.0 * np.abs(np.arange(taps) - peak) / taps) * 0.12
    h[peak] = 1.0
    return np.round(h * 24000.0).astype(np.int16)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    import _reverb_ref as R
    from _dropin_support import import_lhotse, install_wave_backend

    import_lhotse()
    install_wave_backend()
    from lhotse import CutSet, MonoCut, Recording, SupervisionSegment
    from lhotse.audio import AudioSource
    from lhotse.audio.backend import get_current_audio_backend
    from lhotse.augmentation import Speed
    from lhotse.dataset import K2SpeechRecognitionDataset
    from lhotse.dataset.cut_transforms import CutMix, PerturbSpeed, ReverbWithImpulseResponse
    from lhotse.dataset.input_strategies import OnTheFlyFeatures
    from lhotse.features.kaldi.extractors import Fbank
    from lhotse.utils import fastcopy

    import lhotse_amd.input_strategies as IS

    backend = get_current_audio_backend()
    reads = []
    inner = backend.read_audio

    def logging_read(path_or_fd, offset=0.0, duration=None, force_opus_sampling_rate=None):
        audio, sr = inner(path_or_fd, offset=offset, duration=duration, force_opus_sampling_rate=force_opus_sampling_rate)
        if not Path(str(path_or_fd)).stem.startswith("rir"):
            reads.append((Path(str(path_or_fd)).stem, int(round(offset * sr)), int(audio.shape[1])))
        return audio, sr

    backend.read_audio = logging_read

    def recording(cid, path, n):
        return Recording(id=f"rec-{cid}", sources=[AudioSource(type="file", channels=[0], source=str(path))], sampling_rate=SAMPLING_RATE,
                         num_samples=n, duration=n / SAMPLING_RATE)

    def cutset(files, ids, supervised=True):
        cuts = []
        for f in files:
            if f["id"] not in ids:
                continue
            rec = recording(f["id"], f["path"], f["num_samples"])
            sup = SupervisionSegment(id=f"sup-{f['id']}", recording_id=rec.id, start=0.0, duration=rec.duration, channel=0, text=f"text of {f['id']}")
            cuts.append(MonoCut(id=f["id"], start=0, duration=rec.duration, channel=0, recording=rec, supervisions=[sup] if supervised else []))
        return CutSet.from_cuts(sorted(cuts, key=lambda c: ids.index(c.id)))

    def rir_name(spec):
        rir = spec["rir"]
        rid = rir["id"] if isinstance(rir, dict) else rir.id
        return rid[len("rec-"):]

    def table_of(cut):
        """-> (rows of the track table, loaded tracks) through the product's classifier and reader; a plain cut is a cut of one track."""
        if type(cut).__name__ == "MixedCut":
            tracks = IS.deferred_mix(cut)
            assert tracks is not None, cut
        else:
            chain = IS.parse_chain(cut, gpu_resample=False, gpu_level=False)
            assert chain is not None, cut
            tracks = [IS.PendingTrack(cut, 0, None, True, chain)]
        rows, loaded = [], []
        for tr in tracks:
            del reads[:]
            res = IS._read_tracks(cut, [tr])
            assert res is not None
            t, = res[0]
            x, factor, off, snr, is_ref, n = t[:6]
            if isinstance(x, int):
                assert not reads
                rows.append({"file": None, "first": 0, "count": int(x), "factor": 1.0, "offset": int(off), "snr": None, "ref": False, "num_samples": int(n)})
            else:
                assert len(reads) == 1 and reads[0][2] == len(x), (reads, len(x))
                rows.append({"file": reads[0][0], "first": reads[0][1], "count": len(x), "factor": float(factor), "offset": int(off),
                             "snr": None if snr is None else float(snr), "ref": bool(is_ref), "num_samples": int(n)})
                if t.reverb is not None:
                    spec = tr.chain.reverb
                    rows[-1]["reverb"] = {"rir": rir_name(spec), "early_only": bool(spec["early_only"]), "normalize": bool(t.reverb[1])}
                    want_rir = rir_loaded[(rows[-1]["reverb"]["rir"], rows[-1]["reverb"]["early_only"])]
                    assert np.array_equal(t.reverb[0], want_rir)  # the product loaded what the reference loads
            loaded.append(x)
        return rows, loaded

    arrays, meta = {}, {"sampling_rate": SAMPLING_RATE, "groups": {}, "rirs": {k: {"taps": v[0], "peak": v[1]} for k, v in RIRS.items()}}
    fb = Fbank()
    rir_loaded = {}
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        files = write_corpus(td / "wav")
        meta["files"] = [{k: v for k, v in f.items() if k != "path"} for f in files]
        rir_recs = {}
        for name, (taps, peak, seed) in RIRS.items():
            pcm = rir_pcm16(taps, peak, seed)
            write_wav(td / "wav" / f"{name}.wav", pcm)
            arrays[f"rir/{name}"] = pcm
            rir_recs[name] = recording(name, td / "wav" / f"{name}.wav", taps)
            for early in (False, True):  # (rir.py:116-122)
                c = rir_recs[name].to_cut().with_channels([0])
                rir_loaded[(name, early)] = (c.truncate(duration=0.05) if early else c).load_audio()[0]
            assert int(np.argmax(rir_loaded[(name, False)])) == peak
        assert len(rir_loaded[("rir4000", True)]) == 800 and np.array_equal(rir_loaded[("rir4000", True)], arrays["rir/rir4000"][:800].astype(np.float32) / 32768.0)

        speech = cutset(files, ["utt6", "utt4", "utt2"])
        speech = CutSet.from_cuts([c if c.id != "utt2" else c.truncate(offset=0.1, duration=0.45) for c in speech])  # (short cuts: small fixtures)
        noise = cutset(files, ["utt1", "utt7"], supervised=False)

        def record(group, cuts, audio=True):
            out = []
            for i, cut in enumerate(cuts):
                rows, loaded = table_of(cut)
                want = int(cut.num_samples)
                ref_audio = cut.load_audio()[0]
                assert ref_audio.dtype == np.float32 and len(ref_audio) == want
                key = f"{group}/{i}"
                entry = {"tracks": rows, "want": want, "audio": False}
                arrays[f"{key}/feats"] = fb.extract(ref_audio, SAMPLING_RATE)
                rv = rows[0].get("reverb") if len(rows) == 1 else None
                if rv is not None:
                    # the float32 samples the reference had in front of the reverb: the same cut without the transform
                    # (behind a Speed: the UNTRUNCATED resampled segment -- the reverb and its powers see all of it, the sample or two
                    # that assert_and_maybe_fix_num_samples removes come off afterwards, recording.py:1032-1070)
                    if rows[0]["factor"] != 1.0:
                        x_in = Speed(factor=rows[0]["factor"])(loaded[0][None, :], SAMPLING_RATE)[0]
                    else:
                        x_in = fastcopy(cut, recording=fastcopy(cut.recording, transforms=None)).load_audio()[0]
                    assert want <= len(x_in) <= want + 2
                    hs, shift = R.scale_and_shift(rir_loaded[(rv["rir"], rv["early_only"])])
                    model = R.chunked32(x_in, hs, shift, rv["normalize"])[:want]
                    f_model = fb.extract(model, SAMPLING_RATE)
                    d = f_model.astype(np.float64) - arrays[f"{key}/feats"]
                    rel, mx = float(np.linalg.norm(d) / np.linalg.norm(arrays[f"{key}/feats"])), float(np.abs(d).max())
                    assert rel <= 1e-4 and mx <= 2e-3, (group, i, rel, mx)
                    if audio and want <= AUDIO_MAX and len(hs) >= 800:
                        truth = R.exact(x_in, hs, shift, rv["normalize"])[:want]
                        ref_rel, ref_max = R.distances(ref_audio, truth)
                        bar_rel, bar_max = R.bars(ref_rel, ref_max, truth)
                        m_rel, m_max = R.distances(model, truth)
                        s_rel, s_max = R.distances(R.chunked32(x_in, hs, shift, rv["normalize"], chunk=None)[:want], truth)
                        print(f"{key}: N {want} L {len(hs)} reference {ref_rel:.3g} / {ref_max:.3g}  model {m_rel:.3g} / {m_max:.3g}  serial {s_rel:.3g} / {s_max:.3g}")
                        assert m_rel <= bar_rel and m_max <= bar_max, (group, i, "the device's order misses the bar: pick other inputs")
                        assert s_rel > bar_rel or s_max > bar_max, (group, i, "a serial chain meets the bar: pick other inputs")
                        arrays[f"{key}/audio"] = ref_audio
                        arrays[f"{key}/exact_minus_audio"] = (truth - ref_audio.astype(np.float64)).astype(np.float32)
                        g = R._gain64(x_in, R.exact(x_in, hs, shift, False)) if rv["normalize"] else 1.0
                        entry.update(audio=True, reference_rel_l2=ref_rel, reference_max_abs=ref_max, gain=float(g))
                out.append(entry)
            meta["groups"][group] = out

        u6, u4, u2 = list(speech)
        record("reverb", [u6.reverb_rir(rir_recs["rir3001"]), u4.reverb_rir(rir_recs["rir8003"]), u2.reverb_rir(rir_recs["rir257"]),
                          u2.reverb_rir(rir_recs["rir8003"])])
        sp = list(PerturbSpeed(factors=[0.9, 1.1], p=1.0, randgen=random.Random(3))(speech))
        record("speed_reverb", [sp[0].reverb_rir(rir_recs["rir8003"]), sp[1].reverb_rir(rir_recs["rir3001"]), sp[2].reverb_rir(rir_recs["rir257"])])
        rvb = ReverbWithImpulseResponse(list(rir_recs.values()), p=1.0, randgen=random.Random(5))
        sp2 = PerturbSpeed(factors=[0.9, 1.1], p=1.0, randgen=random.Random(4))
        record("reverb_cutmix", list(CutMix(noise, snr=(10, 20), p=1.0, pad_to_longest=True, random_mix_offset=True, seed=11)(rvb(sp2(speech)))), audio=False)
        record("options", [u6.reverb_rir(rir_recs["rir4000"], early_only=True), u4.reverb_rir(rir_recs["rir8003"], normalize_output=False),
                           u2.reverb_rir(rir_recs["rir4000"], early_only=True, normalize_output=False)])

        k2cuts = cutset(files, ["utt0", "utt2", "utt4", "utt6", "utt1", "utt7", "utt3"])
        tf = [PerturbSpeed(factors=[0.9, 1.1], p=2 / 3, randgen=random.Random(23)),
              ReverbWithImpulseResponse(list(rir_recs.values()), p=0.5, randgen=random.Random(24)),
              CutMix(noise, snr=(10, 20), p=0.5, pad_to_longest=False, random_mix_offset=True, seed=25)]
        ds = K2SpeechRecognitionDataset(input_strategy=OnTheFlyFeatures(Fbank()), cut_transforms=tf, return_cuts=True)
        batch = ds[k2cuts]
        bc = batch["supervisions"]["cut"]
        record("k2", bc, audio=False)

        def kind(c):
            if type(c).__name__ == "MixedCut":
                return "mixed"
            names = [IS._transform_name(t) for t in (c.recording.transforms or [])]
            return "reverb" if "ReverbWithImpulseResponse" in names else "speed" if names else "plain"

        kinds = [kind(c) for c in bc]
        assert {"mixed", "reverb", "speed", "plain"} <= set(kinds), kinds
        meta["k2_kinds"] = kinds
        nf = batch["supervisions"]["num_frames"].numpy()
        inputs = batch["inputs"].numpy()
        for i in range(len(bc)):
            arrays[f"k2/{i}/feats"] = inputs[i, : int(nf[i])]  # (the batch's rows replace the per-cut matrix: zero-padded framing)
        arrays["k2/num_frames"] = nf
        arrays["k2/shape"] = np.array(inputs.shape, dtype=np.int32)

    out_dir = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(out_dir, "reverb.npz"), **arrays)
    with open(os.path.join(out_dir, "reverb.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("reverb.npz", os.path.getsize(os.path.join(out_dir, "reverb.npz")), "bytes;", {g: len(v) for g, v in meta["groups"].items()}, "k2:", meta["k2_kinds"])


if __name__ == "__main__":
    main()
