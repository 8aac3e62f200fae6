#!/usr/bin/env python3
"""
TEST INFRASTRUCTURE -- generates tests/golden/level.json (+ level.npz): what the REFERENCE returns for scaled and clipped audio
(``Volume`` / ``Clipping``, lhotse/augmentation/torchaudio.py:395-406 and clipping.py:28-61).

Needs the real lhotse (authoring container only):

    python tools/make_golden_level.py

soft_cases: for every case of tests/_level_ref.py::SOFT_CASES -- a deterministic signal (``_level_ref.signal``: the tests draw the same one,
nothing but its seed is stored) through a program with a soft ``Clipping`` -- the reference's own max-abs and rel-L2 distance from the
float64 truth (``_level_ref.exact``).  The GPU test takes its soft-clip bars from these figures.

Groups (fixed seeds), over the corpus of oracle/driver_corpus.py; ``lhotse.augmentation.torchaudio.is_torchaudio_available`` is set to
``lambda: True`` first, so that the oversampled form takes lhotse's own sinc module (as tools/make_golden_resample_chain.py does):
  1 volume                    perturb_volume                       5 speed_volume_clip_reverb  PerturbSpeed, then level ops on both sides of a reverb
  2 clip_hard                 clip_amplitude(hard=True)            6 volume_cutmix             PerturbVolume on the speech track, then CutMix
  3 clip_soft                 clip_amplitude(hard=False)           7 k2                        one K2SpeechRecognitionDataset batch with [PerturbSpeed,
  4 clip_oversampled          oversampling = 2 and 4                                            PerturbVolume, ClippingTransform, Reverb, CutMix]
Per cut: the track table as in reverb.json plus ``"level": [block in front of the reverb, block behind it]`` -- taken from the product's own
classifier and reader (``parse_chain``, ``deferred_mix``, ``_read_tracks``) with the audio backend logging what each track read --, the
wanted sample count and the reference's Fbank features.  Single-track cuts (all are short) keep ``load_audio()``; where the chain is more than
Volume / hard Clipping also the float64 truth (its float32 difference from ``load_audio()``) and the reference's own max-abs and rel-L2
distance from it.  The product's route is run over every table with the numpy statement of the device's arithmetic in place of the kernels:
its features meet the feature bar (rel-L2 <= 1e-4, max abs <= 2e-3), its audio equals the reference (groups 1, 2) or meets the chain's audio
bar (max abs <= 2 x the reference's own + 2^-24; group 3 also the soft bars).

Every Clipping of every stored case acts: the generator asserts that the peak it meets is at least 4 x SILENCE_PEAK and that the track
differs from the same chain without the Clipping by at least 1 % of its peak.

Asserted for every stored case (other inputs are to be picked if one fails): the numpy statement of the device's arithmetic
(``_level_ref.model32``: the float64 tanh rounded once) stays within the bars, max abs <= 2 x the reference's own + 2^-24 x peak and
rel-L2 <= 2 x the reference's own; and for the same programs with a HARD clip, ``model32`` is ``array_equal`` to the reference.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SAMPLING_RATE = 16000


def reference_program(x, program, Volume, Clipping):
    """One array through the reference's transforms, in order."""
    y = np.asarray(x, np.float32)[None, :]
    for op in program:
        fn = Volume(factor=op[1]) if op[0] == "volume" else Clipping(hard=op[1], gain_db=op[2], normalize=op[3])
        y = fn(y, SAMPLING_RATE)
        assert y.dtype == np.float32
    return y[0]


AUDIO_MAX = 9000  # single-track cuts up to this many samples keep their audio (the fixtures stay small)
REL_TOL, ABS_TOL = 1e-4, 2e-3  # the feature bar


def rir_pcm16(taps: int, peak: int, seed: int) -> np.ndarray:
    rs = np.random.RandomState(seed)
    h = rs.randn(taps) * np.exp(-5.0 * np.abs(np.arange(taps) - peak) / taps) * 0.12
    h[peak] = 1.0
    return np.round(h * 24000.0).astype(np.int16)


def chain_groups(meta):
    """The groups of cuts through the reference (module docstring) -> the arrays of level.npz; their tables go to meta["groups"]."""
    import random
    import tempfile
    from pathlib import Path

    import _level_golden as LG
    import _level_ref as L
    import _resample_chain as RC
    import _reverb_ref as RV
    from _dropin_support import install_wave_backend, make_cpu_plan
    from _mix_ref import mix_in_arena_cpu
    from oracle import resample_ref as R
    from oracle.driver_corpus import write_corpus, write_wav
    from test_level_reference import cpu_level
    from test_resample_chain_reference import cpu_perturb, cpu_resample, cpu_reverb

    install_wave_backend()
    import lhotse.augmentation.torchaudio as ref_ta

    ref_ta.is_torchaudio_available = lambda: True  # the reference's sinc branch: the oversampled clip takes lhotse's own sinc module
    from lhotse import CutSet, MonoCut, Recording, SupervisionSegment
    from lhotse.audio import AudioSource
    from lhotse.audio.backend import get_current_audio_backend
    from lhotse.dataset import K2SpeechRecognitionDataset
    from lhotse.dataset.cut_transforms import ClippingTransform, CutMix, PerturbSpeed, PerturbVolume, ReverbWithImpulseResponse
    from lhotse.dataset.input_strategies import OnTheFlyFeatures
    from lhotse.features.kaldi.extractors import Fbank

    import lhotse_amd as LA
    import lhotse_amd.extractors as E
    import lhotse_amd.input_strategies as IS

    # the numpy statement of the device's arithmetic drives the product's own route (tests/test_level_reference.py does the same)
    E._Plan = make_cpu_plan()
    IS._level_in_arena, IS._resample_in_arena, IS._perturb_in_arena, IS._mix_in_arena, IS._reverb_in_arena = cpu_level, cpu_resample, cpu_perturb, mix_in_arena_cpu, cpu_reverb
    torch.cuda.is_available = lambda: False

    backend = get_current_audio_backend()
    reads, inner = [], backend.read_audio

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
            if f["id"] in ids:
                rec = recording(f["id"], f["path"], f["num_samples"])
                sup = SupervisionSegment(id=f"sup-{f['id']}", recording_id=rec.id, start=0.0, duration=rec.duration, channel=0, text=f"text of {f['id']}")
                cuts.append(MonoCut(id=f["id"], start=0, duration=rec.duration, channel=0, recording=rec, supervisions=[sup] if supervised else []))
        return CutSet.from_cuts(sorted(cuts, key=lambda c: ids.index(c.id)))

    def table_of(cut):
        """-> the rows of the track table, through the product's classifier and reader; a plain cut is a cut of one track."""
        if type(cut).__name__ == "MixedCut":
            tracks = IS.deferred_mix(cut, gpu_resample=True, gpu_level=True)
            assert tracks is not None, cut
        else:
            chain = IS.parse_chain(cut)
            assert chain is not None, cut
            tracks = [IS.PendingTrack(cut, 0, None, True, chain)]
        rows = []
        for tr in tracks:
            del reads[:]
            (t,), _, _ = IS._read_tracks(cut, [tr])
            x, factor, off, snr, is_ref, n = t[:6]
            if isinstance(x, int):
                rows.append({"file": None, "first": 0, "count": int(x), "factor": 1.0, "offset": int(off), "snr": None, "ref": False, "num_samples": int(n)})
                continue
            assert len(reads) == 1 and reads[0][2] == len(x), (reads, len(x))
            row = {"file": reads[0][0], "first": reads[0][1], "count": len(x), "factor": float(factor), "offset": int(off),
                   "snr": None if snr is None else float(snr), "ref": bool(is_ref), "num_samples": int(n)}
            if t.reverb is not None:
                spec = tr.chain.reverb
                rid = spec["rir"]["id"] if isinstance(spec["rir"], dict) else spec["rir"].id
                assert not spec["early_only"] and np.array_equal(t.reverb[0], rir_loaded[rid[len("rec-"):]])
                row["reverb"] = {"rir": rid[len("rec-"):], "normalize": bool(t.reverb[1])}
            if t.levels is not None:
                assert t.source_rate is None
                row["level"] = [t.levels[0], t.levels[1]]
            rows.append(row)
        return rows

    def exact_track(row, x, clip=True, peaks=None):
        """The float64 chain of one track: Speed, the level block, the reverb, the level block, nothing rounded.  ``clip=False``: the same
        chain with its Clipping left out; ``peaks``: a list that receives the peak every Clipping meets."""
        y = RC.exact_track(x, None, row["factor"])
        for w in (0, 1):
            for st in LG.steps_of(row["level"][w]) or []:
                if st[0] == "level":
                    for op in st[1]:
                        if op[0] == "clip" and peaks is not None:
                            peaks.append(float(np.max(np.abs(y))))
                        if op[0] != "clip" or clip:
                            y = L.exact64(y, [op])
                else:
                    a, b = (SAMPLING_RATE, SAMPLING_RATE * st[1]) if st[0] == "up" else (SAMPLING_RATE * st[1], SAMPLING_RATE)
                    y = R.resample(y, a, b, dtype=np.float64)
            if w == 0 and row.get("reverb"):
                hs, shift = RV.scale_and_shift(rir_loaded[row["reverb"]["rir"]])
                y = RV.exact(y, hs, shift, row["reverb"]["normalize"])
        return y

    arrays, fb = {}, Fbank()
    meta.update(groups={}, rirs={"rir257": {"taps": 257, "peak": 0}, "rir3001": {"taps": 3001, "peak": 40}})
    rir_loaded, rir_recs = {}, {}
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        files = write_corpus(td / "wav")
        meta["files"] = [{k: v for k, v in f.items() if k != "path"} for f in files]
        for seed, (name, spec) in enumerate(meta["rirs"].items()):
            pcm = rir_pcm16(spec["taps"], spec["peak"], seed + 1)
            write_wav(td / "wav" / f"{name}.wav", pcm)
            arrays[f"rir/{name}"] = pcm
            rir_recs[name] = recording(name, td / "wav" / f"{name}.wav", spec["taps"])
            rir_loaded[name] = rir_recs[name].to_cut().load_audio()[0]
        paths = {f["id"]: f["path"] for f in files}

        def record(group, cuts, zero_pad=False):
            entries = []
            for i, cut in enumerate(cuts):
                rows = table_of(cut)
                want = int(cut.num_samples)
                ref_audio = cut.load_audio()[0]
                assert ref_audio.dtype == np.float32 and len(ref_audio) == want
                entries.append({"tracks": rows, "want": want, "audio": False})
                for r in rows:  # every Clipping of every stored case ACTS: its input is not silence, and the track differs from the unclipped chain
                    if r.get("level") and any(op[0] == "clip" for w in (0, 1) for st in LG.steps_of(r["level"][w]) or [] if st[0] == "level" for op in st[1]):
                        peaks, x = [], LG.track_samples(r, paths)
                        clipped, unclipped = exact_track(r, x, peaks=peaks), exact_track(r, x, clip=False)
                        assert peaks and min(peaks) >= 4.0 * float(L.SILENCE_PEAK), (group, i, peaks, "the clip meets silence: pick other inputs")
                        diff = float(np.max(np.abs(clipped - unclipped))) / float(np.max(np.abs(unclipped)))
                        print(f"{group}/{i}: peak at the clip {min(peaks):.3g}, the clip moves the track by {diff:.3g} of its peak")
                        assert diff >= 1e-2, (group, i, diff, "the clip leaves the track as it is: pick other inputs")
                arrays[f"{group}/{i}/feats"] = fb.extract(ref_audio, SAMPLING_RATE)
            # the product's route over the tables, with the numpy statement of the device's arithmetic: features and audio meet the bars
            ex = LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad")) if zero_pad else LA.HipFbank(LA.HipFbankConfig())
            rirs = {}
            tracks = [LG.tracks_of(e, paths, arrays, rirs) for e in entries]
            feats, lens, audio = IS.FusedMiniBatch(ex, return_audio=True).features_of_tracks(tracks, [e["want"] for e in entries], SAMPLING_RATE)
            for i, (cut, e) in enumerate(zip(cuts, entries)):
                key, rows = f"{group}/{i}", e["tracks"]
                model, ref_audio = audio[i].numpy(), cut.load_audio()[0]
                if not zero_pad:
                    w = arrays[f"{key}/feats"]
                    d = feats[i, : len(w)].numpy().astype(np.float64) - w
                    rel, mx = float(np.linalg.norm(d) / np.linalg.norm(w)), float(np.abs(d).max())
                    assert int(lens[i]) == len(w) and rel <= REL_TOL and mx <= ABS_TOL, (key, rel, mx)
                if zero_pad or len(rows) != 1 or e["want"] > AUDIO_MAX or not rows[0].get("level"):
                    continue  # (the K2 batch is held to its features alone)
                arrays[f"{key}/audio"] = ref_audio
                e["audio"] = True
                if group in LG.EXACT_GROUPS:
                    assert np.array_equal(model, ref_audio), key
                    continue
                truth = exact_track(rows[0], LG.track_samples(rows[0], paths))[: e["want"]]
                ref_max, ref_rel = L.distances(ref_audio, truth)
                m_max, m_rel = L.distances(model, truth)
                print(f"{key}: N {e['want']} reference {ref_max:.3g} / {ref_rel:.3g}  model {m_max:.3g} / {m_rel:.3g}")
                if group == "clip_soft":
                    bar_max, bar_rel = L.soft_bars(ref_max, ref_rel, truth)
                    assert m_max <= bar_max and m_rel <= bar_rel, (key, "the device's arithmetic misses the soft bar: pick other inputs")
                assert m_max <= 2.0 * ref_max + 2.0 ** -24, (key, "the device's arithmetic misses the chain's audio bar: pick other inputs")
                arrays[f"{key}/exact_minus_audio"] = (truth - ref_audio.astype(np.float64)).astype(np.float32)
                e.update(reference_max_abs=ref_max, reference_rel_l2=ref_rel)
            meta["groups"][group] = entries

        speech = cutset(files, ["utt6", "utt4", "utt2"])
        u6, u4, u2 = [c if c.id != "utt2" else c.truncate(offset=0.1, duration=0.45) for c in speech]  # (short cuts: small fixtures)
        noise = cutset(files, ["utt1", "utt7"], supervised=False)
        record("volume", [u6.perturb_volume(0.37), u4.perturb_volume(1.9), u2.perturb_volume(-0.8).perturb_volume(1.3)])
        record("clip_hard", [u6.clip_amplitude(hard=True, gain_db=12.0, oversampling=None), u4.perturb_volume(3.0).clip_amplitude(hard=True, gain_db=0.05, normalize=False, oversampling=None),  # (samples above 1 are what clips)
                             u2.perturb_volume(1.7).clip_amplitude(hard=True, gain_db=6.0, oversampling=None).perturb_volume(0.6)])
        record("clip_soft", [u6.clip_amplitude(hard=False, gain_db=12.0, oversampling=None), u4.clip_amplitude(hard=False, gain_db=0.0, normalize=False, oversampling=None),
                             u2.perturb_volume(1.7).clip_amplitude(hard=False, gain_db=20.0, oversampling=None)])
        record("clip_oversampled", [u6.clip_amplitude(hard=True, gain_db=12.0, oversampling=2), u4.clip_amplitude(hard=False, gain_db=6.0, oversampling=4),
                                    u2.perturb_volume(0.5).clip_amplitude(hard=False, gain_db=9.0).perturb_volume(1.5), u6.clip_amplitude(hard=True, gain_db=20.0, oversampling=4)])
        sp = list(PerturbSpeed(factors=[0.9, 1.1], p=1.0, randgen=random.Random(3))(CutSet.from_cuts([u6, u4, u2])))
        record("speed_volume_clip_reverb", [
            sp[0].perturb_volume(0.5).clip_amplitude(hard=True, gain_db=9.0, oversampling=None).reverb_rir(rir_recs["rir3001"]).perturb_volume(1.5),
            sp[1].perturb_volume(1.4).clip_amplitude(hard=False, gain_db=6.0, oversampling=None).reverb_rir(rir_recs["rir257"]),
            sp[2].reverb_rir(rir_recs["rir257"]).perturb_volume(0.7).clip_amplitude(hard=False, gain_db=3.0, oversampling=2)])  # (2: a clip BEHIND the reverb)
        vol = PerturbVolume(p=1.0, randgen=random.Random(7))
        record("volume_cutmix", list(CutMix(noise, snr=(10, 20), p=1.0, pad_to_longest=True, random_mix_offset=True, seed=11)(vol(CutSet.from_cuts([u6, u4, u2])))))

        k2cuts = cutset(files, ["utt0", "utt2", "utt4", "utt6", "utt1", "utt7", "utt3"])
        tf = [PerturbSpeed(factors=[0.9, 1.1], p=2 / 3, randgen=random.Random(23)), PerturbVolume(p=0.6, randgen=random.Random(26)),
              ClippingTransform(gain_db=(0.0, 24.0), p=0.5, seed=27), ReverbWithImpulseResponse(list(rir_recs.values()), p=0.5, randgen=random.Random(24)),
              CutMix(noise, snr=(10, 20), p=0.4, pad_to_longest=False, random_mix_offset=True, seed=25)]
        batch = K2SpeechRecognitionDataset(input_strategy=OnTheFlyFeatures(Fbank()), cut_transforms=tf, return_cuts=True)[k2cuts]
        bc = batch["supervisions"]["cut"]
        record("k2", bc, zero_pad=True)

        def kind(c):
            if type(c).__name__ == "MixedCut":
                return "mixed"
            names = [IS._transform_name(t) for t in (c.recording.transforms or [])]
            return "level" if set(names) & {"Volume", "Clipping"} else "speed" if names else "plain"

        meta["k2_kinds"] = [kind(c) for c in bc]
        assert {"mixed", "level"} <= set(meta["k2_kinds"]), meta["k2_kinds"]
        nf, inputs = batch["supervisions"]["num_frames"].numpy(), batch["inputs"].numpy()
        for i in range(len(bc)):
            arrays[f"k2/{i}/feats"] = inputs[i, : int(nf[i])]  # (the batch's rows replace the per-cut matrix: zero-padded framing)
        # ... and the route over the K2 tables meets the feature bar against the batch's own rows
        ex = LA.HipFbank(LA.HipFbankConfig(edge_rule="batch_zero_pad"))
        tracks = [LG.tracks_of(e, paths, arrays, {}) for e in meta["groups"]["k2"]]
        feats, lens, _ = IS.FusedMiniBatch(ex).features_of_tracks(tracks, [e["want"] for e in meta["groups"]["k2"]], SAMPLING_RATE)
        for i in range(len(bc)):
            w = arrays[f"k2/{i}/feats"]
            d = feats[i, : len(w)].numpy().astype(np.float64) - w
            assert int(lens[i]) == len(w) and np.linalg.norm(d) / np.linalg.norm(w) <= REL_TOL and np.abs(d).max() <= ABS_TOL, ("k2", i)
    return arrays


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    import _level_ref as L
    from _dropin_support import import_lhotse

    import_lhotse()
    from lhotse.augmentation import Clipping, Volume

    meta = {"sampling_rate": SAMPLING_RATE, "soft_cases": []}
    for name, seed, n, amp, program in L.SOFT_CASES:
        x = L.signal(seed, n, amp)
        ref = reference_program(x, program, Volume, Clipping)
        truth = L.exact(x, program)
        ref_max, ref_rel = L.distances(ref, truth)
        bar_max, bar_rel = L.soft_bars(ref_max, ref_rel, truth)
        m_max, m_rel = L.distances(L.model32(x, program), truth)
        print(f"{name}: reference {ref_max:.3g} / {ref_rel:.3g}  model {m_max:.3g} / {m_rel:.3g}  bars {bar_max:.3g} / {bar_rel:.3g}")
        assert m_max <= bar_max and m_rel <= bar_rel, (name, "the device's arithmetic misses the bar: pick other inputs")
        hard = [op if op[0] == "volume" else ("clip", True) + tuple(op[2:]) for op in program]
        assert np.array_equal(L.model32(x, hard), reference_program(x, hard, Volume, Clipping)), name
        meta["soft_cases"].append({"name": name, "seed": seed, "num_samples": n, "ref_max_abs": ref_max, "ref_rel_l2": ref_rel})

    arrays = chain_groups(meta)
    out_dir = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(out_dir, "level.npz"), **arrays)
    print("level.npz", os.path.getsize(os.path.join(out_dir, "level.npz")), "bytes;", {g: len(v) for g, v in meta["groups"].items()}, "k2:", meta["k2_kinds"])
    with open(os.path.join(out_dir, "level.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("level.json", os.path.getsize(os.path.join(out_dir, "level.json")), "bytes;", len(meta["soft_cases"]), "soft cases")


if __name__ == "__main__":
    main()
