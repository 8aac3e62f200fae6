#!/usr/bin/env python3
"""
TEST INFRASTRUCTURE -- generates tests/golden/featmix.json (+ featmix.npz): what the REFERENCE returns from
``PrecomputedFeatures`` / ``collate_features`` (lhotse/dataset/collation.py:115-145) for cuts with stored features, ``CutMix`` and padding
included (``MixedCut.load_features``, lhotse/cut/mixed.py:1199-1309).

Needs the real lhotse (authoring container only); seconds on the CPU:

    python tools/make_golden_featmix.py

The signals of oracle/driver_corpus.py (utt0 ... utt7, at most 2.5 s) go through the reference's ``Fbank`` with 40 filters (half the
fixture of 80; the kernel tests run F = 80 on their own data), are quantised to binary16-representable float32 -- one set of fixtures
serves the binary16 and the float32 route -- and stored in ``hip_archive_f16``.  Groups (fixed seeds):
  right, left, both   plain cuts of unequal length through ``collate_features(pad_direction=...)``; ``both``'s tail holds log(2e-10)
  cutmix              ``CutMix(snr=(10, 20), pad_to_longest=True, random_mix_offset=True, seed=3)``, utt4..utt7 onto utt0..utt3: a cut with a
                      frame range only a later track covers and a cut with >= 5 tracks (both asserted here)
  snr_first           a MixedCut whose first track carries the SNR; its reference is track 1
  pad_value           ``pad(pad_feat_value=-5.0)``, right        off_by_one   a cut one frame longer than its stored matrix
  truncated           ``cut.truncate(offset=0.3, duration=0.7)``  k2           one ``K2SpeechRecognitionDataset`` batch with ``CutMix(p=0.5)``
                      (seed 21: two cuts mixed, two left plain; asserted here)
Per group: the byte arena exactly as ``HipPrecomputedFeatures`` packed it (binary16 rows), the table of ``FeatCut``s its classifier made,
the reference's batch and ``features_lens``, and per fold-form cut ``reference_max_abs``: the reference's own max-abs distance from the
float64 truth of tests/_featmix_ref.py.  The numpy model of the launches is checked against the bar here, before anything is written.
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

NUM_FILTERS = 40


def main():
    import tempfile
    from pathlib import Path

    import _featmix_ref as R
    from _dropin_support import import_lhotse

    import_lhotse()
    from lhotse import CutSet, MonoCut
    from lhotse.cut import MixedCut, MixTrack
    from lhotse.dataset import K2SpeechRecognitionDataset
    from lhotse.dataset.cut_transforms import CutMix
    from lhotse.dataset.input_strategies import PrecomputedFeatures
    from lhotse.features import Features
    from lhotse.features.kaldi.extractors import Fbank, FbankConfig
    from lhotse.supervision import SupervisionSegment
    from lhotse.utils import fastcopy

    import lhotse_amd.input_strategies as IS
    from lhotse_amd import HipPrecomputedFeatures
    from lhotse_amd.augmentation import FEATMIX_COPY
    from lhotse_amd.storage import HipArchiveF16Writer
    from oracle.driver_corpus import CORPUS, SAMPLING_RATE, pcm16

    torch.cuda.is_available = lambda: False
    captured = []

    def cpu_featmix(arena, table, num_features, row_frames, layout=None):
        host = arena.numpy().copy()
        captured.append((host, table, num_features, row_frames))
        return torch.from_numpy(R.batch(host, table, num_features, row_frames, model=True)), np.asarray([c.num_frames for c in table], dtype=np.int32)

    IS._featmix_in_arena = cpu_featmix
    extractor = Fbank(FbankConfig(num_filters=NUM_FILTERS))
    tmp = Path(tempfile.mkdtemp(prefix="featmix_golden_"))
    cuts = []
    with HipArchiveF16Writer(tmp / "feats") as w:
        for cid, kind, n, seed in CORPUS:
            m = extractor.extract(pcm16(kind, n, seed).astype(np.float32) / 32768.0, SAMPLING_RATE)
            m = np.asarray(m, dtype=np.float32).astype(np.float16).astype(np.float32)
            dur = n / SAMPLING_RATE
            f = Features(type="kaldi-fbank", num_frames=len(m), num_features=NUM_FILTERS, frame_shift=0.01, sampling_rate=SAMPLING_RATE, start=0.0,
                         duration=dur, storage_type=w.name, storage_path=w.storage_path, storage_key=w.write(cid, m), recording_id=cid, channels=0)
            sup = SupervisionSegment(id=cid, recording_id=cid, start=0.0, duration=dur, text="a")
            cuts.append(MonoCut(id=cid, start=0.0, duration=dur, channel=0, features=f, supervisions=[sup]))
    c = cuts
    short = CutSet.from_cuts([c[0], c[2], c[4]])
    mixed = CutMix(CutSet.from_cuts(c[4:]), snr=(10, 20), p=1.0, pad_to_longest=True, random_mix_offset=True, seed=3)(CutSet.from_cuts(c[:4]))
    snr_first = MixedCut(id="snr-first", tracks=[MixTrack(cut=c[2], snr=7.5), MixTrack(cut=c[6], offset=0.2)])
    longer = fastcopy(c[6], duration=c[6].duration + 0.01, features=fastcopy(c[6].features, duration=c[6].duration + 0.01, num_frames=c[6].num_frames + 1))
    groups = [("right", short, "right"), ("left", short, "left"), ("both", short, "both"), ("cutmix", mixed, "right"),
              ("snr_first", CutSet.from_cuts([snr_first]), "right"), ("pad_value", CutSet.from_cuts([c[4].pad(num_frames=70, pad_feat_value=-5.0)]), "right"),
              ("off_by_one", CutSet.from_cuts([longer, c[4]]), "left"), ("truncated", CutSet.from_cuts([c[0].truncate(offset=0.3, duration=0.7), c[6]]), "right")]
    meta, arrays = {"num_features": NUM_FILTERS, "groups": {}}, {}

    def record(name, ref, ref_lens):
        host, table, nf, rows = captured.pop()
        assert not captured and nf == NUM_FILTERS
        ref = ref.numpy()
        truth, model = R.batch(host, table, nf, rows), R.batch(host, table, nf, rows, model=True)
        entry = {"row_frames": int(rows), "cuts": []}
        for b, cut in enumerate(table):
            d = {"form": int(cut.form), "num_frames": int(cut.num_frames), "pad_value": float(cut.pad_value), "dst_first": int(cut.dst_first),
                 "ref_track": int(cut.ref_track),
                 "tracks": [[int(t.offset), int(t.frames), int(t.frames if t.rows is None else t.rows), bool(t.f16), int(t.first),
                             None if t.snr is None else float(t.snr), float(t.value)] for t in cut.tracks]}
            if cut.form == FEATMIX_COPY:
                assert np.array_equal(model[b].view(np.uint32), ref[b].view(np.uint32)), (name, b)
            else:
                d["reference_max_abs"] = float(np.abs(ref[b].astype(np.float64) - truth[b]).max())
                err = np.abs(model[b].astype(np.float64) - truth[b])
                assert d["reference_max_abs"] < 1e-5 and (err <= R.bar(truth[b], d["reference_max_abs"])).all(), (name, b, d["reference_max_abs"], float(err.max()))
                print(f"{name} cut {b}: {len(cut.tracks)} tracks, reference_max_abs {d['reference_max_abs']:.3e}, model {err.max():.3e}")
            entry["cuts"].append(d)
        meta["groups"][name] = entry
        arrays[f"{name}_arena"], arrays[f"{name}_ref"], arrays[f"{name}_lens"] = host, ref, ref_lens.numpy()
        return table

    for name, cs, direction in groups:
        ref, ref_lens = PrecomputedFeatures()(cs, pad_direction=direction)
        got, lens = HipPrecomputedFeatures(device="cpu")(cs, pad_direction=direction)
        assert torch.equal(lens, ref_lens) and got.shape == ref.shape
        meta["groups"].setdefault(name, {})
        table = record(name, ref, ref_lens)
        meta["groups"][name]["pad_direction"] = direction
        if name == "cutmix":  # (a) a frame range only a later track covers, (b) a cut of >= 5 tracks
            assert max(len(cut.tracks) for cut in table) >= 5
            covered = lambda tr, f: tr.first <= f < tr.first + tr.frames  # noqa: E731
            assert any(not any(covered(e, f) for e in cut.tracks[:k]) for cut in table for k in range(1, len(cut.tracks))
                       for f in range(cut.tracks[k].first, cut.tracks[k].first + cut.tracks[k].frames))
        if name == "both":
            assert np.allclose(ref.numpy()[1][-5:], np.log(2e-10), atol=1e-5)
    # seed 21 mixes the first and the third of the four (duration-sorted) cuts and leaves the other two plain
    mk = lambda s: K2SpeechRecognitionDataset(input_strategy=s, cut_transforms=[CutMix(CutSet.from_cuts(c[4:]), p=0.5, seed=21)])  # noqa: E731
    ref = mk(PrecomputedFeatures())[CutSet.from_cuts(c[:4])]
    got = mk(HipPrecomputedFeatures(device="cpu"))[CutSet.from_cuts(c[:4])]
    assert torch.equal(got["supervisions"]["num_frames"], ref["supervisions"]["num_frames"])
    table = record("k2", ref["inputs"], ref["supervisions"]["num_frames"])
    assert any(cut.form != FEATMIX_COPY for cut in table) and any(cut.form == FEATMIX_COPY for cut in table)  # a mixed and a plain cut
    assert any(t.snr is not None for cut in table for t in cut.tracks)
    meta["groups"]["k2"]["pad_direction"] = "right"
    meta["groups"]["k2"]["sequence_idx"] = ref["supervisions"]["sequence_idx"].tolist()
    out = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(out, "featmix.npz"), **arrays)
    with open(os.path.join(out, "featmix.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print("wrote", os.path.getsize(os.path.join(out, "featmix.npz")), "bytes of featmix.npz")


if __name__ == "__main__":
    main()
