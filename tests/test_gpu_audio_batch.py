"""GPU: ``FusedAudioBatch`` -- the augmentation chain in the arena, then the collate launch -- over the golden cuts of tests/golden/level.*,
mix.*, reverb.* and resample_chain.* that store the reference's per-cut ``audio``.

The bar is equality: ``FusedMiniBatch(ex, return_audio=True).features_of_tracks`` runs the same chain into the same arena and copies every
cut to the host; row ``i`` of the collated tensor up to ``want[i]`` must be those samples, bit for bit, and zero behind them.  That host
audio is held to the reference by tests/test_gpu_level_chain.py, test_gpu_mix.py, test_gpu_reverb.py and test_gpu_resample_chain.py at their
own bars; the groups whose chain is exact (``LG.EXACT_GROUPS``) are re-asserted here against the golden ``audio`` directly."""
import json
import os

import numpy as np
import pytest
import torch

import _level_golden as LG
import _mix_golden as MG
import _resample_chain as RC
import _reverb_golden as RG

import lhotse_amd as LA
from lhotse_amd.input_strategies import FusedAudioBatch, FusedMiniBatch

pytestmark = pytest.mark.gpu
SR = 16000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = {
    "level": (LG.load_level_goldens, LG.corpus_files, lambda e, paths, arrays, rirs: LG.tracks_of(e, paths, arrays, rirs)),
    "mix": (MG.load_mix_goldens, MG.corpus_files, lambda e, paths, arrays, rirs: MG.tracks_of(e, paths)),
    "reverb": (RG.load_reverb_goldens, RG.corpus_files, lambda e, paths, arrays, rirs: RG.tracks_of(e, paths, arrays)),
    "resample_chain": (RC.load_goldens, RC.source_files, lambda e, paths, arrays, rirs: RC.tracks_of(e, paths, arrays, rirs)),
}


def _groups_with_audio():
    out = []
    for family in FAMILIES:
        with open(os.path.join(GOLDEN, family + ".json")) as f:
            meta = json.load(f)
        with np.load(os.path.join(GOLDEN, family + ".npz")) as z:
            names = set(z.files)
        out += [(family, g) for g, entries in meta["groups"].items() if entries and all(f"{g}/{i}/audio" in names for i in range(len(entries)))]
    return out


GROUPS = _groups_with_audio()
_CACHE = {}


def _family(family, tmp_path_factory):
    if family not in _CACHE:
        load, files, tracks_of = FAMILIES[family]
        arrays, meta = load()
        _CACHE[family] = (arrays, meta, files(tmp_path_factory.mktemp(family + "wav"), meta), tracks_of)
    return _CACHE[family]


@pytest.fixture(scope="module")
def extractor():
    return LA.HipFbank(LA.HipFbankConfig(device="cuda:0"))


def test_every_family_has_groups_with_audio():
    assert {f for f, _ in GROUPS} == set(FAMILIES) and set(LG.EXACT_GROUPS) <= {g for f, g in GROUPS if f == "level"}


@pytest.mark.parametrize("family,group", GROUPS, ids=[f"{f}-{g}" for f, g in GROUPS])
def test_collated_audio_is_the_arena_audio(tmp_path_factory, extractor, family, group):
    arrays, meta, paths, tracks_of = _family(family, tmp_path_factory)
    entries = meta["groups"][group]
    rirs = {}
    tracks = [tracks_of(e, paths, arrays, rirs) for e in entries]
    wants = [int(e["want"]) for e in entries]
    feats, feat_lens, host_audio = FusedMiniBatch(extractor, return_audio=True).features_of_tracks(tracks, wants, SR)
    audio, lens = FusedAudioBatch("cuda:0").audio_of_tracks(tracks, wants, SR)
    assert audio.is_cuda and audio.dtype == torch.float32 and tuple(audio.shape) == (len(entries), max(wants))
    assert lens.tolist() == wants == [len(a) for a in host_audio]
    got = audio.cpu()
    for i, a in enumerate(host_audio):
        assert torch.equal(got[i, : wants[i]].view(torch.int32), a.view(torch.int32)), (family, group, i)
        assert not bool(got[i, wants[i] :].view(torch.int32).any()), (family, group, i)  # exactly zero behind the cut
        if family == "level" and group in LG.EXACT_GROUPS:
            assert np.array_equal(got[i, : wants[i]].numpy(), arrays[f"{group}/{i}/audio"]), (group, i)
    # the same call with the audio collated on the device: the features of the default call, the padded host audio
    f2, l2, a2, al2 = FusedMiniBatch(extractor, return_audio=True, audio_device=None).features_of_tracks(tracks, wants, SR)
    assert torch.equal(f2, feats) and torch.equal(l2, feat_lens) and al2.tolist() == wants and a2.is_cuda
    assert torch.equal(a2.cpu().view(torch.int32), torch.nn.utils.rnn.pad_sequence(host_audio, batch_first=True).view(torch.int32))
    # 2-byte samples: one rounding of the same values
    half, _ = FusedAudioBatch("cuda:0", torch.bfloat16).audio_of_tracks(tracks, wants, SR)
    assert torch.equal(half.cpu().view(torch.int16), got.to(torch.bfloat16).view(torch.int16))


def test_plain_cuts_are_pad_sequence_of_their_inputs(extractor):
    rs = np.random.RandomState(4)
    xs = [torch.from_numpy(rs.randn(n).astype(np.float32) * 0.1) for n in (4001, 16000, 1, 9000, 12345)]
    wants = [len(x) for x in xs]
    want = torch.nn.utils.rnn.pad_sequence(xs, batch_first=True)
    batch = FusedAudioBatch("cuda:0")
    audio, lens = batch.audio_of(xs, [1.0] * len(xs), wants, SR)
    assert audio.is_cuda and lens.tolist() == wants and torch.equal(audio.cpu().view(torch.int32), want.view(torch.int32))
    audio, lens = batch.audio_of([x.cuda() for x in xs], [1.0] * len(xs), wants, SR)  # device-resident cuts lie back to back in the arena
    assert torch.equal(audio.cpu().view(torch.int32), want.view(torch.int32))
    audio, lens = batch.audio_of_tracks([[(x.numpy(), 1.0, 0, None, True)] for x in xs], wants, SR)
    assert torch.equal(audio.cpu().view(torch.int32), want.view(torch.int32))
    # ... and through the mini-batch with the audio on the device: the features of the default call
    xs16 = [x for x in xs if len(x) >= 400]
    f1, l1, a1 = FusedMiniBatch(extractor, return_audio=True).features_of_tracks([[(x, 1.0, 0, None, True)] for x in xs16], [len(x) for x in xs16], SR)
    f2, l2, a2, al2 = FusedMiniBatch(extractor, return_audio=True, audio_device="cuda:0").features_of_tracks([[(x, 1.0, 0, None, True)] for x in xs16],
                                                                                                            [len(x) for x in xs16], SR)
    assert torch.equal(f1, f2) and torch.equal(l1, l2) and al2.tolist() == [len(x) for x in xs16]
    assert torch.equal(a2.cpu().view(torch.int32), torch.nn.utils.rnn.pad_sequence(a1, batch_first=True).view(torch.int32))


def test_speed_only_cuts_equal_the_mini_batch_audio(extractor):
    rs = np.random.RandomState(6)
    xs = [torch.from_numpy(rs.randn(n).astype(np.float32) * 0.1) for n in (8000, 16000, 11000, 5000)]
    factors, wants = [1.1, 1.0, 0.9, 0.95], [7272, 16000, 12222, 5263]  # (0.95 is outside the mixed launch's ratios: one launch per factor)
    for sel in ([0, 1, 2], [0, 1, 2, 3]):
        a, f, w = [xs[i] for i in sel], [factors[i] for i in sel], [wants[i] for i in sel]
        _, _, host_audio = FusedMiniBatch(extractor, return_audio=True)._perturb_and_extract(a, f, w, SR)
        audio, lens = FusedAudioBatch("cuda:0").audio_of(a, f, w, SR)
        assert lens.tolist() == w == [len(h) for h in host_audio]
        assert torch.equal(audio.cpu().view(torch.int32), torch.nn.utils.rnn.pad_sequence(host_audio, batch_first=True).view(torch.int32))
