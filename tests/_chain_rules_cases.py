"""The corpus of tests/golden/chain_rules.json: transform lists over a small alphabet on cuts that need no file (the rule of what the
device takes over reads manifests only).  Shared by the generator (tools/make_golden_chain_rules.py) and the test that holds the rule to
the record (tests/test_chain_rules_reference.py).  Needs the real lhotse (``_dropin_support.import_lhotse()`` first).

A list is written as a string of the letters of ``ALPHABET``.  The enumeration:

  * every list of length 0 ... 3, under every on/off combination of the four switches;
  * every list of length 4, and every list of length 5 over ``SHORT_ALPHABET``, with all switches on;
  * every list the record names as served, under every combination (the generator found those of length 4 and 5 over the whole alphabet).
"""
from itertools import product

SR = 16000
SWITCHES = ("gpu_speed", "gpu_reverb", "gpu_resample", "gpu_level")
COMBOS = list(product((True, False), repeat=4))  # mask bit i = COMBOS[i] serves the list
ALL_ON = COMBOS[0]


def _resample(src, dst):
    return {"name": "Resample", "kwargs": {"source_sampling_rate": src, "target_sampling_rate": dst}}


def _reverb(rir, channels):
    return {"name": "ReverbWithImpulseResponse", "kwargs": {"rir": rir, "normalize_output": True, "early_only": False, "rir_channels": channels}}


def alphabet():
    """letter -> the transform as a manifest carries it"""
    from lhotse import Recording
    from lhotse.audio import AudioSource

    rir = Recording(id="rir", sources=[AudioSource(type="file", channels=[0], source="rir.wav")], sampling_rate=SR, num_samples=300,
                    duration=300 / SR).to_dict()
    return {
        "A": _resample(8000, SR), "B": _resample(11127, SR), "C": _resample(SR, 2 * SR), "D": _resample(2 * SR, SR), "E": _resample(SR, 8000),
        "F": _resample(SR, 3 * SR), "G": _resample(SR, 9 * SR),
        "S": {"name": "Speed", "kwargs": {"factor": 1.1}}, "s": {"name": "Speed", "kwargs": {"factor": 1.0}},
        "V": {"name": "Volume", "kwargs": {"factor": 2.0}}, "K": {"name": "Clipping", "kwargs": {"hard": False, "gain_db": 0.0, "normalize": True}},
        "H": _reverb(rir, [0]), "h": _reverb(None, [0]), "J": _reverb(rir, [0, 1]),
        "T": {"name": "Tempo", "kwargs": {"factor": 1.1}},  # a transform the device never serves
    }


ALPHABET = "ABCDEFGSsVKHhJT"
SHORT_ALPHABET = "ACDESVKHhT"  # the lists of length 5 that are enumerated whether served or not


def words(letters, lengths):
    for n in lengths:
        for w in product(letters, repeat=n):
            yield "".join(w)


def base_cuts():
    """-> (a MonoCut over a one-channel 16 kHz recording, a MonoCut over channel 0 of a two-channel one, a MultiCut over both channels)"""
    from lhotse import MonoCut, MultiCut, Recording
    from lhotse.audio import AudioSource

    def rec(name, channels):
        return Recording(id=name, sources=[AudioSource(type="file", channels=channels, source=f"{name}.wav")], sampling_rate=SR, num_samples=SR,
                         duration=1.0)

    one, two = rec("one", [0]), rec("two", [0, 1])
    return (MonoCut(id="mono", start=0, duration=1.0, channel=0, recording=one), MonoCut(id="mono-of-two", start=0, duration=1.0, channel=0, recording=two),
            MultiCut(id="multi", start=0, duration=1.0, channel=[0, 1], recording=two))


def with_word(cut, word, letters, suffix=""):
    from lhotse.utils import fastcopy

    return fastcopy(cut, id=cut.id + suffix, recording=fastcopy(cut.recording, transforms=[letters[ch] for ch in word]))


def plain_chain(answer):
    """A ``Chain`` (or the 5 values of one) as json carries it: the reverb reduced to what tells one from another."""
    if answer is None:
        return None
    src, factor, pre, rv, post = answer

    def block(b):
        return None if b is None else [[st[0], [list(op) for op in st[1]]] if st[0] == "level" else list(st) for st in b]

    rv = None if rv is None else [rv["rir"]["id"], rv["normalize_output"], rv["early_only"], list(rv["rir_channels"])]
    return [src, factor, block(pre), rv, block(post)]


def mixed_cuts(picked, letters):
    """Two-track ``MixedCut``s: a track with one of the lists ``picked`` under a noise track at 10 dB, every other one padded as well
    -> [(id, cut)]."""
    from lhotse.cut import MixedCut, MixTrack, MonoCut, PaddingCut

    mono = base_cuts()[0]
    noise = MonoCut(id="noise", start=0, duration=0.5, channel=0, recording=mono.recording)
    out = []
    for i, w in enumerate(picked):
        tracks = [MixTrack(cut=with_word(mono, w, letters, f"-{w}"), type="MonoCut"), MixTrack(cut=noise, type="MonoCut", offset=0.25, snr=10.0)]
        if i % 2 == 0:
            tracks.append(MixTrack(cut=PaddingCut(id="pad", duration=0.5, sampling_rate=SR, feat_value=0.0, num_samples=SR // 2), type="PaddingCut", offset=1.0))
        out.append((f"mix-{w}", MixedCut(id=f"mix-{w}", tracks=tracks)))
    return out
