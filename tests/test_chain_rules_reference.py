"""CPU, under the real lhotse (authoring container only): the ONE rule of the pending transform chain against the record of what the
five layered rules it replaced answered (tests/golden/chain_rules.json, tools/make_golden_chain_rules.py): over every transform list of
the corpus (tests/_chain_rules_cases.py), ``parse_chain`` serves exactly the recorded lists, with exactly the recorded ``Chain``, under
exactly the recorded switch combinations; ``pending_channel_chain`` and ``deferred_mix`` likewise."""
import json
import os

import pytest

import _chain_rules_cases as C
from test_audio_samples_reference import bound_to_lhotse  # noqa: F401  (the module-scoped binding to the real lhotse)

pytestmark = pytest.mark.reference
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_rules.json")


@pytest.fixture(scope="module")
def env(bound_to_lhotse):  # noqa: F811
    import lhotse.augmentation.torchaudio as ref_ta

    was = ref_ta.is_torchaudio_available
    ref_ta.is_torchaudio_available = lambda: True  # the reference's sinc branch, as when the record was written
    import lhotse_amd.input_strategies as IS

    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["alphabet"] == C.ALPHABET and golden["short_alphabet"] == C.SHORT_ALPHABET and tuple(golden["switches"]) == C.SWITCHES
    yield IS, golden, C.alphabet()
    ref_ta.is_torchaudio_available = was


def _answer(IS, cut, combo):
    ch = IS.parse_chain(cut, bankless=True, **dict(zip(C.SWITCHES, combo)))
    assert ch is None or isinstance(ch, IS.Chain)
    return C.plain_chain(ch)


def _check(IS, cut, word, letters, record, combos):
    """The answers for one list under ``combos`` against its entry of ``record`` (absent: refused under all of them)."""
    c = C.with_word(cut, word, letters)
    chain, mask = record.get(word, (None, 0))
    for i, combo in enumerate(C.COMBOS):
        if combo in combos:
            assert _answer(IS, c, combo) == (chain if mask >> i & 1 else None), (word, combo)


def test_the_record_is_not_empty(env):
    _, golden, _ = env
    served = golden["served"]
    steps = lambda c: [st for b in (c[2], c[4]) for st in b or ()]  # noqa: E731
    count = lambda pred: sum(1 for c, _ in served.values() if pred(c))  # noqa: E731
    assert len(served) == 1072 and golden["enumerated"] == {"all_combinations": 3616, "length_4": 15 ** 4, "length_5_short_alphabet": 10 ** 5,
                                                            "length_5_searched": 15 ** 5, "two_channel": 241, "multi": 241}
    # every field of a Chain away from its default, both kinds of bracket
    assert count(lambda c: c[0] is not None) == 585 and count(lambda c: c[1] != 1.0) == 235 and count(lambda c: c[2]) == 857
    assert count(lambda c: c[3]) == 639 and count(lambda c: c[4]) == 436
    assert count(lambda c: any(st[0] == "rate" for st in steps(c))) == 540 and count(lambda c: any(st[0] == "up" for st in steps(c))) == 51
    # per switch: lists that all switches on serve and that one switch off alone refuses
    for k, name in enumerate(C.SWITCHES):
        off = C.COMBOS.index(tuple(j != k for j in range(4)))
        assert sum(1 for _, mask in served.values() if mask & 1 and not mask >> off & 1) >= 200, name
    assert len(golden["two_channel"]) == 18 and len(golden["multi"]) == 12 and len(golden["mixed"]) == 40
    assert sum(1 for m in golden["mixed"].values() for v in m.values() if v is not None) == 58


def test_parse_chain_answers_what_the_layered_rules_answered(env):
    IS, golden, letters = env
    served = golden["served"]
    mono, mono_of_two, _ = C.base_cuts()
    n = 0
    for w in C.words(C.ALPHABET, range(4)):  # every list of length <= 3 under every combination
        _check(IS, mono, w, letters, served, C.COMBOS)
        n += 1
    assert n == golden["enumerated"]["all_combinations"]
    for w in served:  # every served list under every combination
        _check(IS, mono, w, letters, served, C.COMBOS)
    n4 = n5 = 0
    for w in C.words(C.ALPHABET, (4,)):  # everything else of length 4, and of length 5 over the short alphabet: refused
        _check(IS, mono, w, letters, served, (C.ALL_ON,))
        n4 += 1
    for w in C.words(C.SHORT_ALPHABET, (5,)):
        _check(IS, mono, w, letters, served, (C.ALL_ON,))
        n5 += 1
    assert (n4, n5) == (golden["enumerated"]["length_4"], golden["enumerated"]["length_5_short_alphabet"])
    n = 0
    for w in C.words(C.ALPHABET, range(3)):  # one channel of a two-channel recording: no level block
        _check(IS, mono_of_two, w, letters, golden["two_channel"], C.COMBOS)
        n += 1
    assert n == golden["enumerated"]["two_channel"]


def test_pending_channel_chain_answers_what_it_answered(env):
    IS, golden, letters = env
    multi = C.base_cuts()[2]
    combos = [(True, True), (True, False), (False, True), (False, False)]  # (gpu_speed, gpu_resample)
    n = 0
    for w in C.words(C.ALPHABET, range(3)):
        c = C.with_word(multi, w, letters)
        answer, mask = golden["multi"].get(w, (None, 0))
        for i, (gpu_speed, gpu_resample) in enumerate(combos):
            got = IS.pending_channel_chain(c, gpu_speed, gpu_resample)
            assert (None if got is None else [got[1], got[2]]) == (answer if mask >> i & 1 else None), (w, gpu_speed, gpu_resample)
            assert got is None or (got[0] is c and got[3:] == (0, None))
            assert IS.parse_chain(c, bankless=True) is None  # a MultiCut is not the mono rule's
        n += 1
    assert n == golden["enumerated"]["multi"]


def test_deferred_mix_answers_what_it_answered(env):
    IS, golden, letters = env
    cuts = C.mixed_cuts(golden["mixed_words"], letters)
    assert [name for name, _ in cuts] == list(golden["mixed"])
    for name, cut in cuts:
        for key, want in golden["mixed"][name].items():
            gpu_reverb, gpu_resample, gpu_level = (ch == "1" for ch in key)
            tracks = IS.deferred_mix(cut, gpu_reverb, gpu_resample=gpu_resample, gpu_level=gpu_level)
            got = None if tracks is None else [[t.offset, t.snr, bool(t.is_ref), C.plain_chain(t.chain)] for t in tracks]
            assert got == want, (name, key)
            if tracks is not None:
                assert all(isinstance(t, IS.PendingTrack) for t in tracks) and [t.cut.id for t in tracks] == [t.cut.id for t in cut.tracks]
                # gpu_speed is the reader's question to the tracks' factors: off, a track with a Speed other than 1 refuses the cut
                slow = IS.deferred_mix(cut, gpu_reverb, gpu_resample=gpu_resample, gpu_level=gpu_level, gpu_speed=False)
                assert (slow is None) == any(t.chain is not None and t.chain.factor != 1.0 for t in tracks) and slow in (None, tracks)
