#!/usr/bin/env python3
"""tests/golden/chain_rules.json: what the rule of the pending transform chain (``lhotse_amd.input_strategies.parse_chain``,
``pending_channel_chain``, ``deferred_mix``) answers over the corpus of tests/_chain_rules_cases.py, under the real lhotse.

The committed record was written by this enumeration BEFORE there was one rule: by the five layered ones of the commit in front of
``parse_chain`` (the level rule, else the resample rule, else the speed / reverb rule, in the reader's order), so that
tests/test_chain_rules_reference.py holds the one rule to the answers of the five.  Run it again only when the grammar changes on purpose.

The record names the SERVED lists with their answers; every other list of the enumeration is refused.  Per served list: the ``Chain`` (the
same under every switch combination that serves it -- asserted here) and the combinations that do, as a bit mask over
``_chain_rules_cases.COMBOS``.

    python tools/make_golden_chain_rules.py [--out tests/golden/chain_rules.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def chain_of(IS, cut, combo):
    """-> the 5 values of the cut's ``Chain`` or None"""
    gs, grv, grs, glv = combo
    ch = IS.parse_chain(cut, gpu_speed=gs, gpu_reverb=grv, gpu_resample=grs, gpu_level=glv, bankless=True)
    return None if ch is None else tuple(ch)


def channel_chain_of(IS, cut, gpu_speed, gpu_resample):
    """-> (source rate, factor) of a multi-channel cut or None"""
    ch = IS.pending_channel_chain(cut, gpu_speed, gpu_resample)
    return None if ch is None else (ch[1], ch[2])


def mix_tracks_of(IS, cut, gpu_reverb, gpu_resample, gpu_level):
    """-> [(offset, snr, is_ref, the 5 values of the track's ``Chain`` or None for padding)] or None"""
    tracks = IS.deferred_mix(cut, gpu_reverb, gpu_resample=gpu_resample, gpu_level=gpu_level)
    return None if tracks is None else [(t.offset, t.snr, t.is_ref, None if t.chain is None else tuple(t.chain)) for t in tracks]


def record(IS):
    import _chain_rules_cases as C

    letters = C.alphabet()
    mono, mono_of_two, multi = C.base_cuts()

    def served_under(cut, word, combos):
        """-> (the chain, the mask of the combinations that serve it) or None"""
        c = C.with_word(cut, word, letters)
        got = [chain_of(IS, c, combo) for combo in combos]
        hits = [g for g in got if g is not None]
        if not hits:
            return None
        assert all(C.plain_chain(g) == C.plain_chain(hits[0]) for g in hits), word
        return [C.plain_chain(hits[0]), sum(1 << i for i, g in enumerate(got) if g is not None)]

    served, counts = {}, {}
    short = list(C.words(C.ALPHABET, range(4)))
    counts["all_combinations"] = len(short)
    for w in short:
        r = served_under(mono, w, C.COMBOS)
        if r is not None:
            served[w] = r
    # lengths 4 and 5 over the WHOLE alphabet, all switches on: the served ones join the record under every combination
    counts["length_4"] = len(C.ALPHABET) ** 4
    counts["length_5_short_alphabet"] = len(C.SHORT_ALPHABET) ** 5
    counts["length_5_searched"] = len(C.ALPHABET) ** 5
    for w in C.words(C.ALPHABET, (4, 5)):
        if chain_of(IS, C.with_word(mono, w, letters), C.ALL_ON) is not None:
            served[w] = served_under(mono, w, C.COMBOS)
    two = {}
    multis = {}
    channel_combos = [(True, True), (True, False), (False, True), (False, False)]  # (gpu_speed, gpu_resample)
    for w in C.words(C.ALPHABET, range(3)):
        r = served_under(mono_of_two, w, C.COMBOS)
        if r is not None:
            two[w] = r
        c = C.with_word(multi, w, letters)
        got = [channel_chain_of(IS, c, *combo) for combo in channel_combos]
        hits = [g for g in got if g is not None]
        if hits:
            assert all(g == hits[0] for g in hits), w
            multis[w] = [list(hits[0]), sum(1 << i for i, g in enumerate(got) if g is not None)]
    counts["two_channel"] = counts["multi"] = sum(len(C.ALPHABET) ** n for n in range(3))
    names = sorted(served, key=lambda w: (len(w), w))
    refused = [w for w in short if w not in served]
    picked = names[:: max(1, len(names) // 30)][:30] + refused[:: max(1, len(refused) // 10)][:10]
    mixed = {}
    for name, cut in C.mixed_cuts(picked, letters):
        mixed[name] = {}
        for combo in C.COMBOS[:8]:  # (gpu_speed stays on: the reader asks it of the tracks' factors)
            tr = mix_tracks_of(IS, cut, *combo[1:])
            mixed[name]["".join("01"[int(b)] for b in combo[1:])] = None if tr is None else [[o, s, bool(r), C.plain_chain(ch)] for o, s, r, ch in tr]
    return {"alphabet": C.ALPHABET, "short_alphabet": C.SHORT_ALPHABET, "switches": list(C.SWITCHES), "channel_switches": ["gpu_speed", "gpu_resample"],
            "enumerated": counts, "served": {w: served[w] for w in names}, "two_channel": two, "multi": multis, "mixed_words": picked, "mixed": mixed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "chain_rules.json"))
    args = ap.parse_args()
    from _dropin_support import import_lhotse

    import_lhotse()
    import lhotse.augmentation.torchaudio as ref_ta

    ref_ta.is_torchaudio_available = lambda: True  # the reference's sinc branch, as in the other generators of the goldens
    import lhotse_amd.input_strategies as IS

    rec = record(IS)
    with open(args.out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(rec['served'])} served lists, {len(rec['two_channel'])} on two channels, {len(rec['multi'])} multi-channel, {len(rec['mixed'])} mixed cuts -> {args.out}")


if __name__ == "__main__":
    main()
