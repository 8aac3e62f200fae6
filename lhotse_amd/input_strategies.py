"""
``HipOnTheFlyFeatures`` -- lhotse's ``OnTheFlyFeatures`` input strategy (lhotse/dataset/input_strategies.py:351-476)
with the extraction + collation step fused on the GPU and, since round 3, the speed
perturbation of ``PerturbSpeed``-ed cuts moved there too.

The reference computes a list of per-cut feature matrices and then ``collate_matrices(..., padding_value=LOG_EPSILON)``
copies each of them into a fresh padded tensor (lhotse/dataset/collation.py:506-535).  Here the kernels write every
cut straight into its slot of the ``(B, Tmax, F)`` tensor and only the padding rows are filled
(``hipfeat_extract_collated``); audio reading, wave transforms, ``return_audio`` / ``fault_tolerant`` outputs and the
supervision helpers are inherited unchanged.

The rule.  Which of a recording's pending transforms the device takes over is decided in ONE place, ``parse_chain``: one walk over the
transform list of a mono cut, left to right, against the grammar ``[Resample]? [Speed]? L? [Reverb]? L?`` (L = a block of level ops), each
element behind its switch (``gpu_resample`` / ``gpu_speed_perturb`` / ``gpu_level`` / ``gpu_reverb``) -> a ``Chain(source_rate, factor,
pre, reverb, post)`` or None = the reference's ``cut.load_audio()``.  ``pending_channel_chain`` (a ``MultiCut``) and ``deferred_mix`` (the
tracks of a ``MixedCut``: a ``PendingTrack(cut, offset, snr, is_ref, chain)`` each) ask the same walk.  A cut the rule serves is read ONCE
in front of its whole chain (``read_before_chain``; a chain that keeps the length: ``load_audio()`` of the cut without its transforms)
into a ``Track(samples, factor, offset, snr, is_ref, cap, reverb, source_rate, levels)``, what ``FusedMiniBatch.features_of_tracks``
consumes; a chain whose output would be shorter than the cut (``chain_num_samples``: the reference reflect-pads it) goes back to
``cut.load_audio()``.  The paragraphs below say what each element of the grammar is and what the device does with it.

Speed perturbation.  ``PerturbSpeed`` (lhotse/dataset/cut_transforms/perturb_speed.py:8-47) turns a cut into one whose
recording carries a ``Speed(factor)`` transform; the resampling itself then happens on the CPU inside
``Recording.load_audio`` (lhotse/audio/recording.py:431-490), one torch ``conv1d`` per cut, before the strategy ever
sees the samples -- it is what an on-the-fly pipeline spends its time in once the features are on the GPU.  With
``gpu_speed_perturb=True`` (default) a cut with that ``Speed`` pending is read WITHOUT it -- the
very segment of the original file ``load_audio`` would read, through the same ``reverse_timestamps`` /
``AudioSource.load_audio`` calls -- and the batch is perturbed on the device, mixed factors and all, in the arena the
feature launch reads from (``lhotse_amd.augmentation.perturb_speed_in_arena``).  Sample counts follow
``assert_and_maybe_fix_num_samples`` (truncate; the rare cut that would need reflect-padding takes the reference's own
path), values agree with the CPU ``Speed`` to the resampler's 1e-5.  A mini-batch in which a ``Speed`` is all that is pending takes the route of
``FusedMiniBatch.features_of`` (one launch for all factors).

Mixed cuts.  ``CutMix`` / ``CutSet.mix`` / ``.pad`` turn a cut into a ``MixedCut`` whose samples come out of
``MixedCut.load_audio`` (lhotse/cut/mixed.py:1312-1409): every track is loaded (its ``Speed`` on the CPU), its energy is
taken, a gain is computed from its SNR, and ``AudioMixer`` adds the scaled tracks at their offsets
(lhotse/audio/mixer.py:10-172).  With ``gpu_mix`` (default: on unless ``wave_transforms`` are given, as for the speed) the
tracks of an eligible mixed cut are loaded one by one, the way a mono cut is, and the batch is mixed on the device behind the
resampler: energy launch, mix launch, then the unchanged feature launch over the mixed samples
(``FusedMiniBatch.features_of_tracks``, ``lhotse_amd.augmentation.mix_in_arena``).  Unperturbed tracks come out within the
reference's own float32 rounding of the exact mix (the energies are float64 here, float32 pairwise sums there; bit-equal when no
gain is involved), perturbed ones within the resampler's 1e-5.  ``deferred_mix`` says which cuts qualify; everything else --
multi-channel or nested tracks, other transforms, a ``MixedCut`` with transforms of its own, video, a mix that needs reflect-
padding, a first track with an SNR against another reference track, a muted reference track -- takes ``cut.load_audio()``, and a
mini-batch may combine device-mixed, plain, speed-only and fallback cuts freely.

Reverberation.  ``ReverbWithImpulseResponse`` (lhotse/augmentation/rir.py:12-166; ``cut.reverb_rir``) appends itself to the recording's
transforms and ``Recording.load_audio`` then convolves the loaded (and speed-perturbed) samples with the RIR through three full-length
float32 FFTs on the CPU.  With ``gpu_reverb`` (default: on unless ``wave_transforms`` are given) a recording whose transforms are
``[Reverb]`` or ``[Speed, Reverb]`` (with level blocks around the reverb, below) with a RECORDED RIR and one ``rir_channels`` entry is read in front of them, the RIR is loaded on the
host with the reference's own calls, and the convolution runs on the device between the resampler and the mix
(``lhotse_amd.augmentation.reverb_in_arena``: direct form, float32, within 2 x the reference's own distance from the exact float64
convolution).  ``rir=None`` (the random generator), several ``rir_channels``, a reverb in front of a ``Speed`` and a ``MixedCut`` whose own
``transforms`` hold the reverb (``mix_first``) keep the reference's path.

Resampling.  ``cuts.resample(sr)`` puts a ``Resample(a -> sr)`` at the front of the recording's transforms (lhotse/audio/recording.py:905-935)
and ``Recording.load_audio`` then runs the sinc resampler on the CPU (44.1 -> 16 kHz: 160 filters of 475 taps).  With ``gpu_resample``
(default: on unless ``wave_transforms`` are given, and only where the reference itself runs its sinc resampler: torchaudio importable,
backend ``default``) a mono recording whose transforms are ``[Resample]? [Speed]? ...`` is read in front of ALL of them at the
source rate (``read_before_chain``), and the chain runs on the device: the rate conversion first, one launch per distinct source rate
(``lhotse_amd.augmentation.resample_in_arena``; the many-phase ratios on the matrix cores), then the ``Speed`` as a second pass over
its output, then reverb and mix as before.  A ``Resample`` that is not first (other than the brackets of a level block, below),
the ``sox`` backend and a pair of rates no kernel serves (``resample_route``) keep the reference's path.

Level changes.  ``PerturbVolume`` appends a ``Volume`` to the recording's transforms, the ``Clipping`` cut transform / ``cut.clip_amplitude`` a
``Clipping`` -- with ``oversampling=k`` between ``Resample(sr -> k sr)`` and ``Resample(k sr -> sr)`` (lhotse/audio/recording.py:937-975).  With
``gpu_level`` (default: on unless ``wave_transforms`` are given) a mono recording whose transforms are ``[Resample]? [Speed]? L? [Reverb]? L?``, L =
1 ... 4 such ops with at most one ``Clipping``, is read in front of all of them and scaled / clipped on the device, in place, behind the speed
pass and on both sides of the reverb (``lhotse_amd.augmentation.level_in_arena``: ``Volume`` and hard ``Clipping`` bit for bit, soft ``Clipping`` as
the float64 tanh rounded once); the oversampled form takes two more resample passes and needs the resampling route, as does the band
bracket ``Resample(sr -> m) Resample(m -> sr)`` of ``LowpassUsingResampling``, which counts as two ops of a block.
``deferred_mix(..., gpu_level=True)`` lets such tracks into a device mix.  A level op in front of the ``Speed``, more than 4 ops or two
``Clipping``s in a block, k outside 2 ... 8 and a recording of several channels keep the reference's path.

Raw audio.  ``AudioSamples`` (lhotse/dataset/input_strategies.py:208-299) and ``return_audio=True`` want the cuts' SAMPLES as one zero-padded
``(B, Tmax)`` tensor (``collate_audio``, lhotse/dataset/collation.py:148-260).  The chain above leaves them ragged in the arena; one launch
(``lhotse_amd.augmentation.collate_in_arena``) writes the dense tensor from there.  ``FusedAudioBatch`` is ``FusedMiniBatch`` with that launch in
place of the feature launch, ``HipAudioSamples`` the drop-in for ``AudioSamples``; ``return_audio_device=None`` (or a device) on
``HipOnTheFlyFeatures`` collates the audio of ``return_audio`` there too, instead of one blocking copy per cut and a host ``collate_vectors``.

Multi-channel cuts.  ``collate_audio(..., mono_downmix=None | True | False)`` (lhotse/dataset/collation.py:215-241) downmixes a ``MultiCut`` with
``audio.mean(dim=0)`` on the CPU or collates ``(B, C, T)``.  ``HipAudioSamples`` serves both (``gpu_channels``): every channel of a ``MultiCut``
whose recording's transforms are ``[Resample]? [Speed]?`` (``pending_channel_chain``; padded to the right or to the left as well) is a row of its
own in the arena and runs the chain like a mono cut, and ONE launch of the collate kernel's sources form
(``lhotse_amd.augmentation.collate_sources_in_arena``) writes ``(B, Tmax)`` -- a row is the float64 sum of the cut's channels, divided once,
rounded once -- or ``(B, Cmax, Tmax)`` with zero rows for the channels a cut does not have (``FusedAudioBatch.audio_of_channels``).  Mono cuts in
such a batch keep their whole chain.  Other transforms on a multi-channel cut, a multi-channel track mixed with audio and more than 32 channels
keep the reference's path for the batch.

Needs lhotse (it consumes ``CutSet``s); importing this module without lhotse works, constructing the classes does not.
"""
from __future__ import annotations

from math import gcd, isclose
from typing import List, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from .compat import HAVE_LHOTSE, LOG_EPSILON


BANK_RATIOS = ((9, 10), (11, 10))  # orig : new of the mixed launch's compile-time resamplers (hipfeat_speed_bank_create) = speed 0.9 / 1.1


def _bank_ratio_ok(sampling_rate: int, factor: float) -> bool:
    """Speed(factor) resamples round(sr * factor) -> sr (lhotse/augmentation/torchaudio.py:37-42); the mixed launch serves the ratios
    of BANK_RATIOS after reduction by the gcd (resample.py:219-222)."""
    import math

    orig, new = int(round(sampling_rate * factor)), int(sampling_rate)
    g = math.gcd(orig, new)
    return g > 0 and (orig // g, new // g) in BANK_RATIOS


def _perturb_in_arena(arena, offsets, lengths, factors, sampling_rate, tail_start):
    """(indirection for the CPU stand-in of the tests)"""
    from .augmentation import perturb_speed_in_arena

    return perturb_speed_in_arena(arena, offsets, lengths, factors, sampling_rate, tail_start)


def _resample_in_arena(arena, offsets, lengths, ratios, tail_start):
    """(indirection for the CPU stand-in of the tests)"""
    from .augmentation import resample_in_arena

    return resample_in_arena(arena, offsets, lengths, ratios, tail_start)


def _mix_in_arena(arena, track_first, src_offsets, src_lens, dst_offsets, snrs, ref_tracks, max_samples, tail_start):
    """(indirection for the CPU stand-in of the tests)"""
    from .augmentation import mix_in_arena

    return mix_in_arena(arena, track_first, src_offsets, src_lens, dst_offsets, snrs, ref_tracks, max_samples, tail_start)


def _reverb_in_arena(arena, src_offsets, src_lens, rir_offsets, rir_lens, shifts, normalize, tail_start, method="direct"):
    """(indirection for the CPU stand-in of the tests; with the direct form it is called without ``method``, as before there was one)"""
    from .augmentation import reverb_in_arena

    return reverb_in_arena(arena, src_offsets, src_lens, rir_offsets, rir_lens, shifts, normalize, tail_start, method=method)


def _checked_reverb_method(method: str) -> str:
    from .augmentation import reverb_method_code

    reverb_method_code(method)  # (ValueError for an unknown one)
    return method


def _level_in_arena(arena, src_offsets, src_lens, programs):
    """(indirection for the CPU stand-in of the tests)"""
    from .augmentation import level_in_arena

    return level_in_arena(arena, src_offsets, src_lens, programs)


def _collate_in_arena(arena, offsets, lengths, row_len, dtype):
    """(indirection for the CPU stand-in of the tests) -> the dense zero-padded (B, row_len) tensor on the arena's device"""
    from .augmentation import collate_in_arena

    return collate_in_arena(arena, offsets, lengths, row_len=row_len, dtype=dtype)[0]


def _collate_sources_in_arena(arena, first, src_offsets, lengths, row_len, dst_offsets, dtype):
    """(indirection for the CPU stand-in of the tests) -> the dense (rows, row_len) tensor whose row r is the mean of its sources"""
    from .augmentation import collate_sources_in_arena

    return collate_sources_in_arena(arena, first, src_offsets, lengths, row_len=row_len, dst_offsets=dst_offsets, dtype=dtype)[0]


class Chain(NamedTuple):
    """What the device takes over of a recording's transform list (``parse_chain``): the rate the samples are read at when a ``Resample``
    leads the list, the factor of the pending ``Speed`` (1.0 = none), the level block in front of the reverb, the reverb's kwargs, the
    level block behind it.  A block is None or a list of steps ``("level", [ops])`` / ``("up", k)`` / ``("down", k)`` /
    ``("rate", src, dst)`` (``FusedMiniBatch.features_of_tracks``)."""

    source_rate: Optional[int] = None
    factor: float = 1.0
    pre: Optional[list] = None
    reverb: Optional[dict] = None
    post: Optional[list] = None

    @property
    def pending(self) -> bool:
        """Whether there is anything for the device to do."""
        return self != Chain()

    @property
    def levels(self) -> Optional[tuple]:
        return None if self.pre is None and self.post is None else (self.pre, self.post)

    @property
    def keeps_length(self) -> bool:
        """No element that changes the sample count: no ``Resample``, no ``Speed``, no rate step in a level block."""
        return self.source_rate is None and self.factor == 1.0 and all(st[0] == "level" for b in (self.pre, self.post) for st in b or ())


class PendingTrack(NamedTuple):
    """An audible track of a ``MixedCut`` the device mixes (``deferred_mix``), before it is read; ``chain`` None: a ``PaddingCut``."""

    cut: object
    offset: int
    snr: Optional[float]
    is_ref: bool
    chain: Optional[Chain]


class Track(NamedTuple):
    """A track as ``FusedMiniBatch.features_of_tracks`` / ``FusedAudioBatch.audio_of_tracks`` consume it (a plain tuple of the first 5
    to 9 values is taken as well): the samples in front of the pending chain -- or, for a ``PaddingCut`` track, their count --, the
    ``Speed`` factor still to be applied, the first sample inside the cut, the SNR in dB or None, whether it is the cut's SNR reference
    track, the sample count it is truncated to, ``(rir_samples, normalize_output)``, the rate the samples are at, the level blocks
    ``(in front of the reverb, behind it)``."""

    samples: object
    factor: float
    offset: int
    snr: Optional[float]
    is_ref: bool
    cap: Optional[int] = None
    reverb: Optional[tuple] = None
    source_rate: Optional[int] = None
    levels: Optional[tuple] = None


class _Tracks(list):
    """The cuts of a mini-batch as lists of ``Track``s, normalised (``_as_tracks``)."""


def _as_tracks(cuts_tracks, sampling_rate: int) -> _Tracks:
    """Every incoming track as a ``Track``, once; a source rate that is the mini-batch's own and a pair of empty level blocks are none.
    (Plain loops: this runs per track of every mini-batch, in front of launches that take a fraction of a millisecond.)"""
    if type(cuts_tracks) is _Tracks:
        return cuts_tracks
    sr = int(sampling_rate)
    out = _Tracks()
    for tracks in cuts_tracks:
        row = []
        for tr in tracks:
            if type(tr) is not Track:
                tr = Track(*tr)
            if tr.source_rate is not None and int(tr.source_rate) == sr:
                tr = tr._replace(source_rate=None)
            if tr.levels is not None and not (tr.levels[0] or tr.levels[1]):
                tr = tr._replace(levels=None)
            row.append(tr)
        out.append(row)
    return out


def _is_padding(track: Track) -> bool:
    return isinstance(track.samples, (int, np.integer))


def _is_plain(tracks) -> bool:
    """One track with samples that starts at 0 and is not scaled: the cut IS that track (a MonoCut, speed-perturbed or not; when the
    track carries a reverb, the cut is the reverb's output)."""
    return len(tracks) == 1 and int(tracks[0].offset) == 0 and not _is_padding(tracks[0])


def _speed_only_batch(cuts_tracks: _Tracks):
    """``(audios, factors)`` when every cut is one plain track with at most a ``Speed`` pending -- the mini-batch of ``features_of`` /
    ``audio_of`` --, else None."""
    audios, factors = [], []
    for tracks in cuts_tracks:
        if len(tracks) != 1:
            return None
        tr = tracks[0]  # (``_is_plain`` spelt out: one call less per cut)
        if tr.reverb is not None or tr.source_rate is not None or tr.levels is not None or int(tr.offset) != 0:
            return None
        a = tr.samples
        if not isinstance(a, torch.Tensor):
            if _is_padding(tr):
                return None
            a = torch.from_numpy(np.ascontiguousarray(a))
        audios.append(a)
        factors.append(float(tr.factor))
    return audios, factors


def _level_steps(arena, offs, lens, blocks, sr: int, tail: int):
    """Run one block per track (``blocks[i]`` = its steps or None) over the tracks at ``offs`` / ``lens``: step s of every track that has
    one, s = 0, 1, ... -- the level steps of a round in ONE ``level_in_arena`` call, in place; its rate steps (the oversampling around
    a ``Clipping``: sr -> k sr, k n samples, and back, n samples; the two halves of a band bracket, ``("rate", src, dst)``: the router
    sends their rate pairs to one bankless launch) in one ``resample_in_arena`` call that writes behind ``tail``.
    ``arena`` None: host arithmetic only.  -> (offsets, lengths, the first free float behind what was written, 16-byte aligned)."""
    from .augmentation import resample_layout

    offs, lens = np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)
    tail = (int(tail) + 3) & ~3
    for s in range(max((len(b) for b in blocks if b), default=0)):
        step = [b[s] if b and s < len(b) else None for b in blocks]
        idx = [i for i, st in enumerate(step) if st is not None and st[0] == "level"]
        if idx and arena is not None:
            _level_in_arena(arena, offs[idx], lens[idx], [step[i][1] for i in idx])
        ratios = [None if st is None or st[0] == "level" else (int(st[1]), int(st[2])) if st[0] == "rate" else
                  ((sr, sr * int(st[1])) if st[0] == "up" else (sr * int(st[1]), sr)) for st in step]
        if any(r is not None for r in ratios):
            if arena is None:
                offs, lens, tail = resample_layout(offs, lens, ratios, tail)
            else:
                end = resample_layout(offs, lens, ratios, tail)[2]
                offs, lens = _resample_in_arena(arena, offs, lens, ratios, tail)
                tail = end
    return offs, lens, tail


class _ArenaChain:
    """The augmentation chain of a mini-batch in ONE arena -- rate conversion -> speed -> level -> reverb -> level -> mix -- up to where its
    consumer takes over: ``(arena, cut_off, cut_len)``, the cuts' samples where the chain left them.  The feature launch
    (``FusedMiniBatch``) and the collate launch (``FusedAudioBatch``) both read from there.  A user says where to pack (``_chain_pack``)
    and which sampling rates it takes (``_chain_check_sr``)."""

    def _chain_pack(self, items, headroom: int = 0):
        raise NotImplementedError

    def _chain_check_sr(self, sr: int) -> None:
        pass

    def _tracks_chain(self, cuts_tracks, wants: List[int], sr: int, reverb_method: str = "direct"):
        """Pack every track (and every distinct RIR), resample the tracks with a pending factor into the tail, reverberate those with a RIR
        behind them, mix the mixed cuts behind that -> (arena, cut_off, cut_len).  (Runs under the caller's ``torch.no_grad()``.)
        ``reverb_method``: the route of the reverb (``reverb_in_arena``); this is the one place it is planned."""
        from .augmentation import mixed_num_samples, mixed_tail_floats, perturbed_layout, resample_layout, reverb_workspace_floats, scaled_rir
        from .extractors import _as_1d_float

        self._chain_check_sr(sr)
        cuts_tracks = _as_tracks(cuts_tracks, sr)
        items, factors, caps, ratios = [], [], [], []  # the tracks that have a source, in cut / track order; ratios: (source rate, sr) or None
        levels = []  # per such track: its two level blocks or None
        rirs, rir_of, rv_idx, rv_rir, rv_norm = [], {}, [], [], []  # distinct scaled RIRs (hs, shift); reverberated tracks -> their RIR
        for tracks in cuts_tracks:
            for tr in tracks:
                if _is_padding(tr):
                    if tr.reverb is not None:
                        raise ValueError("a padding track cannot carry a reverb")
                    continue
                a, rv = tr.samples, tr.reverb
                if rv is not None:
                    if id(rv[0]) not in rir_of:  # (the same array object, as the loader's RIR cache hands out: no look at its bytes)
                        h = np.ascontiguousarray(rv[0], dtype=np.float32).reshape(-1)
                        if h.size < 1:
                            raise ValueError("an impulse response needs at least one tap")
                        key = (h.size, h.tobytes())
                        if key not in rir_of:
                            rir_of[key] = len(rirs)
                            rirs.append(scaled_rir(h))
                        rir_of[id(rv[0])] = rir_of[key]
                    rv_idx.append(len(items)), rv_rir.append(rir_of[id(rv[0])]), rv_norm.append(int(bool(rv[1])))
                items.append(_as_1d_float(a.squeeze() if a.ndim > 1 else a, "HipOnTheFlyFeatures"))
                factors.append(float(tr.factor))
                levels.append(tr.levels)
                ratios.append(None if tr.source_rate is None else (int(tr.source_rate), int(sr)))
                caps.append(-1 if tr.cap is None else int(tr.cap))
        caps = np.asarray(caps, dtype=np.int64)
        num_tracks = len(items)
        rir_items = [hs for hs, _ in rirs]  # the RIRs travel in the same pack, behind the tracks
        if rir_items and all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in items):
            rir_items = [torch.from_numpy(h).to(items[0].device) for h in rir_items]  # (device-resident tracks are packed on the device)
        items += rir_items
        factors += [1.0] * len(rirs)
        ratios += [None] * len(rirs)
        two_pass = any(r is not None for r in ratios)
        has_level = any(lv is not None for lv in levels)
        blocks = [[None if lv is None else (lv[w] or None) for lv in levels] for w in (0, 1)]  # [in front of | behind the reverb][track]
        rv_idx = np.asarray(rv_idx, dtype=np.int64)
        cut_off, cut_len = np.zeros(len(cuts_tracks), dtype=np.int64), np.zeros(len(cuts_tracks), dtype=np.int64)

        def tables(po, pl):
            """The mix tables over the tracks at po / pl (a sample or two of a resampled track truncated); plain cuts -> cut_off / cut_len."""
            pl = np.asarray(pl)[: len(caps)]  # (the RIRs behind the tracks are not tracks)
            po, pl = np.asarray(po).tolist(), np.where(caps >= 0, np.minimum(pl, caps), pl).tolist()  # (plain ints: they are read one by one)
            first, so, sl, do, snrs, refs, cap, ids = [0], [], [], [], [], [], [], []
            k = 0
            for c, tracks in enumerate(cuts_tracks):
                if _is_plain(tracks):
                    cut_off[c], cut_len[c] = po[k], min(pl[k], int(wants[c]))
                    k += 1
                    continue
                ref = -1
                for t, tr in enumerate(tracks):
                    if _is_padding(tr):
                        so.append(-1), sl.append(int(tr.samples))
                    else:
                        so.append(po[k]), sl.append(pl[k])
                        k += 1
                    do.append(int(tr.offset)), snrs.append(tr.snr)
                    if tr.is_ref and ref < 0:
                        ref = t
                first.append(len(so)), refs.append(ref), cap.append(int(wants[c])), ids.append(c)
            return first, so, sl, do, snrs, refs, cap, ids

        # sizes first, from the lengths alone (the sample counts of the resampled tracks are known on the host, resample.py:309), so
        # that the tracks are packed straight into the ONE arena everything behind them is written to
        lens0 = np.array([int(x.shape[0]) for x in items], dtype=np.int64)
        rs_floats = 0  # the first pass (source rate -> sr), in front of the pass of the speed factors: both count for the head-room
        if two_pass:
            _, lens0, rs_floats = resample_layout(np.zeros(len(items), dtype=np.int64), lens0, ratios, 0)  # (a multiple of 4)
        _, ll, res_floats = perturbed_layout(np.zeros(len(items), dtype=np.int64), lens0, factors, sr, 0)  # (a multiple of 4)
        lv_floats = [0, 0]  # what the rate steps of the two level blocks write (a level step itself works in place)
        if has_level:  # (a band bracket may give back a sample more than it took: what follows a block counts with the block's lengths)
            ll = np.array(ll, dtype=np.int64)
            _, ll[:num_tracks], lv_floats[0] = _level_steps(None, np.zeros(num_tracks, dtype=np.int64), ll[:num_tracks], blocks[0], int(sr), 0)
        rv_floats = int(((ll[rv_idx] + 3) & ~3).sum())  # the reverb's outputs: as long as the (untruncated) tracks that reach it
        # ... and, on the FFT route, its spectra behind them (what the chain writes there later is stream-ordered behind the reverb)
        rv_ws_floats = reverb_workspace_floats(ll[rv_idx], [len(rirs[r][0]) for r in rv_rir], [rirs[r][1] for r in rv_rir], rv_rir, reverb_method)
        if has_level:
            _, ll[:num_tracks], lv_floats[1] = _level_steps(None, np.zeros(num_tracks, dtype=np.int64), ll[:num_tracks], blocks[1], int(sr), 0)
        first, _, sl, do, _, _, cap, mixed_ids = tables(np.zeros(len(items), dtype=np.int64), ll)
        if mixed_ids:
            short = mixed_num_samples(first, sl, do) < np.asarray(cap, dtype=np.int64)
            if short.any():
                raise ValueError(f"mixed cut {mixed_ids[int(np.nonzero(short)[0][0])]} is shorter than its wanted sample count: the reference "
                                 "reflect-pads such a mix (lhotse/cut/mixed.py:1386-1387); load it with cut.load_audio()")
        headroom = 3 + rs_floats + res_floats + rv_floats + rv_ws_floats + sum(lv_floats) + (mixed_tail_floats(first, sl, do, cap) if mixed_ids else 0)
        arena, offs, lens = self._chain_pack(items, headroom=headroom)
        front = int(offs[-1] + lens[-1])
        if two_pass:  # the tracks at another rate come to sr behind the pack; the speed pass reads them there
            offs, lens = _resample_in_arena(arena, offs, lens, ratios, front)
            front = ((front + 3) & ~3) + rs_floats  # (resample_layout's own end)
        if any(f != 1.0 for f in factors):
            po, pl = _perturb_in_arena(arena, offs, lens, factors, sr, front)
        else:
            po, pl = offs, lens
        mix_start = ((front + 3) & ~3) + res_floats  # behind the resampled tracks (perturbed_layout's own end)
        if has_level:  # the block in front of the reverb: on the whole resampled track, as the reference's transforms see it
            po, pl = np.array(po, dtype=np.int64), np.array(pl, dtype=np.int64)
            po[:num_tracks], pl[:num_tracks], end = _level_steps(arena, po[:num_tracks], pl[:num_tracks], blocks[0], int(sr), mix_start)
            assert end == mix_start + lv_floats[0]
            mix_start = end
        if len(rv_idx):
            # the reverb sees the whole resampled track and takes its powers over that length; the sample or two that
            # assert_and_maybe_fix_num_samples removes come off afterwards (recording.py:1032-1070): `tables` applies the caps
            ro = _reverb_in_arena(arena, po[rv_idx], pl[rv_idx], [int(po[num_tracks + r]) for r in rv_rir], [len(rirs[r][0]) for r in rv_rir],
                                  [rirs[r][1] for r in rv_rir], rv_norm, mix_start, *(() if reverb_method == "direct" else (reverb_method,)))
            po = np.array(po, dtype=np.int64)
            po[rv_idx] = ro
            mix_start += rv_floats
        if has_level:  # the block behind the reverb
            po[:num_tracks], pl[:num_tracks], end = _level_steps(arena, po[:num_tracks], pl[:num_tracks], blocks[1], int(sr), mix_start)
            assert end == mix_start + lv_floats[1]
            mix_start = end
        first, so, sl, do, snrs, refs, cap, mixed_ids = tables(po, pl)
        if not mixed_ids:  # (every cut turned out to be one plain track, e.g. a mixed cut whose other tracks are muted: nothing to mix)
            mo = ml = np.zeros(0, dtype=np.int64)
        else:
            mo, ml = _mix_in_arena(arena, first, so, sl, do, snrs, refs, cap, mix_start)
        cut_off[mixed_ids], cut_len[mixed_ids] = mo, ml
        return arena, cut_off, cut_len

    def _speed_arena(self, audios: List[torch.Tensor], factors: List[float], sr: int):
        """Pack the (partly unperturbed) batch into an arena with room for the resampled cuts behind it -> (arena, offsets, lengths, the
        first float behind the pack)."""
        from .augmentation import perturbed_tail_floats
        from .extractors import _as_1d_float

        self._chain_check_sr(sr)
        items = [_as_1d_float(a.squeeze() if a.ndim > 1 else a, "HipOnTheFlyFeatures") for a in audios]
        packed, offs, lens = self._chain_pack(items)
        front = int(packed.numel())
        arena = torch.empty(((front + 3) & ~3) + perturbed_tail_floats(lens, factors, sr), dtype=torch.float32, device=packed.device)
        arena[:front].copy_(packed, non_blocking=True)
        return arena, offs, lens, front


class FusedMiniBatch(_ArenaChain):
    """The device-facing half of ``HipOnTheFlyFeatures`` -- packing a (partly speed-perturbed) mini-batch into one arena, the launch pair
    of ``hipfeat_minibatch_*`` (or the per-factor route), the collated feature tensor -- WITHOUT any lhotse type in its interface:
    plain waveforms, factors and sample counts in, tensors out.  ``HipOnTheFlyFeatures`` inherits these methods unchanged; on a machine
    without lhotse (the GPU box of the test suite) the class is usable on its own, so that the GPU tests drive the product's code and not
    a restatement of it (tests/test_gpu_reference_drivers.py holds it to what lhotse's K2SpeechRecognitionDataset returned with the
    reference's CPU Speed + Fbank on the same files)."""

    audio_device: Union[str, torch.device, None] = "cpu"  # where `return_audio` hands the samples out ("cpu": per cut, as host tensors)

    def __init__(self, extractor, return_audio: bool = False, audio_device: Union[str, torch.device, None] = "cpu") -> None:
        if not hasattr(extractor, "extract_collated"):
            raise TypeError("FusedMiniBatch needs a Hip* extractor (with extract_collated)")
        self.extractor = extractor
        self.return_audio = return_audio
        self.audio_device = "cpu" if audio_device is not None and torch.device(audio_device).type == "cpu" else audio_device

    def _chain_pack(self, items, headroom: int = 0):
        return self.extractor._pack(items, headroom=headroom)

    def _chain_check_sr(self, sr: int) -> None:
        self.extractor._check_sr(sr)

    def features_of(self, audios: List[torch.Tensor], factors: List[float], wants: List[int], sampling_rate: int):
        """What ``HipOnTheFlyFeatures.__call__`` does between reading the audio and returning: ``audios`` as read from the files (the
        segments in front of a pending ``Speed``), ``factors`` still to be applied (1.0 = none), ``wants`` = samples each cut must end up
        with (``compute_num_samples(cut.duration)``) -> ``(feats (B, Tmax, F) on the extractor's device, feat_lens)``."""
        if any(f != 1.0 for f in factors):
            return self._perturb_and_extract(audios, factors, wants, sampling_rate)[:2]
        return self.extractor.extract_collated(audios, sampling_rate=sampling_rate, padding_value=LOG_EPSILON)

    def features_of_tracks(self, cuts_tracks, wants: List[int], sampling_rate: int, reverb_method: str = "direct"):
        """``features_of`` for a mini-batch in which some cuts are ``MixedCut``s (``CutMix``, ``CutSet.mix`` / ``.pad``), without a lhotse
        type: every cut is a list of tracks, each a ``Track`` or a plain tuple of its first 5 to 9 values (normalised once, on entry)
        ``(samples, factor, offset_samples, snr, is_reference[, num_samples])`` -- ``samples`` as read
        from the file (in front of a pending ``Speed(factor)``; 1.0 = none) or, for a ``PaddingCut`` track, its sample COUNT as an int;
        the track's first sample inside the cut; its SNR in dB or None; whether it is the cut's SNR reference track
        (``_get_snr_reference_track``, lhotse/cut/mixed.py:1909-1918); optionally the samples the track must end up with after its
        ``Speed`` (a sample or two are truncated, recording.py:1058-1060).  ``wants[c]`` = samples cut ``c`` must end up with
        (``cut.num_samples``).  A cut of one unscaled track at offset 0 is a plain cut and is not copied.  An optional 7th element
        ``(rir_samples, normalize_output)`` reverberates the track (``ReverbWithImpulseResponse`` with a recorded RIR behind the track's
        ``Speed``, lhotse/augmentation/rir.py:78-153): ``rir_samples`` = the float32 RIR as the reference loads it (channel selected,
        ``early_only`` applied).  The RIRs of the mini-batch are packed into the arena with the tracks, each distinct one once, scaled by
        2^-15 on the host; the reverb sees the untruncated resampled track, the mix and the plain cuts read its output.  An optional 8th
        element ``source_rate``: the samples are at that rate (a pending ``Resample(source_rate -> sampling_rate)`` in front of the
        ``Speed``, lhotse/augmentation/torchaudio.py:86-139 with the sinc backend) and are resampled to ``sampling_rate`` first, one launch
        per distinct rate (``lhotse_amd.augmentation.resample_in_arena``); the track's ``Speed`` then is a second pass over the first
        pass's output, and only the final length is capped (recording.py:486-490).  A mini-batch without a ``source_rate`` takes exactly
        the route it took before there was one.  An optional 9th element ``(block in front of the reverb, block behind it)`` changes
        the track's level (``Volume`` / ``Clipping``, ``lhotse_amd.augmentation.level_in_arena``): a block is None or a list of steps
        ``("level", [("volume", factor) | ("clip", hard, gain_db, normalize), ...])``, ``("up", k)``, ``("down", k)`` -- the last two are
        the ``Resample(sr -> k sr)`` / ``Resample(k sr -> sr)`` that ``clip_amplitude(oversampling=k)`` puts around its ``Clipping`` --,
        ``("rate", src, dst)`` -- one ``Resample(src -> dst)`` between any two rates that ``resample_in_arena`` routes; the band bracket
        of ``LowpassUsingResampling`` is ``("rate", sr, m)``, ``("rate", m, sr)`` --; the
        blocks run behind the ``Speed`` on the untruncated track, the first in front of the reverb, the second behind it.  Absent or
        None: exactly the route of before.

        Route of a mini-batch with mixed cuts: pack all tracks -> resample launch per pending factor -> convolution and gain launch of
        the reverberated tracks (``lhotse_amd.augmentation.reverb_in_arena``) -> energy launch -> mix launch
        (``lhotse_amd.augmentation.mix_in_arena``) -> the feature launch over the mixed offsets / lengths; one arena, one stream, no
        device -> host copy in between.  Without a mixed cut this IS ``features_of``.
        -> ``(feats (B, Tmax, F), feat_lens, audio)``, ``audio`` = the cuts' samples (host tensors) with ``return_audio``, else None.  With
        ``return_audio`` and an ``audio_device`` other than ``"cpu"`` (None: the extractor's device): ``(feats, feat_lens, audio (B, Tmax),
        audio_lens)``, the samples collated on the device out of the arena the feature launch read, with no per-cut copy.
        ``reverb_method``: ``"direct"`` (default), ``"fft"`` or ``"auto"``, the route of the reverberated tracks' convolution
        (``reverb_in_arena``); the arena then also has room for the spectra."""
        _checked_reverb_method(reverb_method)
        if len(cuts_tracks) != len(wants):
            raise ValueError("features_of_tracks: one wanted sample count per cut")
        cuts_tracks = _as_tracks(cuts_tracks, sampling_rate)
        speed_only = _speed_only_batch(cuts_tracks)
        if speed_only is not None:
            audios, factors = speed_only
            if any(f != 1.0 for f in factors):
                return self._perturb_and_extract(audios, factors, wants, sampling_rate)
            return self._plain_extract(audios, sampling_rate)
        return self._mix_and_extract(cuts_tracks, wants, sampling_rate, reverb_method)

    def _mix_and_extract(self, cuts_tracks, wants: List[int], sr: int, reverb_method: str = "direct"):
        """The chain (``_tracks_chain``), then the feature launch over the cuts where it left them."""
        ex = self.extractor
        with torch.no_grad():
            arena, cut_off, cut_len = self._tracks_chain(cuts_tracks, wants, sr, reverb_method)
            zero_pad = getattr(ex.config, "edge_rule", "reflect") == "batch_zero_pad"  # as extract_collated
            padded = np.full(len(cut_len), int(cut_len.max()), dtype=np.int64) if zero_pad else None
            feats, frames = ex.plan.run_collated(arena, cut_off, cut_len, padded, float(LOG_EPSILON))
        return (feats, torch.from_numpy(np.asarray(frames, dtype=np.int64))) + self._audio_of_arena(arena, cut_off, cut_len)

    def _speed_bank(self, factors, sr: int, device):
        """The bank of the factors met so far on this device (rebuilt when a new factor shows up); None if one of them is not among
        the mixed launch's ratios."""
        from ._lib import ERR_UNSUPPORTED, HipFeatError
        from .augmentation import HipSpeedBank

        need = {float(f) for f in factors if float(f) != 1.0}
        cache = self.__dict__.setdefault("_banks", {})
        key = (int(sr), str(device))
        refused = cache.setdefault("refused", set())
        if need & refused:
            return None
        bank = cache.get(key)
        if bank is None or not need <= set(bank.factors):
            have = set() if bank is None else set(bank.factors)
            # only the factors whose resampling ratio round(sr * f) : sr reduces to one of the mixed launch's compile-time ratios can be
            # served by a bank; every other factor is refused ON ITS OWN (a mini-batch with {0.9, 0.95} used to blacklist 0.9
            # as well, and every later 0.9 / 1.1 mini-batch silently fell back to the three-launch route)
            bad = {f for f in need - have if not _bank_ratio_ok(sr, f)}
            if bad:
                refused |= bad
                return None
            try:
                bank = cache[key] = HipSpeedBank(sorted(have | need), sr, device)
            except HipFeatError as e:
                if e.status != ERR_UNSUPPORTED:
                    raise
                return None  # (this mini-batch goes per factor; nothing is blacklisted on a guess)
        return bank

    def _perturb_and_extract(self, audios: List[torch.Tensor], factors: List[float], wants: List[int], sr: int):
        """Pack the (partly unperturbed) batch, resample the cuts with a pending factor into the tail of the same buffer, extract."""
        ex = self.extractor
        with torch.no_grad():
            arena, offs, lens, front = self._speed_arena(audios, factors, sr)
            zero_pad = getattr(ex.config, "edge_rule", "reflect") == "batch_zero_pad"  # as extract_collated
            want = np.ascontiguousarray(wants, dtype=np.int64)
            bank = self._speed_bank(factors, sr, arena.device) if hasattr(ex.plan, "handle") else None
            if bank is not None:  # ONE launch for all factors + the padding rows, then the feature launch (hipfeat_minibatch_*)
                feats, frames, po, pl = bank.extract_collated(ex.plan, arena, np.ascontiguousarray(offs, dtype=np.int64),
                                                              np.ascontiguousarray(lens, dtype=np.int64), bank.index_of(factors), front,
                                                              float(LOG_EPSILON), max_samples=want, zero_pad_batch=zero_pad)
            else:  # factors outside the mixed launch's compile-time ratios: one resample launch per factor
                po, pl = _perturb_in_arena(arena, offs, lens, factors, sr, front)
                pl = np.minimum(pl, want)  # a sample or two to truncate (recording.py:1058-1060)
                padded = np.full(len(pl), int(pl.max()), dtype=np.int64) if zero_pad else None
                feats, frames = ex.plan.run_collated(arena, po, pl, padded, float(LOG_EPSILON))
        return (feats, torch.from_numpy(np.asarray(frames, dtype=np.int64))) + self._audio_of_arena(arena, po, pl)

    def _plain_extract(self, audios, sr: int):
        """A mini-batch with nothing pending: ``extract_collated``; with ``return_audio`` on a device, the same pack and the same launch
        with the arena kept for the collate launch."""
        ex = self.extractor
        if not (self.return_audio and self.audio_device != "cpu"):
            feats, feat_lens = ex.extract_collated(audios, sampling_rate=sr, padding_value=LOG_EPSILON)
            return (feats, feat_lens, ([a.reshape(-1) for a in audios] if self.return_audio else None))
        from . import _lib
        from .extractors import _as_1d_float

        ex._check_sr(sr)
        items = [_as_1d_float(a.squeeze() if a.ndim > 1 else a, "extract_collated()") for a in audios]
        if not items:
            raise ValueError("extract_collated(): empty batch")
        zero_pad = getattr(ex.config, "edge_rule", "reflect") == "batch_zero_pad"
        with torch.no_grad():
            arena, offs, lens = ex._pack(items)
            padded = np.full(len(items), int(lens.max()), dtype=np.int64) if zero_pad else None
            try:
                feats, frames = ex.plan.run_collated(arena, offs, lens, padded, float(LOG_EPSILON))
            except _lib.HipFeatError as e:
                if e.status == _lib.ERR_TOO_SHORT:
                    raise ValueError(str(e)) from e
                raise
        return (feats, torch.from_numpy(frames)) + self._audio_of_arena(arena, offs, lens)

    def _audio_of_arena(self, arena, cut_off, cut_len) -> tuple:
        """The ``return_audio`` results of a mini-batch whose cuts lie at cut_off / cut_len of the arena the feature launch read:
        ``(None,)`` without ``return_audio``; ``audio_device="cpu"``: ``(the cuts' samples as host tensors,)``, one blocking copy per cut;
        a device or None (the arena's): ``(the dense zero-padded (B, Tmax) tensor there, the lengths)``, one collate launch."""
        if not self.return_audio:
            return (None,)
        if self.audio_device == "cpu":
            return ([arena[int(o) : int(o) + int(n)].cpu() for o, n in zip(cut_off, cut_len)],)
        lens = np.asarray(cut_len, dtype=np.int64)
        audio = _collate_in_arena(arena, cut_off, lens, int(lens.max()) if len(lens) else 0, torch.float32)
        return (audio if self.audio_device is None else audio.to(self.audio_device), torch.from_numpy(lens.copy()))


class FusedAudioBatch(_ArenaChain):
    """``FusedMiniBatch`` for a consumer of samples (``AudioSamples``: wav2vec 2.0 / HuBERT-style encoders, Whisper fine-tuning with the model's
    own front end, codec models): the same packing and the same chain in the arena, then ONE collate launch
    (``lhotse_amd.augmentation.collate_in_arena``) instead of the feature launch.  No lhotse type in its interface, and no extractor: the
    chain needs a device to pack into, nothing else.  ``dtype``: float32, float16 or bfloat16 samples."""

    def __init__(self, device: Union[str, torch.device, None] = None, dtype: torch.dtype = torch.float32) -> None:
        dev = torch.device("cuda" if device is None else device)
        if dev.type == "cuda" and dev.index is None and torch.cuda.is_available():
            dev = torch.device("cuda", torch.cuda.current_device())
        if dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"FusedAudioBatch: float32, float16 or bfloat16 samples, got {dtype}")
        self.device, self.dtype = dev, dtype

    def _chain_pack(self, items, headroom: int = 0):
        from .extractors import pack_items

        if any(x.dtype not in (torch.float32, np.float32) for x in items):
            raise TypeError("FusedAudioBatch: expected float32 samples")
        return pack_items(items, self.device, None, headroom)

    def _collated(self, arena, cut_off, cut_len, wants):
        lens = np.minimum(np.asarray(cut_len, dtype=np.int64), np.asarray(wants, dtype=np.int64))
        audio = _collate_in_arena(arena, cut_off, lens, int(max(wants)) if len(lens) else 0, self.dtype)
        return audio, torch.from_numpy(lens.copy())

    def audio_of(self, audios: List[torch.Tensor], factors: List[float], wants: List[int], sampling_rate: int):
        """The arguments of ``FusedMiniBatch.features_of`` -> ``(audio (B, Tmax) on the device, audio_lens)``, ``Tmax = max(wants)``,
        zeros behind every cut.  A mini-batch with nothing pending is packed and collated with nothing in between."""
        from .extractors import _as_1d_float

        if len(audios) != len(wants) or len(audios) != len(factors):
            raise ValueError("audio_of: one factor and one wanted sample count per cut")
        with torch.no_grad():
            if any(f != 1.0 for f in factors):
                arena, offs, lens, front = self._speed_arena(audios, factors, sampling_rate)
                po, pl = _perturb_in_arena(arena, offs, lens, factors, sampling_rate, front)
            else:
                arena, po, pl = self._chain_pack([_as_1d_float(a.squeeze() if a.ndim > 1 else a, "FusedAudioBatch") for a in audios])
            return self._collated(arena, po, pl, wants)

    def audio_of_tracks(self, cuts_tracks, wants: List[int], sampling_rate: int, reverb_method: str = "direct"):
        """The arguments of ``FusedMiniBatch.features_of_tracks`` (tracks with their pending speed, reverb, source rate and level blocks,
        and the reverb's route) -> ``(audio (B, Tmax) on the device, audio_lens)``: the same chain in the same arena, then the collate
        launch."""
        _checked_reverb_method(reverb_method)
        if len(cuts_tracks) != len(wants):
            raise ValueError("audio_of_tracks: one wanted sample count per cut")
        cuts_tracks = _as_tracks(cuts_tracks, sampling_rate)
        speed_only = _speed_only_batch(cuts_tracks)
        if speed_only is not None:
            return self.audio_of(*speed_only, wants, sampling_rate)
        with torch.no_grad():
            arena, cut_off, cut_len = self._tracks_chain(cuts_tracks, wants, sampling_rate, reverb_method)
            return self._collated(arena, cut_off, cut_len, wants)

    def audio_of_channels(self, cuts_channels, factors: List[float], source_rates, wants: List[int], sampling_rate: int,
                          mono_downmix: Optional[bool] = None, offsets=None, totals=None):
        """Multi-channel cuts (``collate_audio(..., mono_downmix=...)``, lhotse/dataset/collation.py:215-241).  ``cuts_channels[i]``: the
        channel rows of cut ``i`` -- 1-D float32, of equal length, read in front of the cut's pending transforms: ``factors[i]`` (a
        ``Speed``, 1.0 = none) behind ``source_rates[i]`` (a ``Resample`` from that rate to ``sampling_rate``, None = none).  Every channel
        row goes into the arena as a row of its own and runs through the chain of ``audio_of_tracks`` like a mono cut with that factor
        and rate; then ONE collate launch (``lhotse_amd.augmentation.collate_sources_in_arena``) writes the batch:

        ``mono_downmix=True`` -> ``(B, Tmax)``: a cut's row is the mean over its channels (float64 sum in channel order, one division, one
        rounding; a cut of one channel is copied).  ``False`` -> ``(B, Cmax, Tmax)``, written as ``B * Cmax`` rows of the same launch: the
        channels a cut does not have are zero rows, a mono cut sits in channel 0.  ``None``: the reference's rule -- downmix unless every
        cut has more than one channel.  -> ``(audio, audio_lens)`` with ``wants`` truncating as in ``audio_of``.

        An entry of ``cuts_channels`` may instead be the TRACK LIST of a mono cut as ``audio_of_tracks`` takes it (a list of tuples; its
        factor and source rate are the tracks' own): that cut keeps its whole chain -- mix, reverb, level -- in the same arena and counts
        as a cut of one channel.  ``offsets[i]`` / ``totals[i]`` (None: 0 / the cut's own length): a cut padded with silence -- its
        samples start at element ``offsets[i]`` of its row(s) and its reported length is ``totals[i]``."""
        B = len(cuts_channels)
        if B == 0 or not (B == len(factors) == len(source_rates) == len(wants)):
            raise ValueError("audio_of_channels: at least one cut, and one factor, one source rate and one wanted sample count per cut")
        pseudo, pseudo_wants, first = [], [], [0]  # every channel row as a cut of one plain track; the rows of cut i are first[i] : first[i + 1]
        for chans, f, rate, want in zip(cuts_channels, factors, source_rates, wants):
            if len(chans) and isinstance(chans[0], tuple):  # the tracks of a mono cut
                pseudo.append(list(chans)), pseudo_wants.append(int(want))
            else:
                if not len(chans):
                    raise ValueError("audio_of_channels: a cut without channels")
                if len({int(x.shape[-1]) for x in chans}) != 1 or any(x.ndim != 1 for x in chans):
                    raise ValueError("audio_of_channels: the channel rows of a cut are 1-D and equally long")
                for x in chans:
                    pseudo.append([Track(x, float(f), 0, None, True, int(want), source_rate=rate)])
                    pseudo_wants.append(int(want))
            first.append(len(pseudo))
        first = np.asarray(first, dtype=np.int64)
        num_ch = np.diff(first)
        if int(num_ch.max()) > 32:
            raise ValueError(f"audio_of_channels: a cut of {int(num_ch.max())} channels, the collate launch takes at most 32 sources per row")
        if mono_downmix is None:
            mono_downmix = not bool((num_ch > 1).all())
        with torch.no_grad():
            arena, row_off, row_len = self._tracks_chain(pseudo, pseudo_wants, sampling_rate)
            lens = np.minimum(row_len[first[:-1]], np.asarray(wants, dtype=np.int64))
            dst = np.zeros(B, dtype=np.int64) if offsets is None else np.asarray([0 if o is None else int(o) for o in offsets], dtype=np.int64)
            out_lens = lens.copy() if totals is None else np.asarray([int(n) if t is None else int(t) for n, t in zip(lens, totals)], dtype=np.int64)
            if int((dst + lens - out_lens).max()) > 0:
                raise ValueError("audio_of_channels: a cut's samples reach past its total length")
            tmax = max(int(w) if totals is None or totals[i] is None else int(totals[i]) for i, w in enumerate(wants))
            if mono_downmix:
                audio = _collate_sources_in_arena(arena, first, row_off, lens, tmax, dst, self.dtype)
            else:
                cmax = int(num_ch.max())
                k = (np.arange(cmax)[None, :] < num_ch[:, None]).astype(np.int64).reshape(-1)  # row (b, c) has one source, or none
                srcs = np.concatenate([row_off[first[b] : first[b + 1]] for b in range(B)])
                audio = _collate_sources_in_arena(arena, np.concatenate([[0], np.cumsum(k)]), srcs, np.repeat(lens, cmax), tmax,
                                                  np.repeat(dst, cmax), self.dtype).view(B, cmax, tmax)
            return audio, torch.from_numpy(out_lens)



def _featmix_in_arena(arena_bytes, cuts_table, num_features, row_frames, layout=None):
    from . import augmentation as A

    return A.featmix_in_arena(arena_bytes, cuts_table, num_features, row_frames, layout=layout)


class FusedFeatureBatch:
    """The mini-batch of the PRECOMPUTED-features recipe on the device: the stored tracks of every cut go into ONE byte arena as they
    were stored (binary16 stays binary16: half the bytes over PCIe), and the two launches of ``lhotse_amd.augmentation.featmix_in_arena``
    write the padded ``(B, T, F)`` float32 batch -- copies for plain and right-padded cuts, the ``FeatureMixer`` fold (``CutMix``, left /
    both-sided padding) for the rest.  No lhotse type in its interface.

    A CUT is a dict ``{"form": FEATMIX_COPY | FEATMIX_FOLD, "num_frames", "pad_value", "ref_track", "tracks"}`` (``"dst_first"``
    optional), a TRACK a dict ``{"frames", "first", "snr", "value"}`` plus its source: ``"array"`` (a loaded ``(rows, F)`` float32 or
    float16 matrix), or ``"read"`` with ``"rows"`` and ``"f16"`` (``read(out)`` fills the C-contiguous uint8 view ``out`` of ``rows * F *
    itemsize`` bytes, e.g. ``reader.read_raw(key, lo, hi, out=out)``), or neither: a constant track of ``value``."""

    _ALIGN = 16  # every track starts on a 16-byte boundary of the arena

    def __init__(self, device: Union[str, torch.device, None] = None) -> None:
        dev = torch.device("cuda" if device is None else device)
        if dev.type == "cuda" and dev.index is None and torch.cuda.is_available():
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self._staging: Optional[torch.Tensor] = None  # page-locked where a GPU is there
        self._uploaded = None  # the event behind the upload that read the staging buffer last

    def _stage(self, nbytes: int) -> torch.Tensor:
        if self._uploaded is not None:  # the previous batch's upload has read the buffer
            self._uploaded.synchronize()
            self._uploaded = None
        if self._staging is None or self._staging.numel() < nbytes:
            pin = self.device.type == "cuda" and torch.cuda.is_available()
            self._staging = torch.empty(max(2 * nbytes, 1 << 16), dtype=torch.uint8, pin_memory=pin)
        return self._staging

    def features_of(self, cuts: List[dict], num_features: int, row_frames: Optional[int] = None, pool=None):
        """-> ``(features (B, row_frames, F) float32 on the device, features_lens int32)``; ``row_frames=None``: the longest cut.
        ``pool``: a thread pool for the reads."""
        from .augmentation import FeatCut, FeatTrack

        F = int(num_features)
        table, jobs, pos = [], [], 0
        for c in cuts:
            tracks = []
            for t in c["tracks"]:
                arr, read = t.get("array"), t.get("read")
                if arr is None and read is None:
                    tracks.append(FeatTrack(-1, int(t["frames"]), None, False, int(t.get("first", 0)), t.get("snr"), float(t.get("value", 0.0))))
                    continue
                if arr is not None:
                    arr = np.ascontiguousarray(arr)
                    if arr.ndim != 2 or arr.shape[1] != F or arr.dtype not in (np.float32, np.float16):
                        raise ValueError(f"FusedFeatureBatch: a track is a (rows, {F}) float32 or float16 matrix, got {arr.dtype} {arr.shape}")
                    rows, f16 = arr.shape[0], arr.dtype == np.float16
                else:
                    rows, f16 = int(t["rows"]), bool(t["f16"])
                nbytes = rows * F * (2 if f16 else 4)
                jobs.append((pos, nbytes, arr, read))
                tracks.append(FeatTrack(pos, int(t["frames"]), rows, f16, int(t.get("first", 0)), t.get("snr"), 0.0))
                pos += -(-nbytes // self._ALIGN) * self._ALIGN
            table.append(FeatCut(tracks, int(c["num_frames"]), int(c["form"]), float(c.get("pad_value", 0.0)), int(c.get("dst_first", 0)),
                                 int(c.get("ref_track", -1))))
        from .augmentation import featmix_layout

        layout = featmix_layout(max(pos, 1), table, F, row_frames)  # (ValueError before anything is read; the launches take it as it is)
        total = max(pos, self._ALIGN)
        host = self._stage(total).numpy()

        def fill(job):
            at, nbytes, arr, read = job
            out = host[at: at + nbytes]
            if arr is not None:
                out[:] = arr.reshape(-1).view(np.uint8)
            elif nbytes:
                read(out)

        if pool is not None and len(jobs) > 1:
            list(pool.map(fill, jobs))
        else:
            for j in jobs:
                fill(j)
        with torch.no_grad():
            arena = torch.empty(total, dtype=torch.uint8, device=self.device)
            arena.copy_(self._staging[:total], non_blocking=True)
            if self.device.type == "cuda":
                self._uploaded = torch.cuda.Event()
                self._uploaded.record()
            feats, lens = _featmix_in_arena(arena, table, F, row_frames, layout)
        return feats, torch.from_numpy(np.asarray(lens, dtype=np.int32).copy())


if HAVE_LHOTSE:  # pragma: no cover - authoring container only
    from concurrent.futures import ThreadPoolExecutor

    from lhotse.audio.utils import suppress_audio_loading_errors  # type: ignore
    from lhotse.dataset.collation import collate_vectors, read_audio_from_cuts  # type: ignore
    from lhotse.dataset.input_strategies import AudioSamples, OnTheFlyFeatures, PrecomputedFeatures, _get_executor  # type: ignore
    from lhotse.utils import compute_num_samples  # type: ignore

    def _transform_name(t) -> str:
        return t.get("name") if isinstance(t, dict) else type(t).__name__

    def _kwargs_of(t, names) -> dict:
        return {k: t["kwargs"][k] for k in names if k in t["kwargs"]} if isinstance(t, dict) else {k: getattr(t, k) for k in names}

    def _resample_rates(t) -> Tuple[int, int]:
        kw = _kwargs_of(t, ("source_sampling_rate", "target_sampling_rate"))
        return int(kw["source_sampling_rate"]), int(kw["target_sampling_rate"])

    from .augmentation import MAX_RESAMPLE_BANK_FLOATS, _sinc_bank_floats, resample_route  # noqa: F401  (one rule for both sides)

    MAX_CHANNELS = 32  # channels of one cut = sources of one row of the collate launch (COLLATE_MAX_SOURCES)
    MAX_LEVEL_OPS = 4  # ops of one block = of one program of hipfeat_level_plan

    def _reference_resamples_with_sinc() -> bool:
        """Whether lhotse's ``Resample.__call__`` would run ``ResampleTensor`` (the sinc resampler the device implements): torchaudio
        importable and the resampling backend ``default`` (lhotse/augmentation/torchaudio.py:108-139)."""
        import lhotse.augmentation.torchaudio as ref  # (looked up on the module: the very name Resample.__call__ consults)
        from lhotse.audio.resampling_backend import get_current_resampling_backend

        return bool(ref.is_torchaudio_available()) and get_current_resampling_backend() == "default"

    def _level_block(tf: list, pos: int, sr: int):
        """The run of level elements of ``tf`` from ``pos`` on -- ``Volume`` | ``Clipping`` | ``Resample(sr -> k sr) Clipping
        Resample(k sr -> sr)`` | the band bracket ``Resample(sr -> m) Resample(m -> sr)``, which counts as two ops -- as steps -> (steps or
        None when there is none, the position behind it); ``False`` in place of the steps: the run is not served (more than 4 ops, two
        ``Clipping``s, k outside 2 ... 8 or not an integer, a ``Resample`` that is not such a bracket, a band bracket whose rates no
        route serves: ``resample_route``)."""
        steps, ops, clips = [], 0, 0

        def level(op):
            if steps and steps[-1][0] == "level":
                steps[-1][1].append(op)
            else:
                steps.append(("level", [op]))

        def clip_op(t):
            kw = {"hard": False, "gain_db": 0.0, "normalize": True, **_kwargs_of(t, ("hard", "gain_db", "normalize"))}
            return ("clip", bool(kw["hard"]), float(kw["gain_db"]), bool(kw["normalize"]))

        while pos < len(tf):
            name = _transform_name(tf[pos])
            if name == "Volume":
                level(("volume", float(_kwargs_of(tf[pos], ("factor",))["factor"])))
                pos += 1
            elif name == "Clipping":
                level(clip_op(tf[pos]))
                clips, pos = clips + 1, pos + 1
            elif name == "Resample" and _resample_rates(tf[pos])[0] == sr and pos + 1 < len(tf) and _transform_name(tf[pos + 1]) == "Resample":
                # the band bracket B = Resample(sr -> m) Resample(m -> sr) of LowpassUsingResampling (cut_transforms/lowpass.py): two ops
                m = _resample_rates(tf[pos])[1]
                if _resample_rates(tf[pos + 1]) != (m, sr) or m == sr or resample_route(sr, m) is None or resample_route(m, sr) is None:
                    return False, pos  # (among them a window beyond the bankless kernel's cap: 48 kHz -> under 6.2 kHz)
                steps += [("rate", sr, m), ("rate", m, sr)]
                pos, ops = pos + 2, ops + 1  # (and the common count below: a bracket is two of a block's four ops)
            elif name == "Resample" and _resample_rates(tf[pos])[0] == sr:  # the opening of clip_amplitude(oversampling=k) (recording.py:959-973)
                up = _resample_rates(tf[pos])[1]
                if pos + 2 >= len(tf) or _transform_name(tf[pos + 1]) != "Clipping" or _transform_name(tf[pos + 2]) != "Resample":
                    return False, pos
                if _resample_rates(tf[pos + 2]) != (up, sr) or up % sr or not 2 <= up // sr <= 8:
                    return False, pos
                steps += [("up", up // sr), ("level", [clip_op(tf[pos + 1])]), ("down", up // sr)]
                clips, pos = clips + 1, pos + 3
            else:
                break
            ops += 1
            if ops > MAX_LEVEL_OPS or clips > 1:
                return False, pos
        return (steps or None), pos

    def _parse_transforms(tf, sr: int, gpu_speed: bool, gpu_reverb: bool, gpu_resample: bool, gpu_level: bool, bankless: bool) -> Optional[Chain]:
        """ONE walk over a recording's transform list, left to right, for ``parse_chain`` (a mono cut) and ``pending_channel_chain`` (a
        ``MultiCut``: ``gpu_reverb`` and ``gpu_level`` off).  An element whose switch is off is not taken, and whatever is left over at the
        end refuses the list."""
        tf, pos = list(tf or []), 0
        src, factor, pre, reverb, post = None, 1.0, None, None, None
        if tf and _transform_name(tf[0]) == "Resample" and _resample_rates(tf[0])[0] != sr:  # cuts.resample(sr); one FROM sr opens a bracket
            src, dst = _resample_rates(tf[0])
            if not gpu_resample or dst != sr or src <= 0:
                return None
            from lhotse.audio.resampling_backend import get_current_resampling_backend  # the reference's own switch is the contract

            if get_current_resampling_backend() != "default":
                return None
            if resample_route(src, dst) is None if bankless else _sinc_bank_floats(src, dst) > MAX_RESAMPLE_BANK_FLOATS:
                return None
            pos = 1
        if pos < len(tf) and _transform_name(tf[pos]) == "Speed":
            factor = float(_kwargs_of(tf[pos], ("factor",))["factor"])
            if factor != 1.0 and not gpu_speed:
                return None
            pos += 1
        if gpu_level:
            pre, pos = _level_block(tf, pos, sr)
            if pre is False:
                return None
        if gpu_reverb and pos < len(tf) and _transform_name(tf[pos]) == "ReverbWithImpulseResponse":
            kw = _kwargs_of(tf[pos], ("rir", "normalize_output", "early_only", "rir_channels"))
            if kw.get("rir") is None or len(kw.get("rir_channels") or [0]) != 1:
                return None
            reverb = {"rir": kw["rir"], "normalize_output": bool(kw.get("normalize_output", True)), "early_only": bool(kw.get("early_only", False)),
                      "rir_channels": [int(c) for c in (kw.get("rir_channels") or [0])]}
            pos += 1
        if gpu_level:
            post, pos = _level_block(tf, pos, sr)
            if post is False:
                return None
        if pos != len(tf):
            return None
        if any(st[0] != "level" for st in (pre or []) + (post or [])) and not (gpu_resample and _reference_resamples_with_sinc()):
            return None  # (a bracket runs the device's sinc resampler: only where the reference's Resample runs its own)
        return Chain(src, factor, pre, reverb, post)

    def parse_chain(cut, gpu_speed: bool = True, gpu_reverb: bool = True, gpu_resample: bool = True, gpu_level: bool = True,
                    bankless: bool = False) -> Optional[Chain]:
        """THE rule of what the device takes over: a mono cut (no video) over a recording whose transform list is

            [Resample(a -> sr)]? [Speed]? L? [ReverbWithImpulseResponse]? L?
            L = ( Volume | Clipping | Resample(sr -> k sr) Clipping Resample(k sr -> sr) | B ){1 ... 4 ops, at most one Clipping}
            B = Resample(sr -> m) Resample(m -> sr), m != sr: the band bracket of LowpassUsingResampling (m = 2 x cutoff); two ops

        -> its ``Chain``; an empty list gives ``Chain()``, with nothing ``pending``.  None = load it the reference's way.  Every element
        has its switch and its conditions:

        * the leading ``Resample`` (``cuts.resample(sr)``): ``gpu_resample``; ``sr == cut.sampling_rate``, ``a != sr``; the reference's
          ``default`` resampling backend (``sox``: another filter); a reduced filter bank of at most 2^20 floats -- or, with ``bankless``
          as the strategies set it, any pair of rates that ``resample_in_arena`` routes (``resample_route``: 11127 -> 16000 goes to the
          kernel without a bank);
        * the ``Speed``: ``gpu_speed`` unless its factor is 1;
        * the reverb: ``gpu_reverb``; a recorded ``rir`` (not the random generator) and exactly one entry in ``rir_channels``;
        * the level blocks: ``gpu_level`` and a recording of ONE channel (a ``MonoCut`` that selects one channel of several is left to the
          reference); k an integer 2 ... 8 (what ``clip_amplitude(oversampling=k)`` appends, recording.py:937-975); the rate steps of either
          bracket need ``gpu_resample``, a route for each pair of rates and a reference that resamples with its sinc module
          (``_reference_resamples_with_sinc``).

        Refused with it: anything but a ``MonoCut`` (a ``MultiCut``: ``pending_channel_chain``; a ``MixedCut``: ``deferred_mix``), any other
        transform, any other order (a ``Resample`` that is not first, a level op in front of the ``Speed``, a reverb in front of a
        ``Speed``, two reverbs), a block of more than 4 ops or with two ``Clipping``s."""
        if type(cut).__name__ != "MonoCut" or not cut.has_recording or getattr(cut.recording, "has_video", False):
            return None
        return _parse_transforms(cut.recording.transforms, int(cut.sampling_rate), gpu_speed, gpu_reverb, gpu_resample,
                                 gpu_level and cut.recording.num_channels == 1, bankless)

    def pending_channel_chain(cut, gpu_speed: bool = True, gpu_resample: bool = True):
        """``parse_chain`` for a cut of SEVERAL channels: a ``MultiCut`` (no video, 1 ... 32 channels) over a recording whose transform
        list is ``[Resample(a -> sr)]? [Speed]?`` -- the same walk with ``bankless``, without a reverb and level blocks -- or a ``MixedCut``
        (no transforms of its own, no video) whose audible tracks are ONE such ``MultiCut`` and ``PaddingCut``s, none with an SNR
        (``cut.pad``, to the right or to the left) -> ``(the MultiCut, a or None, factor still to be applied (1.0 = none), the samples of
        padding in front of it, the cut's own num_samples or None when it is not padded)``.  None = load it the reference's way: any other
        transform (``Volume``, ``Clipping``, a reverb, a ``Resample`` that is not first or a bracket of two), more than 32 channels, a
        multi-channel track that is mixed with audio, a padded cut whose tracks do not add up to its length (deferred_mix's rule)."""
        if type(cut).__name__ == "MixedCut":
            if not cut.has_recording or cut.transforms or getattr(cut, "has_video", False):
                return None
            from lhotse.audio.utils import get_audio_duration_mismatch_tolerance
            from lhotse.cut.mixed import _get_audible_tracks

            sr = cut.sampling_rate
            tracks = _get_audible_tracks(cut)
            data = [t for t in tracks if type(t.cut).__name__ != "PaddingCut"]
            if len(data) != 1 or type(data[0].cut).__name__ != "MultiCut" or any(t.snr is not None or t.cut.sampling_rate != sr for t in tracks):
                return None
            inner = pending_channel_chain(data[0].cut, gpu_speed, gpu_resample)
            if inner is None:
                return None
            off = compute_num_samples(data[0].offset, sr)
            total = max(compute_num_samples(t.offset, sr) + compute_num_samples(t.cut.duration, sr) for t in tracks)
            diff = total - cut.num_samples
            if diff < 0 or diff >= max(1, compute_num_samples(get_audio_duration_mismatch_tolerance(), sampling_rate=sr)):
                return None
            return inner[0], inner[1], inner[2], off, int(cut.num_samples)
        if type(cut).__name__ != "MultiCut" or not cut.has_recording or getattr(cut.recording, "has_video", False):
            return None
        channels = cut.channel if isinstance(cut.channel, (list, tuple)) else [cut.channel]
        if not 1 <= len(channels) <= MAX_CHANNELS:
            return None
        chain = _parse_transforms(cut.recording.transforms, int(cut.sampling_rate), gpu_speed, False, gpu_resample, False, True)
        return None if chain is None else (cut, chain.source_rate, chain.factor, 0, None)

    def chain_num_samples(num_samples: int, source_rate: Optional[int], factor: float, sampling_rate: int, blocks=None) -> int:
        """Samples that come out of ``[Resample(source_rate -> sr)]? [Speed(factor)]?`` and the rate steps of the level ``blocks`` behind
        them (``Chain.levels``: the two stages of a band bracket; an oversampling bracket gives back what it took; the level
        ops and the reverb keep the length) for ``num_samples`` going in: per stage ``ceil(new * n / orig)`` in float32 with the rates
        reduced by their gcd (resample.py:219-222, :309)."""
        sr = int(sampling_rate)
        stages = [(source_rate, sr), (None if factor == 1.0 else round(sr * factor), sr)]
        for block in blocks or ():
            for st in block or ():
                if st[0] != "level":
                    stages.append((int(st[1]), int(st[2])) if st[0] == "rate" else (sr, sr * int(st[1])) if st[0] == "up" else (sr * int(st[1]), sr))
        n = int(num_samples)
        for src, dst in stages:
            if src is not None and int(src) != int(dst):
                g = gcd(int(src), int(dst))
                n = int(np.ceil(np.float32((int(dst) // g) * n / (int(src) // g))))
        return n

    def read_before_chain(cut) -> np.ndarray:
        """The segment of the ORIGINAL audio that ``Recording.load_audio`` reads for this cut before it applies the recording's
        transforms (lhotse/audio/recording.py:412-467) -- the backward pass over ALL of them with the reference's own objects
        (recording.py:436-444), then the same per-source reads -> ``(T,)`` for a ``MonoCut``, ``(C, T)`` for a ``MultiCut``."""
        from lhotse.augmentation import AudioTransform  # the reference's own classes: their reverse_timestamps are the contract

        rec = cut.recording
        offset, duration = cut.start, cut.duration
        if duration is not None and isclose(duration, rec.duration, abs_tol=1e-3):
            duration = None  # (recording.py:415-417)
        transforms = [t if isinstance(t, AudioTransform) else AudioTransform.from_dict(t) for t in rec.transforms or []]
        for t in reversed(transforms):
            offset, duration = t.reverse_timestamps(offset=offset, duration=duration, sampling_rate=rec.sampling_rate)
        multi = isinstance(cut.channel, (list, tuple))
        channels = frozenset(cut.channel if multi else [cut.channel])
        per_source = []
        for source in rec.sources:
            if not channels.intersection(source.channels):
                continue
            samples = source.load_audio(offset=offset, duration=duration, force_opus_sampling_rate=rec.sampling_rate)
            drop = [i for i, cid in enumerate(source.channels) if cid not in channels]
            if drop:
                samples = np.delete(samples, drop, axis=0)
            per_source.append(samples)
        audio = np.ascontiguousarray(rec._stack_audio_channels(per_source), dtype=np.float32)
        return audio if multi else audio.reshape(-1)

    def _read_channels(cut, chain, suppress_errors: bool):
        """The entry of ``FusedAudioBatch.audio_of_channels`` for a cut ``pending_channel_chain`` serves (``chain`` = its answer):
        ``(channel rows, factor, source rate, wanted samples, offset, total)``, read in front of the pending transforms -- or, when their
        output would be shorter than the cut (it would need reflect-padding: the rule of ``_read_one``), the reference's own
        ``load_audio`` of the ``MultiCut`` with nothing pending.  None when the read failed and errors are suppressed."""
        with suppress_audio_loading_errors(enabled=suppress_errors):
            data, src, factor, off, total = chain
            sr = data.sampling_rate
            want = compute_num_samples(data.duration, sr)
            if src is not None or factor != 1.0:
                raw = read_before_chain(data)
                if chain_num_samples(raw.shape[-1], src, factor, sr) >= want:
                    return list(raw), factor, src, want, off, total
            audio = data.load_audio()
            return list(np.ascontiguousarray(audio, dtype=np.float32)), 1.0, None, int(audio.shape[-1]), off, total
        return None

    _RIR_CACHE: dict = {}

    def load_reverb_rir(spec: dict) -> np.ndarray:
        """The float32 RIR ``(L,)`` of a reverb the way the reference loads it (lhotse/augmentation/rir.py:116-122): ``to_cut()``,
        ``with_channels``, ``truncate(duration=0.05)`` for ``early_only``, ``load_audio()`` -- through the reference's own class, whose
        ``__post_init__`` reads the manifest back.  Cached per (recording id, channel, early_only)."""
        from lhotse.augmentation import ReverbWithImpulseResponse  # the reference's own class: its loading calls are the contract

        from .augmentation import load_rir

        rir = spec["rir"]
        if isinstance(rir, dict):
            rir = ReverbWithImpulseResponse(rir=rir, rir_channels=list(spec["rir_channels"])).rir
        key = (getattr(rir, "id", None), getattr(getattr(rir, "recording", None), "id", None), getattr(rir, "start", None),
               getattr(rir, "duration", None), spec["rir_channels"][0], spec["early_only"])
        hit = _RIR_CACHE.get(key)
        if hit is None:
            if len(_RIR_CACHE) >= 4096:
                _RIR_CACHE.clear()
            hit = _RIR_CACHE[key] = load_rir(rir, spec["rir_channels"], spec["early_only"])[0]
        return hit

    def _read_track(cut, chain: Chain, offset: int = 0, snr=None, is_ref: bool = True) -> Optional[Track]:
        """The ``Track`` of a mono cut read in front of its ``chain``, or None when the chain's output would be shorter than the cut (it
        would need reflect-padding: the reference's own path).  A chain that keeps the length is read through ``load_audio()`` of the
        cut without its transforms, which fixes the sample count the way the reference does (``assert_and_maybe_fix_num_samples``)."""
        sr = cut.sampling_rate
        want = compute_num_samples(cut.duration, sr)
        if chain.keeps_length:
            from lhotse.utils import fastcopy

            raw = np.ascontiguousarray(fastcopy(cut, recording=fastcopy(cut.recording, transforms=None)).load_audio().reshape(-1), dtype=np.float32)
        else:
            raw = read_before_chain(cut)
            if chain_num_samples(len(raw), chain.source_rate, chain.factor, sr, chain.levels) < want:
                return None
        rv = chain.reverb
        return Track(raw, chain.factor, offset, snr, is_ref, want, None if rv is None else (load_reverb_rir(rv), rv["normalize_output"]),
                     chain.source_rate, chain.levels)

    def _read_one(cut, gpu_speed: bool, suppress_errors: bool, gpu_mix: bool = False, gpu_reverb: bool = False,
                  gpu_resample: bool = False, gpu_level: bool = False) -> Optional[Tuple[torch.Tensor, float, int]]:
        """(samples, factor still to be applied, samples the cut must end up with) or None when the read failed and errors are suppressed.
        For a mixed cut the device will mix, and for a cut with more than a ``Speed`` pending, ``samples`` is the list of its loaded tracks
        (``FusedMiniBatch.features_of_tracks``); a failed track drops the cut.  Whatever the rule refuses, and whatever would come out
        short of the cut (the reference reflect-pads it), is ``cut.load_audio()``."""
        with suppress_audio_loading_errors(enabled=suppress_errors):
            switches = dict(gpu_speed=gpu_speed, gpu_reverb=gpu_reverb, gpu_resample=gpu_resample, gpu_level=gpu_level)
            tracks = deferred_mix(cut, **switches) if gpu_mix else None
            res = None if tracks is None else _read_tracks(cut, tracks)
            if res is not None:
                return res
            chain = parse_chain(cut, bankless=True, **switches)
            track = _read_track(cut, chain) if chain is not None and chain.pending else None
            if track is not None:
                if chain == Chain(factor=chain.factor):  # a Speed and nothing else: the mini-batch may take the route of features_of
                    return torch.from_numpy(track.samples), chain.factor, track.cap
                return [track], 1.0, track.cap
            audio = cut.load_audio()
            if audio.shape[0] == 1:
                audio = audio.squeeze(0)  # collapse channel dim if mono (collation.py:674-675)
            return torch.from_numpy(audio), 1.0, int(audio.shape[-1])
        return None

    def deferred_mix(cut, gpu_reverb: bool = True, gpu_resample: bool = False, gpu_level: bool = False, gpu_speed: bool = True) -> Optional[List[PendingTrack]]:
        """The tracks of a ``MixedCut`` the device can mix -- a ``PendingTrack`` per audible track, ``chain`` = None for a ``PaddingCut``
        track -- or None: load it the reference's way (``cut.load_audio()``).  Decided on the host before anything is read.  Refused:
        anything but a ``MixedCut`` with audio and without video or ``transforms`` of its own; a track that is not a ``PaddingCut`` or a
        mono cut that ``parse_chain`` serves under the same switches (with ``bankless``): multi-channel cuts, nested mixed cuts, other
        transforms, a reverb the device does not serve; tracks at another sampling rate; no determinable, a muted or a padding SNR
        reference track; a first track with an SNR while the reference track is another one (the reference scales it through float64,
        mixed.py:1346-1350); a mix that comes out shorter than ``cut.num_samples`` (reflect-padded, mixed.py:1386-1387) or longer by
        lhotse's tolerance or more.  (A perturbed track that would need reflect-padding is found when it is read, as for a mono cut:
        ``_read_tracks`` returns None and the cut is loaded the reference's way.)"""
        if type(cut).__name__ != "MixedCut" or not cut.has_recording or cut.transforms or getattr(cut, "has_video", False):
            return None
        from lhotse.audio.utils import get_audio_duration_mismatch_tolerance
        from lhotse.cut.mixed import _get_audible_tracks, _get_snr_reference_track  # the reference's own rules are the contract

        try:
            _, ref = _get_snr_reference_track(cut)
        except ValueError:
            return None
        if ref.mute or all(t.mute for t in cut.tracks) or type(ref.cut).__name__ == "PaddingCut":  # (an explicit is_snr_reference on padding: E_ref = 0)
            return None
        tracks = _get_audible_tracks(cut)
        sr = cut.sampling_rate
        if tracks[0].snr is not None and tracks[0] is not ref:
            return None
        out, total = [], 0
        for t in tracks:
            c = t.cut
            if c.sampling_rate != sr:
                return None
            chain = None
            if type(c).__name__ != "PaddingCut":
                chain = parse_chain(c, gpu_speed, gpu_reverb, gpu_resample, gpu_level, bankless=True)
                if chain is None:
                    return None
            off = compute_num_samples(t.offset, sr)
            total = max(total, off + compute_num_samples(c.duration, sr))
            out.append(PendingTrack(c, off, t.snr, t is ref, chain))
        diff = total - cut.num_samples
        if diff < 0 or diff >= max(1, compute_num_samples(get_audio_duration_mismatch_tolerance(), sampling_rate=sr)):
            return None
        return out

    def _read_tracks(cut, tracks: List[PendingTrack]) -> Optional[Tuple[List[Track], float, int]]:
        """The tracks of an eligible mixed cut, each loaded the way a mono cut is (``load_audio`` / ``_read_track``); None when a
        perturbed track would need reflect-padding (the rule of ``_read_one``)."""
        sr = cut.sampling_rate
        loaded = []
        for c, off, snr, is_ref, chain in tracks:
            n = compute_num_samples(c.duration, sr)
            if chain is None:
                loaded.append(Track(n, 1.0, off, snr, is_ref, n))
            elif not chain.pending:
                loaded.append(Track(np.ascontiguousarray(c.load_audio().reshape(-1), dtype=np.float32), 1.0, off, snr, is_ref, n))
            else:
                track = _read_track(c, chain, off, snr, is_ref)
                if track is None:
                    return None
                loaded.append(track)
        return loaded, 1.0, int(cut.num_samples)

    class _ChainReader:
        """The reading half of ``HipOnTheFlyFeatures`` and ``HipAudioSamples``: the cuts of a mini-batch as read in front of the transforms
        the device takes over (``self.gpu_speed_perturb`` / ``gpu_mix`` / ``gpu_reverb`` / ``gpu_resample`` / ``gpu_level``,
        ``self.fault_tolerant``)."""

        def _read(self, cuts, pool, recording_field):
            """read_audio_from_cuts (lhotse/dataset/collation.py:541-600) with the Speed of eligible cuts left for the device."""
            cuts = list(cuts)
            switches = dict(gpu_speed=self.gpu_speed_perturb, gpu_reverb=self.gpu_reverb, gpu_resample=self.gpu_resample, gpu_level=self.gpu_level)

            def pending(cut) -> bool:
                chain = parse_chain(cut, bankless=True, **switches)
                return chain is not None and chain.pending

            on_device = recording_field is None and any((self.gpu_mix and type(c).__name__ == "MixedCut") or pending(c) for c in cuts)
            if not on_device:
                audios, ok = read_audio_from_cuts(cuts, executor=pool, suppress_errors=self.fault_tolerant, recording_field=recording_field)
                return audios, [1.0] * len(audios), [int(a.shape[-1]) for a in audios], ok
            from functools import partial

            from lhotse import CutSet

            map_fn = map if pool is None else pool.map
            audios, factors, wants, ok = [], [], [], []
            read = partial(_read_one, suppress_errors=self.fault_tolerant, gpu_mix=self.gpu_mix, **switches)
            for cut, res in zip(cuts, map_fn(read, cuts)):
                if res is None:
                    continue
                audios.append(res[0]), factors.append(res[1]), wants.append(res[2]), ok.append(cut)
            return audios, factors, wants, CutSet.from_cuts(ok)

    class HipOnTheFlyFeatures(_ChainReader, OnTheFlyFeatures, FusedMiniBatch):
        """Same constructor as ``OnTheFlyFeatures`` plus ``return_device`` (``None`` keeps the padded feature tensor on the
        extractor's GPU, ready for the training step; ``"cpu"`` hands back a host tensor like the reference does) and
        ``gpu_speed_perturb`` / ``gpu_mix`` / ``gpu_reverb`` / ``gpu_resample`` / ``gpu_level`` (see the module docstring), and
        ``return_audio_device`` for the samples of ``return_audio`` (``"cpu"``, the default: as the reference; ``None`` or a device: the
        ``(B, Tmax)`` tensor is collated there, see ``FusedMiniBatch.features_of_tracks``)."""

        def __init__(self, extractor, *args, return_device: Optional[Union[str, torch.device]] = None,
                     return_audio_device: Optional[Union[str, torch.device]] = "cpu", gpu_speed_perturb: Optional[bool] = None, gpu_mix: Optional[bool] = None, gpu_reverb: Optional[bool] = None,
                     gpu_resample: Optional[bool] = None, gpu_level: Optional[bool] = None, reverb_method: str = "direct", **kwargs) -> None:
            if not hasattr(extractor, "extract_collated"):
                raise TypeError("HipOnTheFlyFeatures needs a Hip* extractor (with extract_collated)")
            super().__init__(extractor, *args, **kwargs)
            self.return_device = return_device
            # where `return_audio` hands the samples out: "cpu" (default) = host tensors, collated on the host as the parent does;
            # None (the extractor's device) or a device = collated there by one launch out of the arena the feature launch read
            self.audio_device = "cpu" if return_audio_device is not None and torch.device(return_audio_device).type == "cpu" else return_audio_device
            # None (default) = on the device unless `wave_transforms` are given: those run on the LOADED samples, i.e. after the
            # Speed that Recording.load_audio applies, so with them the reference order (CPU Speed inside load_audio, then the
            # transforms) is kept and the strategy behaves exactly like OnTheFlyFeatures.  An explicit True together with
            # wave_transforms is a contradiction and raises when a perturbed cut is met.
            self._gpu_speed_explicit = gpu_speed_perturb is not None
            self.gpu_speed_perturb = (not self.wave_transforms) if gpu_speed_perturb is None else bool(gpu_speed_perturb)
            # the same for the tracks of mixed cuts: wave_transforms run on the MIXED samples, so with them the mix stays where the
            # reference does it (MixedCut.load_audio); an explicit True together with wave_transforms raises when a mixed cut is met
            self.gpu_mix = (not self.wave_transforms) if gpu_mix is None else bool(gpu_mix)
            # and for a reverb with a recorded RIR at the end of a recording's transforms (ReverbWithImpulseResponse): None = on the
            # device unless wave_transforms are given, False = always Recording.load_audio, True with wave_transforms raises when such a
            # cut is met
            self.gpu_reverb = (not self.wave_transforms) if gpu_reverb is None else bool(gpu_reverb)
            # and for a Resample at the front of a recording's transforms (cuts.resample(sr)): None = on the device unless wave_transforms
            # are given AND only where the reference itself would run its sinc resampler -- without torchaudio its Resample substitutes
            # scipy.signal.resample_poly, another filter (lhotse/augmentation/torchaudio.py:124-139), which the device does not
            # implement; False = always Recording.load_audio; True forces the device's sinc resampler, and raises together with
            # wave_transforms when such a cut is met
            self.gpu_resample = (not self.wave_transforms and _reference_resamples_with_sinc()) if gpu_resample is None else bool(gpu_resample)
            # and for Volume / Clipping in a recording's transforms (PerturbVolume, the Clipping cut transform): None = on the device unless
            # wave_transforms are given, False = always Recording.load_audio, True with wave_transforms raises when such a cut is met.  The
            # oversampled clip (clip_amplitude(oversampling=k)) and a leading Resample in such a chain also need the resampling route, and
            # that only where the reference itself would run its sinc resampler
            self.gpu_level = (not self.wave_transforms) if gpu_level is None else bool(gpu_level)
            # the route of the device reverb: "direct" (the default), "fft" or "auto" (lhotse_amd.augmentation.reverb_in_arena)
            self.reverb_method = _checked_reverb_method(reverb_method)

        def __call__(self, cuts, recording_field: Optional[str] = None):
            """Only the middle of the parent's pipeline differs: ``extract_batch`` + ``collate_matrices`` become ONE fused launch, and
            pending speed factors are applied to the packed batch on the device in front of it.  The parent offers no hook between
            reading the audio and collating the features, so the two ends of its pipeline are invoked here through the same public
            helpers it uses."""
            pool = _get_executor(self.num_workers, executor_type=self._executor_type)
            audios, factors, wants, cuts = self._read(cuts, pool, recording_field)
            mixed = any(isinstance(a, list) for a in audios)  # (the loaded tracks of the cuts the device mixes)
            for transform in self.wave_transforms:
                if any(isinstance(a, list) and any(t.levels is not None for t in a) for a in audios):
                    raise ValueError("gpu_level=True was requested together with wave_transforms: the transforms run on the scaled and clipped "
                                     "samples, before the device scales and clips them; leave gpu_level at its default (None: "
                                     "Recording.load_audio whenever wave_transforms are given) or pass False")
                if any(isinstance(a, list) and any(t.source_rate is not None for t in a) for a in audios):
                    raise ValueError("gpu_resample=True was requested together with wave_transforms: the transforms run on the resampled "
                                     "samples, before the device resamples them; leave gpu_resample at its default (None: "
                                     "Recording.load_audio whenever wave_transforms are given) or pass False")
                if any(isinstance(a, list) and any(t.reverb is not None for t in a) for a in audios):
                    raise ValueError("gpu_reverb=True was requested together with wave_transforms: the transforms run on the reverberated "
                                     "samples, before the device convolves them; leave gpu_reverb at its default (None: "
                                     "Recording.load_audio whenever wave_transforms are given) or pass False")
                if mixed:
                    raise ValueError("gpu_mix=True was requested together with wave_transforms: the transforms run on the mixed samples, "
                                     "before the device mixes the tracks; leave gpu_mix at its default (None: MixedCut.load_audio whenever "
                                     "wave_transforms are given) or pass False")
                if any(f != 1.0 for f in factors):
                    raise ValueError("gpu_speed_perturb=True was requested together with wave_transforms: the transforms run on the loaded "
                                     "samples, before the device applies the pending speed factors; leave gpu_speed_perturb at its default "
                                     "(None: the reference's CPU Speed whenever wave_transforms are given) or pass False")
                audios = [transform(a) for a in audios]
            rates = {c.sampling_rate for c in cuts}
            assert len(rates) == 1, f"one launch per batch needs a single sampling rate, got {sorted(rates)}"
            sr = rates.pop()
            if mixed:  # (FusedMiniBatch.features_of_tracks: a plain cut is a cut of one track)
                tracks = [a if isinstance(a, list) else [Track(a, f, 0, None, True)] for a, f in zip(audios, factors)]
                feats, feat_lens, *audio = self._mix_and_extract(tracks, wants, sr, *(() if self.reverb_method == "direct" else (self.reverb_method,)))
            elif any(f != 1.0 for f in factors):  # (FusedMiniBatch.features_of, with the perturbed samples kept for `return_audio`)
                feats, feat_lens, *audio = self._perturb_and_extract(audios, factors, wants, sr)
            else:
                feats, feat_lens, *audio = self._plain_extract(audios, sr)
            result = [feats if self.return_device is None else feats.to(self.return_device), feat_lens]
            if self.return_audio and self.audio_device != "cpu":  # (B, Tmax) zero-padded samples, collated on the device, + their lengths
                result += audio
            elif self.return_audio:  # (B, Tmax) zero-padded samples + their lengths, as the parent returns them
                flat = [a.reshape(-1) for a in audio[0]]
                result += [collate_vectors(flat, padding_value=0), torch.tensor([len(a) for a in flat], dtype=torch.int64)]
            if self.fault_tolerant:  # the cuts that survived audio loading
                result.append(cuts)
            return tuple(result)

    def _num_channels(cut) -> int:
        try:
            return int(cut.num_channels or 1)
        except Exception:  # noqa: BLE001  (a cut that cannot say: the reference's path decides)
            return 2

    class HipAudioSamples(_ChainReader, AudioSamples):
        """``AudioSamples`` (lhotse/dataset/input_strategies.py:208-299) with the transforms of the cuts and the collation on the GPU: the
        cuts are read in front of the transforms the device takes over (as ``HipOnTheFlyFeatures`` reads them), the chain runs in one arena
        and ONE launch writes the zero-padded ``(B, T)`` tensor (``FusedAudioBatch``).  Same constructor as ``AudioSamples`` plus ``device``
        (where the chain runs), ``return_device`` (``None`` keeps the samples there, ``"cpu"`` hands back a host tensor like the reference),
        ``dtype`` (float32, float16 or bfloat16 samples) and ``gpu_speed_perturb`` / ``gpu_mix`` / ``gpu_reverb`` / ``gpu_resample`` /
        ``gpu_level`` with the meaning and defaults they have on ``HipOnTheFlyFeatures`` (there are no ``wave_transforms`` here: None = on).
        Returns ``(audio, audio_lens[, cuts])`` with the parent's int32 lengths and its ``fault_tolerant`` contract.

        Multi-channel batches (``gpu_channels``; ``mono_downmix`` None / True / False as on the parent): a batch with ``MultiCut``s that
        ``pending_channel_chain`` serves, and any batch with ``mono_downmix=False``, is collated by ONE launch as ``(B, T)`` -- a cut's row
        is the correctly rounded mean over its channels -- or ``(B, C, T)`` (``FusedAudioBatch.audio_of_channels``); the mono cuts of
        such a batch keep their whole device chain.  ``gpu_channels``: None = on where ``device`` is a GPU, False = the parent's path.

        The parent's own ``__call__`` runs, and its result is moved to ``return_device`` (None: ``device``), for ``recording_field``,
        ``use_batch_loader`` and a batch with a multi-channel cut that ``pending_channel_chain`` refuses (a transform other than
        ``[Resample]? [Speed]?``, a multi-channel track mixed with audio, more than 32 channels)."""

        def __init__(self, *args, device: Union[str, torch.device, None] = None, return_device: Optional[Union[str, torch.device]] = None,
                     dtype: torch.dtype = torch.float32, gpu_speed_perturb: Optional[bool] = None, gpu_mix: Optional[bool] = None,
                     gpu_reverb: Optional[bool] = None, gpu_resample: Optional[bool] = None, gpu_level: Optional[bool] = None,
                     gpu_channels: Optional[bool] = None, reverb_method: str = "direct", **kwargs) -> None:
            super().__init__(*args, **kwargs)
            self.batch = FusedAudioBatch(device, dtype)
            self.reverb_method = _checked_reverb_method(reverb_method)  # the route of the device reverb (reverb_in_arena), mono cuts
            self.device, self.dtype, self.return_device = self.batch.device, dtype, return_device
            self.gpu_speed_perturb = True if gpu_speed_perturb is None else bool(gpu_speed_perturb)
            self.gpu_mix = True if gpu_mix is None else bool(gpu_mix)
            self.gpu_reverb = True if gpu_reverb is None else bool(gpu_reverb)
            # (only where the reference itself would run its sinc resampler, as on HipOnTheFlyFeatures)
            self.gpu_resample = _reference_resamples_with_sinc() if gpu_resample is None else bool(gpu_resample)
            self.gpu_level = True if gpu_level is None else bool(gpu_level)
            # multi-channel cuts and the (B, C, T) form: None = on where the chain has a GPU to run on (a CPU `device` has no launch
            # that could write the batch: the parent's path, as before), False = always the parent's path
            self.gpu_channels = (self.device.type == "cuda") if gpu_channels is None else bool(gpu_channels)

        def _moved(self, result):
            dev = self.device if self.return_device is None else self.return_device
            return (result[0].to(dev),) + tuple(result[1:])

        def _channel_chains(self, cuts):
            """Per cut of a batch that needs the channel route: None for a cut of one channel (the mono route reads it), else the answer of
            ``pending_channel_chain``; the whole result is None when the parent has to serve the batch."""
            if not self.gpu_channels:
                return None
            chains = [None if _num_channels(c) == 1 else pending_channel_chain(c, self.gpu_speed_perturb, self.gpu_resample) for c in cuts]
            return None if any(ch is None and _num_channels(c) != 1 for c, ch in zip(cuts, chains)) else chains

        def _call_channels(self, cuts, chains):
            """The batch through ``FusedAudioBatch.audio_of_channels``: multi-channel cuts as their channel rows, every other cut as the
            tracks the mono route reads."""
            from lhotse import CutSet

            pool = _get_executor(self.num_workers, executor_type=self._executor_type)
            map_fn = map if pool is None else pool.map

            def read(pair):
                cut, chain = pair
                if chain is not None:
                    return _read_channels(cut, chain, self.fault_tolerant)
                res = _read_one(cut, gpu_speed=self.gpu_speed_perturb, suppress_errors=self.fault_tolerant, gpu_mix=self.gpu_mix,
                                gpu_reverb=self.gpu_reverb, gpu_resample=self.gpu_resample, gpu_level=self.gpu_level)
                if res is None:
                    return None
                a, f, want = res
                return (a if isinstance(a, list) else [Track(a, f, 0, None, True)]), 1.0, None, want, None, None

            entries, ok = [], []
            for cut, res in zip(cuts, map_fn(read, list(zip(cuts, chains)))):
                if res is not None:
                    entries.append(res), ok.append(cut)
            if not entries:
                raise ValueError("HipAudioSamples: no cut of the mini-batch could be read")
            rates = {c.sampling_rate for c in ok}
            assert len(rates) == 1, f"one launch per batch needs a single sampling rate, got {sorted(rates)}"
            chans, factors, srcs, wants, offs, totals = (list(x) for x in zip(*entries))
            audio, lens = self.batch.audio_of_channels(chans, factors, srcs, wants, rates.pop(), self.mono_downmix, offs, totals)
            result = self._moved((audio, lens.to(torch.int32)))  # (collation.py:242)
            return result + (CutSet.from_cuts(ok),) if self.fault_tolerant else result

        def __call__(self, cuts, recording_field: Optional[str] = None):
            if recording_field is not None or self.use_batch_loader:
                return self._moved(super().__call__(cuts, recording_field=recording_field))
            if self.mono_downmix is False or any(_num_channels(c) != 1 for c in cuts):
                chains = self._channel_chains(list(cuts))
                if chains is None:
                    return self._moved(super().__call__(cuts, recording_field=recording_field))
                return self._call_channels(list(cuts), chains)
            pool = _get_executor(self.num_workers, executor_type=self._executor_type)
            audios, factors, wants, ok = self._read(cuts, pool, None)
            if not len(audios):
                raise ValueError("HipAudioSamples: no cut of the mini-batch could be read")
            rates = {c.sampling_rate for c in ok}
            assert len(rates) == 1, f"one launch per batch needs a single sampling rate, got {sorted(rates)}"
            sr = rates.pop()
            if any(isinstance(a, list) for a in audios):  # (the loaded tracks of the cuts the device mixes, reverberates, resamples, scales)
                tracks = [a if isinstance(a, list) else [Track(a, f, 0, None, True)] for a, f in zip(audios, factors)]
                audio, lens = self.batch.audio_of_tracks(tracks, wants, sr, *(() if self.reverb_method == "direct" else (self.reverb_method,)))
            else:
                audio, lens = self.batch.audio_of(audios, factors, wants, sr)
            result = self._moved((audio, lens.to(torch.int32)))  # (collation.py:242)
            return result + (ok,) if self.fault_tolerant else result

    # ---- precomputed features: CutMix / padding mixed and collated on the device --------------------------------------------------
    _ARCHIVE_STORAGES = ("hip_archive", "hip_archive_f16")
    _LOG_DOMAIN_TYPES: Optional[frozenset] = None
    _archive_readers: Dict[Tuple[str, str], object] = {}

    def _method_body(fn) -> str:
        """The statements of a function without its signature, comments and layout (the dump of its syntax tree's body)."""
        import ast
        import inspect
        import textwrap

        body = ast.parse(textwrap.dedent(inspect.getsource(fn))).body[0].body
        return "\n".join(ast.dump(st) for st in body)

    def log_domain_feature_types() -> frozenset:
        """The ``features.type`` names whose mix is the log-sum-exp pair of ``Fbank`` (lhotse/features/kaldi/extractors.py:135-152:
        ``log(max(EPSILON, exp(a) + g * exp(b)))`` and ``sum(exp(x))``): ``kaldi-fbank``, ``hip-fbank``, and every other registered
        extractor whose ``mix`` / ``compute_energy`` bodies are exactly those.  ``Spectrogram``'s linear mix is not among them."""
        global _LOG_DOMAIN_TYPES
        if _LOG_DOMAIN_TYPES is None:
            from lhotse.features.base import FEATURE_EXTRACTORS  # type: ignore
            from lhotse.features.kaldi.extractors import Fbank  # type: ignore

            from .extractors import _log_mix

            want = (_method_body(Fbank.mix), _method_body(Fbank.compute_energy))
            names = {"kaldi-fbank", "hip-fbank"}
            for name, cls in FEATURE_EXTRACTORS.items():
                try:
                    if getattr(cls, "mix", None) is _log_mix or (_method_body(cls.mix), _method_body(cls.compute_energy)) == want:
                        names.add(name)
                except Exception:  # noqa: BLE001  (no source to read: not served)
                    pass
            _LOG_DOMAIN_TYPES = frozenset(names)
        return _LOG_DOMAIN_TYPES

    def _archive_reader(storage_type: str, storage_path: str):
        from lhotse.features.io import get_reader  # type: ignore

        r = _archive_readers.get((storage_type, storage_path))
        if r is None:
            r = _archive_readers[(storage_type, storage_path)] = get_reader(storage_type)(storage_path)
        return r

    def _feature_track(cut, num_features: int) -> Optional[dict]:
        """The source of one single-channel cut's features, or None: a PaddingCut is a constant; a cut stored in ``hip_archive`` /
        ``hip_archive_f16`` is read raw with the frame range ``Features.load`` computes (lhotse/features/base.py:488-524); every other
        storage is loaded through ``cut.load_features()`` here and uploaded as float32."""
        from lhotse.cut import MonoCut, PaddingCut  # type: ignore
        from lhotse.utils import compute_num_frames  # type: ignore

        if isinstance(cut, PaddingCut):
            return {"frames": int(cut.num_frames), "value": float(cut.feat_value)}
        if not isinstance(cut, MonoCut) or not cut.has_features or int(cut.num_features) != num_features:
            return None
        f, frames = cut.features, int(cut.num_frames)
        if f.storage_type in _ARCHIVE_STORAGES:
            from math import isclose

            from .storage import _parse_key

            _, rows, cols, dt = _parse_key(f.storage_key)
            if cols != num_features or cut.start < f.start - 1e-3:
                return None
            lo = 0 if isclose(cut.start, f.start) else compute_num_frames(cut.start - f.start, frame_shift=f.frame_shift, sampling_rate=f.sampling_rate)
            hi = lo + compute_num_frames(cut.duration, frame_shift=f.frame_shift, sampling_rate=f.sampling_rate)
            n = max(0, min(rows, hi) - max(0, lo))
            if abs(n - frames) > 1 or (frames > 0 and n < 1):
                return None
            reader, key = _archive_reader(f.storage_type, f.storage_path), f.storage_key
            return {"frames": frames, "rows": n, "f16": dt == "<f2", "read": lambda out: reader.read_raw(key, lo, hi, out=out)}
        m = cut.load_features()  # (the fix-up of mono.py:61-64 applied)
        if m is None or m.ndim != 2 or m.shape != (frames, num_features):
            return None
        return {"frames": frames, "array": np.ascontiguousarray(m, dtype=np.float32)}

    def pending_feature_mix(cut) -> Optional[dict]:
        """The track table of one (padded) cut for ``FusedFeatureBatch``, or None when the cut keeps lhotse's own path: the classifier of
        ``MixedCut.load_features`` (lhotse/cut/mixed.py:1199-1309).  None for: multi-channel (3-D) features, tracks with differing
        ``num_features`` or ``frame_shift``, a frame-count mismatch beyond +-1, more than 256 tracks, a fold whose ``features.type`` is
        not a log-domain type (``log_domain_feature_types``), a fold of a single audible track, and a reference track that is muted."""
        from lhotse.cut import MixedCut, MonoCut, PaddingCut  # type: ignore
        from lhotse.utils import compute_num_frames  # type: ignore

        from .augmentation import FEATMIX_COPY, FEATMIX_FOLD, FEATMIX_MAX_TRACKS

        if not getattr(cut, "has_features", False):
            return None
        F, T = int(cut.num_features), int(cut.num_frames)
        if isinstance(cut, (MonoCut, PaddingCut)):
            tr = _feature_track(cut, F)
            return None if tr is None else {"form": FEATMIX_COPY, "num_frames": T, "pad_value": 0.0, "ref_track": -1, "num_features": F, "tracks": [tr]}
        if not isinstance(cut, MixedCut):
            return None
        tracks = [t for t in cut.tracks if not getattr(t, "mute", False)] or list(cut.tracks)  # (_get_audible_tracks)
        if len(tracks) > FEATMIX_MAX_TRACKS or not all(isinstance(t.cut, (MonoCut, PaddingCut)) for t in tracks):
            return None
        shift = tracks[0].cut.frame_shift
        if any(t.cut.num_features != F or t.cut.frame_shift != shift for t in tracks):
            return None
        first = tracks[0]
        if first.snr is None and tracks[1:] and all(isinstance(t.cut, PaddingCut) for t in tracks[1:]):  # (mixed.py:1223-1243)
            tr = _feature_track(first.cut, F)
            if tr is None or tr["frames"] > T:
                return None
            return {"form": FEATMIX_COPY, "num_frames": T, "pad_value": float(tracks[1].cut.feat_value), "ref_track": -1, "num_features": F, "tracks": [tr]}
        if len(tracks) < 2:  # (the reference hands the one track back as it is: not a fold)
            return None
        try:
            from lhotse.cut.mixed import _get_snr_reference_track  # type: ignore

            _, ref_track = _get_snr_reference_track(cut)
        except Exception:  # noqa: BLE001  (no reference can be told: lhotse's path raises its own error)
            return None
        ref = next((i for i, t in enumerate(tracks) if t is ref_track), -1)
        if ref < 0 or getattr(ref_track.cut, "features_type", None) not in log_domain_feature_types():
            return None
        out, total = [], 0
        for i, t in enumerate(tracks):
            tr = _feature_track(t.cut, F)
            if tr is None:
                return None
            tr["first"] = 0 if i == 0 else compute_num_frames(t.offset, frame_shift=shift, sampling_rate=t.cut.sampling_rate)
            tr["snr"] = None if t.snr is None else float(t.snr)
            if i == 0 or tr["frames"] > 0:
                total = max(total, tr["first"] + tr["frames"])
            out.append(tr)
        if abs(total - T) > 1 or (T > 0 and total < 1):  # (the reference's assertion, mixed.py:1301-1306)
            return None
        return {"form": FEATMIX_FOLD, "num_frames": T, "pad_value": 0.0, "ref_track": ref, "num_features": F, "tracks": out}

    class HipPrecomputedFeatures(PrecomputedFeatures):
        """``PrecomputedFeatures`` (lhotse/dataset/input_strategies.py:102-129) with the mix and the collation on the GPU: the stored
        tracks of the padded cuts go to the device as they were stored and two launches write the ``(B, T, F)`` batch
        (``FusedFeatureBatch``) -- what ``collate_features`` (lhotse/dataset/collation.py:115-145) does per cut on the host through
        ``MixedCut.load_features`` and ``FeatureMixer``.  Same constructor as the parent plus ``device`` (where the launches run) and
        ``return_device`` (``None`` keeps the batch there, ``"cpu"`` hands back a host tensor like the reference).  Returns
        ``(features, features_lens)`` with the parent's dtypes; ``supervision_intervals`` is inherited.

        The parent's own ``__call__`` runs, and its result is moved to ``return_device`` (None: ``device``), when ``pending_feature_mix``
        returns None for any cut of the batch or the cuts differ in ``num_features``."""

        def __init__(self, *args, device: Union[str, torch.device, None] = None, return_device: Optional[Union[str, torch.device]] = None, **kwargs) -> None:
            super().__init__(*args, **kwargs)
            self.batch = FusedFeatureBatch(device)
            self.device, self.return_device = self.batch.device, return_device

        def _moved(self, result):
            dev = self.device if self.return_device is None else self.return_device
            return (result[0].to(dev),) + tuple(result[1:])

        def __call__(self, cuts, pad_direction: Optional[str] = "right"):
            assert all(cut.has_features for cut in cuts)
            lens = torch.tensor([cut.num_frames for cut in cuts], dtype=torch.int)  # (collation.py:133)
            padded = cuts.pad(num_frames=max(lens).item(), direction=pad_direction)
            tables = []
            for cut in padded:
                tab = pending_feature_mix(cut)
                if tab is None or (tables and tab["num_features"] != tables[0]["num_features"]):
                    return self._moved(super().__call__(cuts, pad_direction=pad_direction))
                tables.append(tab)
            pool = _get_executor(self.num_workers, executor_type=self._executor_type)
            if pool is not None and not isinstance(pool, ThreadPoolExecutor):  # (the reads fill this process's staging buffer)
                pool = None
            feats, _ = self.batch.features_of(tables, tables[0]["num_features"], int(max(lens).item()), pool)
            return self._moved((feats, lens))


else:

    class HipOnTheFlyFeatures:  # type: ignore[no-redef]
        def __init__(self, *args, **kwargs):
            raise ImportError("HipOnTheFlyFeatures consumes lhotse CutSets: install lhotse (lhotse.dataset.input_strategies.OnTheFlyFeatures)")

    class HipAudioSamples:  # type: ignore[no-redef]
        def __init__(self, *args, **kwargs):
            raise ImportError("HipAudioSamples consumes lhotse CutSets: install lhotse (lhotse.dataset.input_strategies.AudioSamples)")

    class HipPrecomputedFeatures:  # type: ignore[no-redef]
        def __init__(self, *args, **kwargs):
            raise ImportError("HipPrecomputedFeatures consumes lhotse CutSets: install lhotse (lhotse.dataset.input_strategies.PrecomputedFeatures)")
