// Host-side tables of the mix kernels (kernel_mix.hpp): what hipfeat_mix_plan validates and builds, once per plan.
// Pure C++ (no HIP): also compiled by tests/native/mix_tables_capi.cpp and checked on the CPU (tests/test_mix_abi.py).
//
// A CUT is mixed from its TRACKS [h_track_first[c], h_track_first[c + 1]): track t contributes the src_len float32 samples at arena +
// src_offset (-1: a padding track, no source) from sample dst_offset of the cut on, scaled to its SNR against the cut's reference track
// (NaN or no reference: gain 1).  The mixed cuts are written from tail_start on, each on a 16-byte boundary.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace hipfeat {

constexpr int kMixEnergyBlock = 16384;  // samples per energy item (256 lanes x 64): a 30 s track at 16 kHz is 30 partials
constexpr int kMixBlock = 4096;         // output samples per mix item (256 lanes x 4 x float4)
constexpr int kMixMaxTracks = 256;      // tracks of one cut (their gains live in LDS, one lane forms each)

struct MixTrack {
  int64_t src_off;     // arena offset of the track's samples; < 0: a padding track (no source)
  int32_t src_len;     // samples
  int32_t dst_off;     // first sample of the track inside its cut
  int32_t part_first;  // exclusive prefix sum of the tracks' energy items = index of the track's first partial
  int32_t part_count;  // 0: no energy needed
  double ratio;        // 10^(-snr/10); < 0: no SNR (gain 1)
};
struct MixCut {
  int64_t out_off;      // arena offset of the mixed cut (16-byte aligned)
  int32_t out_len;      // samples written
  int32_t item_first;   // exclusive prefix sum of the cuts' mix items
  int32_t track_first;  // tracks of the cut = [track_first, track_first + track_count)
  int32_t track_count;
  int32_t ref_track;    // index into the track table, < 0: none
  int32_t pad;
};
static_assert(sizeof(MixTrack) == 32 && sizeof(MixCut) == 32, "descriptor size");

struct MixPlan {
  int status = 0;       // 0 OK, 1 INVALID, 3 UNSUPPORTED (hipfeat_status)
  std::string message;  // of a refusal
  std::vector<MixCut> cuts;
  std::vector<MixTrack> tracks;
  int64_t energy_items = 0, mix_items = 0, arena_need = 0;
};

#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline MixPlan mix_refuse(int status, const char* fmt, ...) {
  MixPlan p;
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  p.status = status;
  p.message = buf;
  return p;
}

// h_track_first[num_cuts + 1]; h_snr_db, h_ref_track, h_max_samples may be nullptr (no SNR, no reference, no truncation)
inline MixPlan build_mix_plan(int64_t num_cuts, const int64_t* h_track_first, const int64_t* h_src_offset, const int64_t* h_src_len, const int64_t* h_dst_offset,
                              const double* h_snr_db, const int32_t* h_ref_track, const int64_t* h_max_samples, int64_t tail_start) {
  if (!h_track_first || !h_src_offset || !h_src_len || !h_dst_offset) return mix_refuse(1, "NULL argument");
  if (num_cuts <= 0 || num_cuts > 65535) return mix_refuse(1, "bad batch arguments (1 ... 65535 cuts)");
  if (tail_start < 0) return mix_refuse(1, "tail_start %lld is negative", (long long)tail_start);
  if (h_track_first[0] != 0) return mix_refuse(1, "h_track_first[0] must be 0");
  constexpr int64_t kMaxLen = INT32_MAX / 2;
  MixPlan p;
  p.cuts.resize((size_t)num_cuts);
  std::vector<MixTrack>& tracks = p.tracks;
  int64_t tail = (tail_start + 3) & ~(int64_t)3, parts = 0, items = 0;
  for (int64_t c = 0; c < num_cuts; ++c) {
    const int64_t t0 = h_track_first[c], t1 = h_track_first[c + 1], nt = t1 - t0;
    if (nt < 1 || t0 > INT32_MAX / 4) return mix_refuse(1, "cut %lld: tracks [%lld, %lld): every cut has at least one track", (long long)c, (long long)t0, (long long)t1);
    if (nt > kMixMaxTracks) return mix_refuse(3, "cut %lld has %lld tracks, the mix launch serves up to %d per cut", (long long)c, (long long)nt, kMixMaxTracks);
    const int64_t ref = h_ref_track ? h_ref_track[c] : -1;
    if (ref < -1 || ref >= nt) return mix_refuse(1, "cut %lld: reference track %lld of %lld", (long long)c, (long long)ref, (long long)nt);
    if (ref >= 0 && h_src_offset[t0 + ref] < 0) return mix_refuse(1, "cut %lld: reference track %lld is a padding track", (long long)c, (long long)ref);
    int64_t total = 0;
    bool any_snr = false;
    for (int64_t t = t0; t < t1; ++t) {
      const int64_t so = h_src_offset[t], n = h_src_len[t], off = h_dst_offset[t];
      const bool padding = so == -1;
      if (so < -1 || off < 0) return mix_refuse(1, "cut %lld, track %lld: negative offset (source %lld, in the cut %lld)", (long long)c, (long long)(t - t0), (long long)so, (long long)off);
      if (n < (padding ? 0 : 1) || n > kMaxLen || off + n > kMaxLen)
        return mix_refuse(1, "cut %lld, track %lld: %lld samples at offset %lld out of range", (long long)c, (long long)(t - t0), (long long)n, (long long)off);
      if (!padding && so + n > tail_start)  // the mixed cuts are written from tail_start on: output and source ranges would overlap
        return mix_refuse(1, "cut %lld, track %lld (offset %lld, %lld samples) reaches into the arena's tail (tail_start %lld), where the mixed cuts are written",
                          (long long)c, (long long)(t - t0), (long long)so, (long long)n, (long long)tail_start);
      const double snr = h_snr_db ? h_snr_db[t] : NAN;
      // no SNR, no reference, a padding track, or the first track being the reference itself (mixed.py:1346-1350): gain 1
      const bool scaled = !std::isnan(snr) && ref >= 0 && !padding && !(t == t0 && ref == 0);
      MixTrack tr{};
      tr.src_off = so;
      tr.src_len = (int32_t)n;
      tr.dst_off = (int32_t)off;
      tr.part_first = 0;
      tr.part_count = scaled ? 1 : 0;  // (flag; counted below)
      tr.ratio = scaled ? std::pow(10.0, -snr / 10.0) : -1.0;
      if (scaled && !(tr.ratio >= 0.0 && std::isfinite(tr.ratio))) return mix_refuse(1, "cut %lld, track %lld: SNR %g dB out of range", (long long)c, (long long)(t - t0), snr);
      any_snr |= scaled;
      tracks.push_back(tr);
      total = std::max(total, off + n);
    }
    if (any_snr) tracks[(size_t)(t0 + ref)].part_count = 1;
    for (int64_t t = t0; t < t1; ++t) {
      MixTrack& tr = tracks[(size_t)t];
      tr.part_first = (int32_t)parts;
      if (tr.part_count) tr.part_count = (tr.src_len + kMixEnergyBlock - 1) / kMixEnergyBlock;
      parts += tr.part_count;
    }
    int64_t n_out = total;
    if (h_max_samples && h_max_samples[c] >= 0) n_out = std::min(n_out, h_max_samples[c]);  // (mixed.py:1381-1385: a sample or two to truncate)
    if (n_out < 1) return mix_refuse(1, "cut %lld: the mix is empty", (long long)c);
    MixCut& cd = p.cuts[(size_t)c];
    cd.out_off = tail;
    cd.out_len = (int32_t)n_out;
    cd.item_first = (int32_t)items;
    cd.track_first = (int32_t)t0;
    cd.track_count = (int32_t)nt;
    cd.ref_track = ref >= 0 ? (int32_t)(t0 + ref) : -1;
    cd.pad = 0;
    items += (n_out + kMixBlock - 1) / kMixBlock;
    tail += (n_out + 3) & ~(int64_t)3;
    if (items > INT32_MAX - (1 << 24) || parts > INT32_MAX - (1 << 24)) return mix_refuse(1, "batch too large for one launch");
  }
  p.energy_items = parts;
  p.mix_items = items;
  p.arena_need = tail;
  return p;
}

}  // namespace hipfeat
