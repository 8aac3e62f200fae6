// Host-side tables of the feature-mix kernels (kernel_featmix.hpp): what hipfeat_featmix_plan validates and builds, once per plan.
// Pure C++ (no HIP): also compiled by tests/native/featmix_tables_capi.cpp and checked on the CPU (tests/test_featmix_abi.py).
//
// Reference: collate_features (lhotse/dataset/collation.py:115-145) pads every cut of a mini-batch (cuts.pad) and fills row c of a
// (B, max num_frames, F) float32 tensor with cut.load_features(); for a MixedCut that is the copy of a single padded cut
// (lhotse/cut/mixed.py:1223-1243) or the FeatureMixer fold of its tracks (mixed.py:1245-1307, lhotse/features/mixer.py).
//
// A CUT is made from its TRACKS [h_track_first[c], h_track_first[c + 1]).  Track t is a stored matrix of `rows` rows of F values at BYTE
// offset src_off of the arena (float32, or binary16 with the dtype flag), or a constant matrix (src_off -1: a PaddingCut); it stands for
// `frames` frames (the MonoCut fix-up, lhotse/cut/mono.py:61-64: frames == rows - 1 drops the last stored row, frames == rows + 1 repeats
// it) from frame `first` of the cut on.  The cut's num_frames frames go to frames [dst_first, dst_first + num_frames) of row c of `out`.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "ticket_slots.hpp"

namespace hipfeat {

constexpr int kFmEnergyBlock = 16384;  // track elements per energy item (256 lanes x 64)
constexpr int kFmTile = 4096;          // output elements per fold item (256 lanes x 4 x 16-byte stores)
constexpr int kFmMaxTracks = 256;      // tracks of one cut (their gains live in LDS, one lane forms each)

constexpr int32_t kFmCopy = 0, kFmFold = 1;  // forms
constexpr int32_t kFmF32 = 0, kFmF16 = 1;    // track types

struct FmTrack {
  int64_t src_off;     // BYTE offset of the track's first stored value in the arena; < 0: a constant track (no source)
  int32_t frames;      // frames the track stands for
  int32_t rows;        // stored rows (frames - 1 ... frames + 1; a constant track: == frames)
  int32_t first;       // first frame of the track inside its cut
  int32_t f16;         // 1: binary16 values, 0: float32
  int32_t part_first;  // exclusive prefix sum of the tracks' energy items = index of the track's first partial
  int32_t part_count;  // 0: no partial sums (no energy needed, or a constant track: its energy is frames * F * exp(value))
  double ratio;        // 10^(-snr/10); < 0: gain 1
  float value;         // of a constant track
  int32_t pad;
};
struct FmCut {
  int32_t track_first;  // tracks of the cut = [track_first, track_first + track_count)
  int32_t track_count;
  int32_t form;         // kFmCopy / kFmFold
  int32_t num_frames;   // frames of the cut written to its row
  int32_t dst_first;    // first frame of the row that receives them
  int32_t mix_frames;   // fold: N = max(first + frames) over the tracks (num_frames - 1 ... num_frames + 1)
  int32_t ref_track;    // index into the track table, < 0: none
  float pad_value;      // copy form: the frames of the cut behind track 0
};
static_assert(sizeof(FmTrack) == 48 && sizeof(FmCut) == 32, "descriptor size");

struct FmPlan {
  int status = 0;       // 0 OK, 1 INVALID, 3 UNSUPPORTED (hipfeat_status)
  std::string message;  // of a refusal
  std::vector<FmCut> cuts;
  std::vector<FmTrack> tracks;
  int64_t num_features = 0, row_frames = 0, row_len = 0, tiles_per_row = 0;
  int64_t energy_items = 0, fold_items = 0, arena_need = 0, out_need = 0;
};

#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline FmPlan fm_refuse(int status, const char* fmt, ...) {
  FmPlan p;
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  p.status = status;
  p.message = buf;
  return p;
}

// work items of a row: tiles of kFmTile elements counted from the 16-byte boundary at or below the row's first element, which lies at
// most 3 elements in front of it (rows start at c * row_len: every row has its own alignment)
inline int64_t fm_tiles(int64_t row_len) { return row_len == 0 ? 0 : (row_len - 1 + 3) / kFmTile + 1; }

// per cut: h_track_first[num_cuts + 1], h_form, h_num_frames, h_pad_value, h_dst_first (nullptr: 0), h_ref_track (nullptr: none; an index
// WITHIN the cut).  per track: h_src_offset (bytes; -1: constant), h_src_rows (nullptr: == h_frames), h_frames, h_dtype (nullptr: float32),
// h_first (nullptr: 0), h_snr_db (nullptr / NaN: none), h_value (nullptr: 0; of constant tracks)
inline FmPlan build_featmix_plan(int64_t num_cuts, const int64_t* h_track_first, const int32_t* h_form, const int64_t* h_num_frames, const double* h_pad_value,
                                 const int64_t* h_dst_first, const int32_t* h_ref_track, const int64_t* h_src_offset, const int64_t* h_src_rows,
                                 const int64_t* h_frames, const int32_t* h_dtype, const int64_t* h_first, const double* h_snr_db, const double* h_value,
                                 int64_t num_features, int64_t row_frames) {
  if (!h_track_first || !h_form || !h_num_frames || !h_src_offset || !h_frames) return fm_refuse(1, "NULL argument");
  if (num_cuts <= 0 || num_cuts > 65535) return fm_refuse(1, "bad batch arguments (1 ... 65535 cuts)");
  constexpr int64_t kMaxRow = INT32_MAX / 2;  // elements of one row, and of one track: 32-bit arithmetic inside a row
  if (num_features < 1 || num_features > kMaxRow) return fm_refuse(1, "%lld features per frame", (long long)num_features);
  if (row_frames < 0 || row_frames > kMaxRow / num_features)
    return fm_refuse(1, "a row of %lld frames of %lld features is out of range", (long long)row_frames, (long long)num_features);
  if (h_track_first[0] != 0) return fm_refuse(1, "h_track_first[0] must be 0");
  const int64_t F = num_features, max_frames = kMaxRow / F;
  FmPlan p;
  p.cuts.resize((size_t)num_cuts);
  std::vector<FmTrack>& tracks = p.tracks;
  int64_t parts = 0;
  for (int64_t c = 0; c < num_cuts; ++c) {
    const int64_t t0 = h_track_first[c], t1 = h_track_first[c + 1], nt = t1 - t0;
    if (nt < 1 || t0 > INT32_MAX / 4) return fm_refuse(1, "cut %lld: tracks [%lld, %lld): every cut has at least one track", (long long)c, (long long)t0, (long long)t1);
    if (nt > kFmMaxTracks) return fm_refuse(3, "cut %lld has %lld tracks, the feature-mix launch serves up to %d per cut", (long long)c, (long long)nt, kFmMaxTracks);
    const int32_t form = h_form[c];
    if (form != kFmCopy && form != kFmFold) return fm_refuse(1, "cut %lld: unknown form %d (0 copy, 1 fold)", (long long)c, (int)form);
    const int64_t T = h_num_frames[c], d0 = h_dst_first ? h_dst_first[c] : 0;
    if (T < 0 || d0 < 0 || T > row_frames || d0 > row_frames - T)
      return fm_refuse(1, "cut %lld: %lld frames at frame %lld do not fit a row of %lld", (long long)c, (long long)T, (long long)d0, (long long)row_frames);
    const int64_t ref = h_ref_track ? h_ref_track[c] : -1;
    if (ref < -1 || ref >= nt) return fm_refuse(1, "cut %lld: reference track %lld of %lld", (long long)c, (long long)ref, (long long)nt);
    const double pad_value = h_pad_value ? h_pad_value[c] : 0.0;
    if (form == kFmCopy && nt != 1) return fm_refuse(1, "cut %lld: the copy form takes one track (the padding is the cut's pad value), got %lld", (long long)c, (long long)nt);
    int64_t total = 0;
    bool any_snr = false;
    for (int64_t t = t0; t < t1; ++t) {
      const int64_t so = h_src_offset[t], n = h_frames[t], off = h_first ? h_first[t] : 0;
      const bool constant = so == -1;
      const int64_t rows = constant || !h_src_rows ? n : h_src_rows[t];
      const int32_t f16 = h_dtype ? h_dtype[t] : kFmF32;
      if (so < -1 || off < 0) return fm_refuse(1, "cut %lld, track %lld: negative offset (source %lld, in the cut %lld)", (long long)c, (long long)(t - t0), (long long)so, (long long)off);
      if (f16 != kFmF32 && f16 != kFmF16) return fm_refuse(1, "cut %lld, track %lld: unknown type %d (0 float32, 1 binary16)", (long long)c, (long long)(t - t0), (int)f16);
      if (n < 0 || n > max_frames || off > max_frames - n)
        return fm_refuse(1, "cut %lld, track %lld: %lld frames at frame %lld out of range", (long long)c, (long long)(t - t0), (long long)n, (long long)off);
      if (rows < n - 1 || rows > n + 1 || (n > 0 && rows < 1))  // (mono.py:61-64: one frame too many is dropped, one too few repeats the last)
        return fm_refuse(1, "cut %lld, track %lld: %lld stored rows for %lld frames (one more or one less at the most)", (long long)c, (long long)(t - t0), (long long)rows, (long long)n);
      if (!constant && (so & (f16 ? 1 : 3))) return fm_refuse(1, "cut %lld, track %lld: byte offset %lld is not aligned to the track's type", (long long)c, (long long)(t - t0), (long long)so);
      const int64_t read_bytes = std::min(rows, n) * F * (f16 ? 2 : 4);
      if (!constant && so > INT64_MAX - read_bytes) return fm_refuse(1, "cut %lld, track %lld: source %lld + %lld bytes overflows a 64-bit count", (long long)c, (long long)(t - t0), (long long)so, (long long)read_bytes);
      const double snr = h_snr_db ? h_snr_db[t] : NAN;
      // no SNR, no reference, or the first track being the reference itself (mixed.py:1255-1266): gain 1
      const bool scaled = form == kFmFold && !std::isnan(snr) && ref >= 0 && !(t == t0 && ref == 0);
      FmTrack tr{};
      tr.src_off = so;
      tr.frames = (int32_t)n;
      tr.rows = (int32_t)rows;
      tr.first = (int32_t)off;
      tr.f16 = f16;
      tr.part_first = 0;
      tr.part_count = scaled && !constant ? 1 : 0;  // (flag; counted below)
      tr.ratio = scaled ? std::pow(10.0, -snr / 10.0) : -1.0;
      tr.value = (float)(h_value ? h_value[t] : 0.0);
      tr.pad = 0;
      if (scaled && !(tr.ratio >= 0.0 && std::isfinite(tr.ratio))) return fm_refuse(1, "cut %lld, track %lld: SNR %g dB out of range", (long long)c, (long long)(t - t0), snr);
      any_snr |= scaled;
      tracks.push_back(tr);
      if (n > 0 || t == t0) total = std::max(total, off + n);  // (a later track of no frames is not mixed at all: mixer.py:116-117)
      if (!constant && n > 0) p.arena_need = std::max(p.arena_need, so + read_bytes);
    }
    if (any_snr && tracks[(size_t)(t0 + ref)].src_off >= 0) tracks[(size_t)(t0 + ref)].part_count = 1;
    for (int64_t t = t0; t < t1; ++t) {
      FmTrack& tr = tracks[(size_t)t];
      tr.part_first = (int32_t)parts;
      if (tr.part_count) tr.part_count = (int32_t)(((int64_t)tr.frames * F + kFmEnergyBlock - 1) / kFmEnergyBlock);
      parts += tr.part_count;
    }
    if (parts > INT32_MAX - (1 << 24)) return fm_refuse(1, "batch too large for one launch");
    if (form == kFmCopy) {
      if (tracks[(size_t)t0].first != 0) return fm_refuse(1, "cut %lld: the track of the copy form starts at frame 0", (long long)c);
      if (total > T) return fm_refuse(1, "cut %lld: a track of %lld frames does not fit a cut of %lld", (long long)c, (long long)total, (long long)T);
    } else if (total - T > 1 || total - T < -1 || (T > 0 && total < 1)) {  // (mixed.py:1294-1306)
      return fm_refuse(1, "cut %lld: the tracks mix to %lld frames, the cut has %lld (one more or one less at the most)", (long long)c, (long long)total, (long long)T);
    }
    FmCut& cd = p.cuts[(size_t)c];
    cd.track_first = (int32_t)t0;
    cd.track_count = (int32_t)nt;
    cd.form = form;
    cd.num_frames = (int32_t)T;
    cd.dst_first = (int32_t)d0;
    cd.mix_frames = (int32_t)total;
    cd.ref_track = ref >= 0 ? (int32_t)(t0 + ref) : -1;
    cd.pad_value = (float)pad_value;
  }
  p.num_features = F;
  p.row_frames = row_frames;
  p.row_len = row_frames * F;
  p.tiles_per_row = fm_tiles(p.row_len);
  p.out_need = num_cuts * p.row_len;
  p.energy_items = parts;
  p.fold_items = num_cuts * p.tiles_per_row;
  return p;
}

}  // namespace hipfeat
