// Host-side table of the collate kernel (kernel_collate.hpp): what hipfeat_collate_plan validates and builds, once per plan.
// Pure C++ (no HIP): also compiled by tests/native/collate_tables_capi.cpp and checked on the CPU (tests/test_collate_abi.py); the sources
// form further down by tests/native/collate_sources_capi.cpp (tests/test_collate_sources_abi.py).
//
// Reference: collate_audio (lhotse/dataset/collation.py:148-260) pads every cut of a mini-batch to the longest one and stacks them
// with collate_vectors(..., padding_value=0.0): row r of a dense (rows, row_len) tensor holds the cut's samples and zeros elsewhere.
// Here ROW r receives the `len` float32 samples at arena + src_off, starting at element dst_off of the row (0: right padding,
// row_len - len: left padding); every other element of the row is +0.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "ticket_slots.hpp"

namespace hipfeat {

constexpr int kCoTile = 4096;  // output elements per work item (256 lanes x 16-byte stores: 4 rounds of float32, 2 of the 2-byte types)

constexpr int32_t kCoF32 = 0, kCoF16 = 1, kCoBF16 = 2;  // output types

struct CoRow {
  int64_t src_off;  // arena offset of the row's samples
  int64_t dst_off;  // element of the row that receives the first sample
  int64_t len;      // samples (0: a row of padding only)
  int64_t pad;
};
static_assert(sizeof(CoRow) == 32, "descriptor size");

inline int co_elem_bytes(int32_t out_type) { return out_type == kCoF32 ? 4 : 2; }
inline int co_vec(int32_t out_type) { return 16 / co_elem_bytes(out_type); }  // elements of one 16-byte store

// work items of a row: tiles of kCoTile elements counted from the 16-byte boundary at or below the row's first element, which lies at
// most (vec - 1) elements in front of it (rows start at r * row_len: every row has its own alignment)
inline int64_t co_tiles(int64_t row_len, int32_t out_type) { return row_len == 0 ? 0 : (row_len - 1 + co_vec(out_type) - 1) / kCoTile + 1; }

struct CoPlan {
  int status = 0;       // 0 OK, 1 INVALID, 3 UNSUPPORTED (hipfeat_status)
  std::string message;  // of a refusal
  std::vector<CoRow> rows;
  int64_t row_len = 0, tiles_per_row = 0, work_items = 0, arena_need = 0, out_need = 0;
  int32_t out_type = 0;
  // the sources form (build_collate_sources_plan): row r reads srcs[first .. first + k), first and k packed in rows[r].pad
  bool sources = false;
  std::vector<int64_t> srcs;
};

inline CoPlan co_refuse(const char* fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
  CoPlan p;
  char buf[256];
  std::snprintf(buf, sizeof(buf), fmt, a, b, c, d);
  p.status = 1;
  p.message = buf;
  return p;
}

// h_dst_offset == nullptr: 0 for every row (right padding)
inline CoPlan build_collate_plan(int64_t num_rows, const int64_t* h_src_offset, const int64_t* h_src_len, const int64_t* h_dst_offset, int64_t row_len,
                                 int32_t out_type) {
  if (out_type != kCoF32 && out_type != kCoF16 && out_type != kCoBF16) return co_refuse("unknown output type %lld (0 float32, 1 binary16, 2 bfloat16)", out_type);
  if (num_rows < 0) return co_refuse("%lld rows", num_rows);
  if (row_len < 0) return co_refuse("a row of %lld elements", row_len);
  if (num_rows > 0 && (!h_src_offset || !h_src_len)) return co_refuse("NULL argument");
  if (row_len > 0 && num_rows > INT64_MAX / row_len) return co_refuse("%lld rows of %lld elements overflow a 64-bit count", num_rows, row_len);
  CoPlan p;
  p.rows.resize((size_t)num_rows);
  for (int64_t i = 0; i < num_rows; ++i) {
    const int64_t so = h_src_offset[i], n = h_src_len[i], d = h_dst_offset ? h_dst_offset[i] : 0;
    if (so < 0 || d < 0) return co_refuse("row %lld: negative offset (source %lld, destination %lld)", i, so, d);
    if (n < 0) return co_refuse("row %lld: %lld samples", i, n);
    if (so > INT64_MAX - n) return co_refuse("row %lld: source %lld + %lld overflows a 64-bit count", i, so, n);
    if (n > row_len || d > row_len - n) return co_refuse("row %lld: %lld samples at element %lld do not fit a row of %lld", i, n, d, row_len);
    CoRow& r = p.rows[(size_t)i];
    r.src_off = so;
    r.dst_off = d;
    r.len = n;
    r.pad = 0;
    if (n > 0) p.arena_need = std::max(p.arena_need, so + n);  // (a row of padding reads nothing: its source offset does not count)
  }
  p.row_len = row_len;
  p.out_type = out_type;
  p.out_need = num_rows * row_len;
  p.tiles_per_row = co_tiles(row_len, out_type);
  p.work_items = num_rows * p.tiles_per_row;  // (<= rows * row_len, or rows where a row is shorter than a tile: fits)
  return p;
}

// ---- the sources form: a row is the mean of k >= 0 equally long runs of the arena (collate_mean_kernel) --------------------------------
// Reference: collate_audio's channel handling (lhotse/dataset/collation.py:215-241): a multi-channel cut is either downmixed to mono by
// the mean over its channels, row (B, T), or kept as (B, C, T) with all-zero rows for the channels a cut does not have.  Row r has
// k_r = h_first[r + 1] - h_first[r] sources, each of h_src_len[r] samples, source c at arena + h_src_offset[h_first[r] + c]:
//   k = 0: the row is +0 everywhere;  k = 1: the row of build_collate_plan (float32: a bit copy);
//   k >= 2: element i = float32((0.0 + double(x_0[i]) + double(x_1[i]) + ... + double(x_{k-1}[i])) / double(k)), the sum in ascending
//   source order in float64, one float64 division, one rounding to nearest even -- then the conversion of a float32 sample to the output type.
constexpr int kCoMaxSources = 32;  // sources of one row
constexpr int kCoSourceBits = 6;   // CoRow.pad = first << kCoSourceBits | k
static_assert(kCoMaxSources < (1 << kCoSourceBits), "the count fits its field");

constexpr int64_t co_pack_sources(int64_t first, int64_t k) { return (first << kCoSourceBits) | k; }
constexpr int64_t co_first_source(int64_t pad) { return pad >> kCoSourceBits; }
constexpr int co_num_sources(int64_t pad) { return (int)(pad & ((1 << kCoSourceBits) - 1)); }

// h_dst_offset == nullptr: 0 for every row (right padding).  status 3 (UNSUPPORTED): a row of more than kCoMaxSources sources
inline CoPlan build_collate_sources_plan(int64_t num_rows, const int64_t* h_first, const int64_t* h_src_offset, const int64_t* h_src_len,
                                         const int64_t* h_dst_offset, int64_t row_len, int32_t out_type) {
  if (out_type != kCoF32 && out_type != kCoF16 && out_type != kCoBF16) return co_refuse("unknown output type %lld (0 float32, 1 binary16, 2 bfloat16)", out_type);
  if (num_rows < 0) return co_refuse("%lld rows", num_rows);
  if (row_len < 0) return co_refuse("a row of %lld elements", row_len);
  if (!h_first || (num_rows > 0 && !h_src_len)) return co_refuse("NULL argument");
  if (h_first[0] != 0) return co_refuse("the sources of row 0 start at %lld, not at 0", h_first[0]);
  if (row_len > 0 && num_rows > INT64_MAX / row_len) return co_refuse("%lld rows of %lld elements overflow a 64-bit count", num_rows, row_len);
  for (int64_t i = 0; i < num_rows; ++i)
    if (h_first[i + 1] < h_first[i]) return co_refuse("row %lld: its sources end at %lld, in front of their start %lld", i, h_first[i + 1], h_first[i]);
  const int64_t num_srcs = h_first[num_rows];
  if (num_srcs > 0 && !h_src_offset) return co_refuse("NULL argument");
  if (num_srcs > (INT64_MAX >> kCoSourceBits)) return co_refuse("%lld sources", num_srcs);
  CoPlan p;
  p.sources = true;
  p.rows.resize((size_t)num_rows);
  p.srcs.assign(h_src_offset, h_src_offset + num_srcs);
  for (int64_t i = 0; i < num_rows; ++i) {
    const int64_t first = h_first[i], k = h_first[i + 1] - first, n = h_src_len[i], d = h_dst_offset ? h_dst_offset[i] : 0;
    if (d < 0) return co_refuse("row %lld: negative destination offset %lld", i, d);
    if (n < 0) return co_refuse("row %lld: %lld samples", i, n);
    if (n > row_len || d > row_len - n) return co_refuse("row %lld: %lld samples at element %lld do not fit a row of %lld", i, n, d, row_len);
    for (int64_t c = 0; c < k; ++c) {
      const int64_t so = p.srcs[(size_t)(first + c)];
      if (so < 0) return co_refuse("row %lld: source %lld has the negative offset %lld", i, c, so);
      if (so > INT64_MAX - n) return co_refuse("row %lld: source %lld + %lld overflows a 64-bit count", i, so, n);
      if (n > 0) p.arena_need = std::max(p.arena_need, so + n);  // (a row of no samples reads nothing: its sources do not count)
    }
    if (k > kCoMaxSources) {
      CoPlan u = co_refuse("row %lld has %lld sources, a row takes at most %lld", i, k, kCoMaxSources);
      u.status = 3;
      return u;
    }
    CoRow& r = p.rows[(size_t)i];
    r.src_off = k > 0 ? p.srcs[(size_t)first] : 0;
    r.dst_off = d;
    r.len = k > 0 ? n : 0;  // (a row without sources is a row of padding)
    r.pad = co_pack_sources(first, k);
  }
  p.row_len = row_len;
  p.out_type = out_type;
  p.out_need = num_rows * row_len;
  p.tiles_per_row = co_tiles(row_len, out_type);
  p.work_items = num_rows * p.tiles_per_row;
  return p;
}

// The tickets of hipfeat_collate are the ring every ticketed handle shares (ticket_slots.hpp); its names from before the ring was shared
using CoSlots = TicketRing;
constexpr int kCoSlots = 16;
static_assert(kCoSlots == kTicketSlots, "one ring");

}  // namespace hipfeat
