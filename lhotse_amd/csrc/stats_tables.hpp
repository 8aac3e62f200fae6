// Host-side table of the global-statistics kernels (kernel_stats.hpp): what hipfeat_stats_update validates and builds, once per call.
// Pure C++ (no HIP): also compiled by tests/native/stats_tables_capi.cpp and checked on the CPU (tests/test_stats_host.py).
//
// Reference: CutSet.compute_global_feature_stats (lhotse/cut/set.py:2533-2583) feeds one feature matrix per cut to
// StatsAccumulator.update (lhotse/features/base.py:990-1033).
//
// The feature buffer is row-major with row_stride elements per row (row_stride >= F); cut b owns the rows
// [h_first_row[b], h_first_row[b] + h_num_frames[b]) (h_first_row == nullptr: the cuts are packed back to back from row 0).  A cut is
// read in BLOCKS of kStBlockFrames frames; block k of the update is row k of the slab of partial results, and the blocks of a cut are
// consecutive: [block_first, block_first + ceil(frames / kStBlockFrames)).  A cut of no frames has no block and contributes nothing.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace hipfeat {

constexpr int kStBlockFrames = 256;  // frames of one work item: kStRowLanes lanes x 16 frames each
constexpr int kStRowLanes = 16;      // lanes of a workgroup along the frames
constexpr int kStColLanes = 16;      // lanes along the bins; each owns 4 (float32) or 8 (binary16) bins: one 16-byte load per frame
constexpr int kStMaxCuts = 65535;    // cuts of one update
constexpr int kStMaxDim = 65535;     // bins

constexpr int32_t kStF32 = 0, kStF16 = 1;  // element types

struct StCut {
  int64_t first_elem;   // element index of the cut's first value: first_row * row_stride
  int32_t frames;
  int32_t block_first;  // exclusive prefix sum of the cuts' block counts
};
static_assert(sizeof(StCut) == 16, "descriptor size");

struct StPlan {
  int status = 0;       // 0 OK, 1 INVALID, 3 UNSUPPORTED (hipfeat_status)
  std::string message;  // of a refusal
  std::vector<StCut> cuts;
  int64_t feature_dim = 0, row_stride = 0, total_frames = 0, total_blocks = 0, col_tiles = 0, items = 0;
  int32_t dtype = 0, vec_ok = 0;  // vec_ok: base and stride keep every lane's group of 4 / 8 bins on a 16-byte boundary
};

#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline StPlan st_refuse(int status, const char* fmt, ...) {
  StPlan p;
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  p.status = status;
  p.message = buf;
  return p;
}

inline int64_t st_blocks(int64_t frames) { return (frames + kStBlockFrames - 1) / kStBlockFrames; }
inline int64_t st_tile_cols(int32_t dtype) { return kStColLanes * (dtype == kStF16 ? 8 : 4); }
inline int64_t st_col_tiles(int64_t F, int32_t dtype) { return (F + st_tile_cols(dtype) - 1) / st_tile_cols(dtype); }

// base: the address of element 0 of the buffer (only its alignment is looked at); feats_elems: elements the buffer holds
inline StPlan build_stats_plan(int64_t feature_dim, uint64_t base, int64_t feats_elems, int32_t dtype, int64_t num_cuts, const int64_t* h_first_row,
                               const int64_t* h_num_frames, int64_t row_stride) {
  if (feature_dim < 1 || feature_dim > kStMaxDim) return st_refuse(1, "%lld bins per frame (1 ... %d)", (long long)feature_dim, kStMaxDim);
  if (dtype != kStF32 && dtype != kStF16) return st_refuse(1, "unknown element type %d (0 float32, 1 binary16)", (int)dtype);
  if (num_cuts < 1 || num_cuts > kStMaxCuts) return st_refuse(1, "bad batch arguments (1 ... %d cuts)", kStMaxCuts);
  if (!h_num_frames) return st_refuse(1, "NULL argument");
  if (feats_elems < 0) return st_refuse(1, "a buffer of %lld elements", (long long)feats_elems);
  const int64_t F = feature_dim, esize = dtype == kStF16 ? 2 : 4;
  if (row_stride < F) return st_refuse(1, "a row stride of %lld elements is shorter than a frame of %lld bins", (long long)row_stride, (long long)F);
  // (the stride counts elements, so rows keep the alignment of the base; a byte stride would have to be checked here as well)
  if (base % (uint64_t)esize) return st_refuse(1, "the feature buffer is not aligned to its element size (%lld bytes)", (long long)esize);
  StPlan p;
  p.cuts.resize((size_t)num_cuts);
  int64_t next_row = 0, blocks = 0, frames = 0;
  for (int64_t b = 0; b < num_cuts; ++b) {
    const int64_t T = h_num_frames[b], r0 = h_first_row ? h_first_row[b] : next_row;
    if (T < 0 || r0 < 0) return st_refuse(1, "cut %lld: negative rows (first row %lld, %lld frames)", (long long)b, (long long)r0, (long long)T);
    if (T > INT32_MAX / 2) return st_refuse(1, "cut %lld: %lld frames out of range", (long long)b, (long long)T);
    // the cut's last element is (r0 + T - 1) * row_stride + F - 1: it lies inside the buffer, and nothing overflows on the way
    if (T > 0) {
      const int64_t rows_fit = feats_elems >= F ? (feats_elems - F) / row_stride + 1 : 0;  // rows r with r * row_stride + F <= feats_elems
      if (r0 > rows_fit || T > rows_fit - r0)
        return st_refuse(1, "cut %lld: rows [%lld, %lld) reach beyond a buffer of %lld elements (row stride %lld)", (long long)b, (long long)r0, (long long)(r0 + T),
                         (long long)feats_elems, (long long)row_stride);
    } else if (r0 > INT64_MAX / row_stride) {
      return st_refuse(1, "cut %lld: first row %lld out of range", (long long)b, (long long)r0);
    }
    p.cuts[(size_t)b] = StCut{r0 * row_stride, (int32_t)T, (int32_t)blocks};
    blocks += st_blocks(T);
    frames += T;
    next_row = r0 + T;
    if (blocks > (1 << 24)) return st_refuse(3, "more than 2^24 blocks of %d frames in one update: split it", kStBlockFrames);
  }
  p.feature_dim = F;
  p.row_stride = row_stride;
  p.dtype = dtype;
  p.total_frames = frames;
  p.total_blocks = blocks;
  p.col_tiles = st_col_tiles(F, dtype);
  p.items = blocks * p.col_tiles;
  p.vec_ok = (base % 16 == 0 && (row_stride * esize) % 16 == 0) ? 1 : 0;
  if (p.items > INT32_MAX - (1 << 24)) return st_refuse(3, "update too large for one launch (%lld work items): split it", (long long)p.items);
  return p;
}

}  // namespace hipfeat
