// Host-side table of the reverb kernels (kernel_reverb.hpp): what hipfeat_reverb_plan validates and builds, once per plan.
// Pure C++ (no HIP): also compiled by tests/native/reverb_tables_capi.cpp and checked on the CPU (tests/test_reverb_abi.py).
//
// An ITEM is one (input channel, RIR channel) pair: n float32 samples at arena + src_offset, convolved with the `taps` scaled taps at
// arena + rir_offset, the n outputs from `shift` on kept.  The outputs are written from tail_start on, each on a 16-byte boundary.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace hipfeat {

constexpr int kRvLane = 8;                     // consecutive outputs per lane
constexpr int kRvBlock = 256 * kRvLane;        // outputs per work item
constexpr int kRvChunk = 256;                  // taps per partial sum
constexpr int kRvWindow = kRvBlock + kRvChunk; // floats of x in LDS per chunk (the last one is never used)

struct RvItem {
  int64_t src_off;     // arena offset of the input channel
  int64_t rir_off;     // arena offset of the scaled RIR
  int64_t out_off;     // arena offset of the output (16-byte aligned)
  int32_t n;           // samples in = samples out
  int32_t taps;        // L
  int32_t shift;       // first index of max(hs)
  int32_t item_first;  // exclusive prefix sum of the items' work items
  int32_t normalize;
  int32_t pad;
};
static_assert(sizeof(RvItem) == 48, "descriptor size");

struct RvPlan {
  int status = 0;       // 0 OK, 1 INVALID (hipfeat_status)
  std::string message;  // of a refusal
  std::vector<RvItem> items;
  int64_t work_items = 0, arena_need = 0;
};

inline RvPlan rv_refuse(const char* fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0, long long e = 0, long long f = 0) {
  RvPlan p;
  char buf[256];
  std::snprintf(buf, sizeof(buf), fmt, a, b, c, d, e, f);
  p.status = 1;
  p.message = buf;
  return p;
}

// h_normalize may be nullptr (no item is normalised)
inline RvPlan build_reverb_plan(int64_t num_items, const int64_t* h_src_offset, const int64_t* h_src_len, const int64_t* h_rir_offset, const int64_t* h_rir_len,
                                const int64_t* h_shift, const int32_t* h_normalize, int64_t tail_start) {
  if (!h_src_offset || !h_src_len || !h_rir_offset || !h_rir_len || !h_shift) return rv_refuse("NULL argument");
  if (num_items <= 0 || num_items > 65535) return rv_refuse("bad batch arguments (1 ... 65535 items)");
  if (tail_start < 0) return rv_refuse("tail_start %lld is negative", tail_start);
  constexpr int64_t kMaxLen = INT32_MAX / 2;
  RvPlan p;
  p.items.resize((size_t)num_items);
  int64_t tail = (tail_start + 3) & ~(int64_t)3, work = 0;
  for (int64_t i = 0; i < num_items; ++i) {
    const int64_t so = h_src_offset[i], n = h_src_len[i], ro = h_rir_offset[i], taps = h_rir_len[i], shift = h_shift[i];
    if (so < 0 || ro < 0) return rv_refuse("item %lld: negative offset (source %lld, impulse response %lld)", i, so, ro);
    if (n < 1 || n > kMaxLen || taps < 1 || taps > kMaxLen) return rv_refuse("item %lld: %lld samples, %lld taps: both must be 1 ... %lld", i, n, taps, kMaxLen);
    if (shift < 0 || shift >= taps) return rv_refuse("item %lld: shift %lld outside [0, %lld)", i, shift, taps);
    if (so + n > tail_start || ro + taps > tail_start)  // the outputs are written from tail_start on: output and source ranges would overlap
      return rv_refuse("item %lld (source %lld + %lld, impulse response %lld + %lld) reaches into the arena's tail (tail_start %lld), where the outputs are written", i, so,
                       n, ro, taps, tail_start);
    RvItem& it = p.items[(size_t)i];
    it.src_off = so;
    it.rir_off = ro;
    it.out_off = tail;
    it.n = (int32_t)n;
    it.taps = (int32_t)taps;
    it.shift = (int32_t)shift;
    it.item_first = (int32_t)work;
    it.normalize = (h_normalize && h_normalize[i]) ? 1 : 0;
    it.pad = 0;
    work += (n + kRvBlock - 1) / kRvBlock;
    tail += (n + 3) & ~(int64_t)3;
    if (work > INT32_MAX - (1 << 24)) return rv_refuse("batch too large for one launch");
  }
  p.work_items = work;
  p.arena_need = tail;
  return p;
}

}  // namespace hipfeat
