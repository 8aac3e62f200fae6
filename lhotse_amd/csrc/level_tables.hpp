// Host-side table of the level kernels (kernel_level.hpp): what hipfeat_level_plan validates and builds, once per plan.
// Pure C++ (no HIP): also compiled by tests/native/level_tables_capi.cpp and checked on the CPU (tests/test_level_abi.py).
//
// An ITEM is a run of `len` float32 samples of the arena with a PROGRAM of 1 ... 4 ops that every sample goes through in order:
//   SCALE f                                Volume.__call__ (lhotse/augmentation/torchaudio.py:395-406):  y = x * (float)f
//   CLIP hard | soft, g, normalize, gain   Clipping.__call__ (lhotse/augmentation/clipping.py:28-61), p = max |x| of the op's input over the item:
//       p == 0 or p < kLvSilencePeak: y = x;  else, float32, in this order:  [x / p]  [* g]  clamp(., -1, 1) | tanh  [/ g]  [* p]
// The result is written at dst_offset; dst_offset == src_offset is in-place operation.  Nothing else may overlap: an item's destination
// with its own source in part, with another item's source, or with another item's destination.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace hipfeat {

constexpr int kLvBlock = 4096;  // samples per work item of both launches (256 lanes x 4 x float4)
constexpr int kLvMaxOps = 4;

constexpr int32_t kLvScale = 0, kLvClip = 1;                       // op kinds
constexpr int32_t kLvHard = 1, kLvNormalize = 2, kLvUseGain = 4;   // CLIP flags

// clipping.py:36 treats a peak with `20 * np.log10(p) < -96` (float32) as silence.  That is p < 0x1.09e69ep-16 (1.5848926e-05): the
// smallest float32 for which the expression is False; tests/test_level_reference.py walks the floats on both sides of it.
constexpr float kLvSilencePeak = 0x1.09e69ep-16f;

struct LvItem {
  int64_t src_off;     // arena offset of the item's samples
  int64_t dst_off;     // arena offset of the result (== src_off: in place)
  int32_t len;         // samples
  int32_t item_first;  // exclusive prefix sum of the items' work items = index of the item's first partial peak
  int32_t nops;        // 1 ... kLvMaxOps
  int32_t clip_at;     // index of the program's CLIP, -1: none (the peak launch skips the item)
  int32_t op[kLvMaxOps];   // kind | flags << 8
  float value[kLvMaxOps];  // SCALE: the factor; CLIP: the linear gain g
};
static_assert(sizeof(LvItem) == 64, "descriptor size");

// work items of an item: tiles of kLvBlock samples counted from the 16-byte boundary at or below its source
inline int64_t lv_blocks(int64_t src_off, int64_t len) { return ((src_off & 3) + len + kLvBlock - 1) / kLvBlock; }

struct LvPlan {
  int status = 0;       // 0 OK, 1 INVALID, 3 UNSUPPORTED (hipfeat_status)
  std::string message;  // of a refusal
  std::vector<LvItem> items;
  int64_t work_items = 0, peak_items = 0, arena_need = 0;
};

inline LvPlan lv_refuse(int status, const char* fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
  LvPlan p;
  char buf[256];
  std::snprintf(buf, sizeof(buf), fmt, a, b, c, d);
  p.status = status;
  p.message = buf;
  return p;
}

// h_op_first[num_items + 1]: the ops of item i are [h_op_first[i], h_op_first[i + 1]) of the three op tables
inline LvPlan build_level_plan(int64_t num_items, const int64_t* h_src_offset, const int64_t* h_src_len, const int64_t* h_dst_offset, const int64_t* h_op_first,
                               const int32_t* h_op_kind, const float* h_op_value, const int32_t* h_op_flags) {
  constexpr int64_t kMaxLen = INT32_MAX / 2;
  if (num_items < 0 || num_items > 65535) return lv_refuse(1, "bad batch arguments (0 ... 65535 items)");
  if (num_items > 0 && (!h_src_offset || !h_src_len || !h_dst_offset || !h_op_first || !h_op_kind || !h_op_value || !h_op_flags)) return lv_refuse(1, "NULL argument");
  LvPlan p;
  p.items.resize((size_t)num_items);
  if (num_items > 0 && h_op_first[0] != 0) return lv_refuse(1, "h_op_first[0] is %lld, not 0", (long long)h_op_first[0]);
  for (int64_t i = 0; i < num_items; ++i) {
    const int64_t so = h_src_offset[i], n = h_src_len[i], d = h_dst_offset[i], nops = h_op_first[i + 1] - h_op_first[i];
    if (so < 0 || d < 0) return lv_refuse(1, "item %lld: negative offset (source %lld, destination %lld)", i, so, d);
    if (n < 1 || n > kMaxLen) return lv_refuse(1, "item %lld: %lld samples, must be 1 ... %lld", i, n, kMaxLen);  // (np.max of nothing raises in the reference)
    if (nops < 1 || nops > kLvMaxOps) return lv_refuse(1, "item %lld: a program of %lld ops, must be 1 ... %lld", i, nops, kLvMaxOps);
    if (d != so && d < so + n && so < d + n) return lv_refuse(1, "item %lld: destination %lld overlaps its source %lld + %lld in part", i, d, so, n);
    LvItem& it = p.items[(size_t)i];
    it.src_off = so;
    it.dst_off = d;
    it.len = (int32_t)n;
    it.item_first = (int32_t)p.work_items;
    it.nops = (int32_t)nops;
    it.clip_at = -1;
    for (int k = 0; k < kLvMaxOps; ++k) it.op[k] = 0, it.value[k] = 0.0f;
    for (int k = 0; k < (int)nops; ++k) {
      const int64_t at = h_op_first[i] + k;
      const int32_t kind = h_op_kind[at], flags = h_op_flags[at];
      const float v = h_op_value[at];
      if (kind == kLvClip) {
        if (it.clip_at >= 0) return lv_refuse(3, "item %lld: more than one CLIP in a program", i);
        if (flags & ~(kLvHard | kLvNormalize | kLvUseGain)) return lv_refuse(1, "item %lld, op %lld: unknown CLIP flags %lld", i, k, flags);
        if ((flags & kLvUseGain) && !(v > 0.0f && std::isfinite(v))) return lv_refuse(1, "item %lld, op %lld: the linear gain must be positive and finite", i, k);
        it.clip_at = k;
      } else if (kind != kLvScale) {
        return lv_refuse(1, "item %lld, op %lld: unknown op kind %lld", i, k, kind);
      } else if (flags != 0) {
        return lv_refuse(1, "item %lld, op %lld: SCALE takes no flags (%lld)", i, k, flags);
      }
      it.op[k] = kind | (flags << 8);
      it.value[k] = v;
    }
    const int64_t blocks = lv_blocks(so, n);
    p.work_items += blocks;
    if (it.clip_at >= 0) p.peak_items += blocks;
    p.arena_need = std::max(p.arena_need, std::max(so, d) + n);
    if (p.work_items > INT32_MAX - (1 << 24)) return lv_refuse(1, "batch too large for one launch");
  }
  // across items: destinations are disjoint, and a destination meets a source only as the same item's in-place range
  std::vector<int64_t> order((size_t)num_items);
  for (int64_t i = 0; i < num_items; ++i) order[(size_t)i] = i;
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return p.items[(size_t)a].dst_off < p.items[(size_t)b].dst_off; });
  for (int64_t k = 1; k < num_items; ++k) {
    const LvItem &a = p.items[(size_t)order[(size_t)k - 1]], &b = p.items[(size_t)order[(size_t)k]];
    if (a.dst_off + a.len > b.dst_off) return lv_refuse(1, "items %lld and %lld: their destinations overlap", order[(size_t)k - 1], order[(size_t)k]);
  }
  for (int64_t i = 0; i < num_items; ++i) {
    const LvItem& it = p.items[(size_t)i];
    // the first destination that ends behind the source's start (destinations are disjoint and sorted: their ends ascend too)
    auto lo = std::partition_point(order.begin(), order.end(), [&](int64_t j) { return p.items[(size_t)j].dst_off + p.items[(size_t)j].len <= it.src_off; });
    for (; lo != order.end() && p.items[(size_t)*lo].dst_off < it.src_off + it.len; ++lo)
      if (*lo != i || it.dst_off != it.src_off) return lv_refuse(1, "item %lld: its source overlaps the destination of item %lld", i, *lo);
  }
  return p;
}

}  // namespace hipfeat
