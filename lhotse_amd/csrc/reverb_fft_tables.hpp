// Host-side tables of the partitioned-FFT reverb launches (kernel_reverb_fft.hpp): what hipfeat_reverb_plan_method validates and builds,
// once per plan.  Pure C++ (no HIP): also compiled by tests/native/reverb_fft_tables_capi.cpp and checked on the CPU
// (tests/test_reverb_fft_abi.py).
//
// Geometry (uniformly partitioned overlap-save).  Block B = kRfBlock = 1024 samples, transform size 2 B = 2048.  For an item with N
// samples, L taps and shift s, with yf[m] = sum_k hs[k] x[m - k] the full convolution and y[n] = yf[n + s], 0 <= n < N, what is kept:
//   partitions     P  = ceil(L / B):  h_p = hs[p B, (p + 1) B), zero-padded to 2048            -> spectrum H_p
//   input blocks   nx = min(j1, floor((N - 1) / B) + 1) + 1:  block i = x[(i - 1) B, (i + 1) B), zero outside [0, N)  -> spectrum X_i,
//                  i = 0 ... nx - 1 (these are all the blocks that hold a sample of x and that an output block of the item reads)
//   output blocks  j  = j0 ... j1,  j0 = floor(s / B),  j1 = floor((s + N - 1) / B),  ny = j1 - j0 + 1:
//                  Y_j = sum_p H_p X_{j - p} over the p with 0 <= p < P and 0 <= j - p < nx, p ASCENDING; the upper 1024 samples of the
//                  inverse transform of Y_j are yf[j B, (j + 1) B); the part inside [s, s + N) is stored
// A spectrum is 1024 complex floats (bins 0 ... 1023, the real Nyquist bin packed into the imaginary part of bin 0) = kRfSpecFloats =
// 2048 floats = 8 KB.  WORKSPACE FORMULA: the spectra lie in the arena behind the outputs, from the first 16-byte boundary at or behind
// the last output on:
//   workspace floats = 2048 * (sum over the DISTINCT (rir_offset, rir_len) of the ticket's FFT items of P  +  sum over its FFT items of nx)
// first the RIR spectra (distinct RIRs in order of first use, partitions ascending), then every FFT item's input spectra (items in
// order, blocks ascending).  Items of the direct form add nothing.
//
// Work items.  Launch A (spectra): one WAVE per transform -- the RIR partitions first, then the input blocks.  Launch B (accumulate and
// invert): one wave per output block.  Gain: one workgroup per kRvBlock (2048) outputs, as the direct form's.  Partial sums of squares
// (float64): [x_total] one per input block (its NEW samples x[i B, (i + 1) B)), then [b_work] one per output block (what it stored).
#pragma once
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "reverb_tables.hpp"

namespace hipfeat {

constexpr int kRfBlock = 1024;              // B: new samples per transform
constexpr int kRfSpecFloats = 2 * kRfBlock; // floats of one spectrum (1024 complex, Nyquist beside DC)
constexpr int kRfWaves = 4;                 // transforms per workgroup trip (one per wave)
constexpr int kRfGridSlots = 1792;          // workgroups of launches A and B at the most (items_grid)

enum : int32_t { kRvDirect = 0, kRvFft = 1, kRvAuto = 2 };

struct RfRir {           // one distinct scaled RIR of a ticket's FFT items
  int64_t rir_off;       // arena offset of the taps
  int64_t spec_off;      // arena offset of H_0 (16-byte aligned)
  int32_t taps, parts;   // L, P
  int32_t first;         // exclusive prefix sum of the RIRs' partitions = launch A work item of H_0
  int32_t pad;
};
static_assert(sizeof(RfRir) == 32, "descriptor size");

struct RfItem {
  int64_t src_off;       // arena offset of the input channel
  int64_t out_off;       // arena offset of the output (16-byte aligned)
  int64_t hspec_off;     // arena offset of its RIR's H_0
  int64_t xspec_off;     // arena offset of X_0
  int32_t n, taps, shift, parts;
  int32_t nx, j0, ny, normalize;
  int32_t a_first;       // launch A work item of X_0 (the RIR partitions of the ticket come first)
  int32_t b_first;       // launch B work item of Y_j0 = exclusive prefix sum of ny
  int32_t g_first;       // gain work item of output 0 = exclusive prefix sum of ceil(n / kRvBlock)
  int32_t pad;
};
static_assert(sizeof(RfItem) == 80, "descriptor size");

struct RfPlan {
  std::vector<RfItem> items;
  std::vector<RfRir> rirs;
  int64_t rir_work = 0, x_total = 0, a_work = 0, b_work = 0, g_work = 0;
};

struct RvMethodPlan : RvPlan {  // items: the direct-form items of the ticket (their own prefix sums); fft: the others
  RfPlan fft;
  std::vector<int64_t> out_offsets;  // of all items, in the caller's order
  int64_t fft_partials() const { return fft.x_total + fft.b_work; }
};

inline RvMethodPlan rf_refuse(const RvPlan& r) {
  RvMethodPlan p;
  p.status = r.status ? r.status : 1;
  p.message = r.message;
  return p;
}

// method: kRvDirect | kRvFft | kRvAuto (an item takes the FFT route when its rir_len >= min_fft_taps).  With no FFT item the result is
// build_reverb_plan's, to the byte.
inline RvMethodPlan build_reverb_plan_method(int64_t num_items, const int64_t* h_src_offset, const int64_t* h_src_len, const int64_t* h_rir_offset,
                                             const int64_t* h_rir_len, const int64_t* h_shift, const int32_t* h_normalize, int64_t tail_start, int32_t method,
                                             int64_t min_fft_taps) {
  if (method != kRvDirect && method != kRvFft && method != kRvAuto) return rf_refuse(rv_refuse("method %lld is not 0 (direct), 1 (fft) or 2 (auto)", method));
  if (min_fft_taps < 0) return rf_refuse(rv_refuse("min_fft_taps %lld is negative", min_fft_taps));
  RvPlan all = build_reverb_plan(num_items, h_src_offset, h_src_len, h_rir_offset, h_rir_len, h_shift, h_normalize, tail_start);
  if (all.status != 0) return rf_refuse(all);
  RvMethodPlan p;
  p.out_offsets.resize((size_t)num_items);
  for (int64_t i = 0; i < num_items; ++i) p.out_offsets[(size_t)i] = all.items[(size_t)i].out_off;
  std::vector<char> fft((size_t)num_items);
  bool any = false;
  for (int64_t i = 0; i < num_items; ++i) any |= (fft[(size_t)i] = method == kRvFft || (method == kRvAuto && h_rir_len[i] >= min_fft_taps)) != 0;
  if (!any) {
    static_cast<RvPlan&>(p) = std::move(all);
    return p;
  }
  // the direct items keep their outputs and get prefix sums of their own
  int64_t work = 0;
  for (int64_t i = 0; i < num_items; ++i) {
    if (fft[(size_t)i]) continue;
    RvItem it = all.items[(size_t)i];
    it.item_first = (int32_t)work;
    work += (it.n + kRvBlock - 1) / kRvBlock;
    p.items.push_back(it);
  }
  p.work_items = work;
  // the FFT items: distinct RIRs in order of first use, then the items
  RfPlan& f = p.fft;
  const int64_t ws = (all.arena_need + 3) & ~(int64_t)3;
  constexpr int64_t kMaxWork = INT32_MAX - (1 << 24);
  std::map<std::pair<int64_t, int64_t>, size_t> seen;
  std::vector<size_t> rir_of((size_t)num_items, 0);
  for (int64_t i = 0; i < num_items; ++i) {
    if (!fft[(size_t)i]) continue;
    const std::pair<int64_t, int64_t> key(h_rir_offset[i], h_rir_len[i]);
    auto at = seen.find(key);
    if (at == seen.end()) {
      const int64_t parts = (key.second + kRfBlock - 1) / kRfBlock;
      f.rirs.push_back(RfRir{key.first, ws + f.rir_work * kRfSpecFloats, (int32_t)key.second, (int32_t)parts, (int32_t)f.rir_work, 0});
      f.rir_work += parts;
      at = seen.emplace(key, f.rirs.size() - 1).first;
      if (f.rir_work > kMaxWork) return rf_refuse(rv_refuse("batch too large for one launch"));
    }
    rir_of[(size_t)i] = at->second;
  }
  for (int64_t i = 0; i < num_items; ++i) {
    if (!fft[(size_t)i]) continue;
    const RvItem& d = all.items[(size_t)i];
    const RfRir& r = f.rirs[rir_of[(size_t)i]];
    const int64_t n = d.n, s = d.shift;
    const int64_t j0 = s / kRfBlock, j1 = (s + n - 1) / kRfBlock;
    const int64_t last_x = (n - 1) / kRfBlock + 1;  // the last block that holds a sample of x
    const int64_t nx = (j1 < last_x ? j1 : last_x) + 1;
    RfItem it;
    it.src_off = d.src_off;
    it.out_off = d.out_off;
    it.hspec_off = r.spec_off;
    it.xspec_off = ws + (f.rir_work + f.x_total) * kRfSpecFloats;
    it.n = d.n, it.taps = d.taps, it.shift = d.shift, it.parts = r.parts;
    it.nx = (int32_t)nx, it.j0 = (int32_t)j0, it.ny = (int32_t)(j1 - j0 + 1), it.normalize = d.normalize;
    it.a_first = (int32_t)(f.rir_work + f.x_total);
    it.b_first = (int32_t)f.b_work;
    it.g_first = (int32_t)f.g_work;
    it.pad = 0;
    f.items.push_back(it);
    f.x_total += nx;
    f.b_work += j1 - j0 + 1;
    f.g_work += (n + kRvBlock - 1) / kRvBlock;
    if (f.rir_work + f.x_total > kMaxWork || f.b_work > kMaxWork) return rf_refuse(rv_refuse("batch too large for one launch"));
  }
  f.a_work = f.rir_work + f.x_total;
  p.arena_need = ws + f.a_work * kRfSpecFloats;
  return p;
}

}  // namespace hipfeat
