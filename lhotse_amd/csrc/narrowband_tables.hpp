// Host side of narrowband_kernel (kernel_narrowband.hpp): for a source rate, the geometry, weights and first taps of the two resamplers
// of Narrowband(codec="mulaw") (rate -> 8000 and 8000 -> rate; lhotse/augmentation/torchaudio.py:337-378), the tile geometry, the LDS
// map and the blob the kernel copies into LDS as it is.  Pure C++ (no HIP): hipfeat_narrowband_tables / _geometry hand it to the CPU
// tests.  The weight formula, the window and the length rule are sinc_tables.hpp's (sinc_weight, sinc_first_tap, sinc_out_len): they
// are not stated again.
//
// Per filter (orig : new reduced, W = 2 width + 2 taps per phase; the up filter always has width 7, W = 16):
//   w[new][W], first[new]         what sinc_tables.hpp gives: tap d of phase ph is the reference's kernel[ph][first[ph] + d]
//   start[p] = (p / new) * orig + first[p % new] - width, p < np
//                                 the input sample under tap 0 of output p (outputs counted from a multiple of `new`); ascending in p
//   wt[W][np], wt[d][p] = w[p % new][d]
//                                 the LDS form: tap-major, phases continued periodically up to np = roundup(new + 64 K - 1, 64) so that
//                                 a wave whose lanes own K consecutive outputs each reads phase p0 + K * lane + k without a wrap
//                                 (kernel_narrowband.hpp has the bank arithmetic)
// Tile: M consecutive 8 kHz samples [m0, m0 + M) and the outputs o with floor(o * orig_u / new_u) in that range.  Their 16-tap windows
// reach from m0 - halo_lo to m0 + M + halo_hi (exclusive): halo_lo = max over phases of floor(p * orig_u / new_u) - start_u[p],
// halo_hi = max of start_u[p] + 16 - floor(p * orig_u / new_u) - 1; both are read off the first-tap table (7 or 8 and 9: the window has
// 12.12 live taps around the output's position and one or two clamped ones on either side).
// M is 1024 where the LDS map fits 160 KB, else 512, else 256; a rate that does not fit at 256 is not served.
#pragma once
#include "sinc_tables.hpp"

namespace hipfeat {

constexpr int kNbThreads = 256;
constexpr int kNbBlock = 3;           // K: consecutive outputs of a lane, both phases (odd: see the bank arithmetic)
constexpr int kNbUpTaps = 16;         // W of every 8000 -> rate filter with rate > 8000
constexpr int kNbTileMax = 1024, kNbTileMin = 256;
constexpr int64_t kNbMaxLds = 160 * 1024;
constexpr int32_t kNbRate = 8000;
constexpr int64_t kNbMaxCols = 1 << 30;

struct NbFilter {
  int32_t orig = 0, nw = 0, width = 0, W = 0, np = 0;
  std::vector<float> w;        // [nw][W]
  std::vector<int32_t> first;  // [nw]
  int32_t start(int64_t p) const { return (int32_t)((p / nw) * orig + first[(size_t)(p % nw)] - width); }
};

struct NbPlan {
  int status = 0;  // 0 OK, 1 INVALID, 3 UNSUPPORTED (hipfeat_status)
  std::string message;
  int32_t rate = 0;
  bool passthrough = false;  // rate == 8000: no filter at all
  NbFilter down, up;
  int32_t M = 0, halo_lo = 0, halo_hi = 0;
  int32_t span_cap = 0;      // floats of the staging area: the input span of a tile, later its outputs
  int32_t off_wd = 0, off_wu = 0, off_sd = 0, off_su = 0, off_x = 0, off_q = 0;  // LDS map, in floats
  int32_t table_floats = 0;  // the blob: [wt_down | wt_up | start_down | start_up], copied to LDS offset 0
  int64_t lds_bytes = 0;
};

inline int32_t nb_np(int32_t nw) { return (nw + 64 * kNbBlock - 1 + 63) / 64 * 64; }

inline NbPlan nb_refuse(int status, const char* fmt, long long a = 0, long long b = 0) {
  NbPlan p;
  char buf[256];
  std::snprintf(buf, sizeof(buf), fmt, a, b);
  p.status = status;
  p.message = buf;
  return p;
}

// dims of one resampler, nothing built
inline int nb_filter_dims(int32_t src, int32_t dst, NbFilter& f) {
  int32_t d[4];
  const int st = sinc_supported(src, dst, d);
  f.orig = d[0], f.nw = d[1], f.width = d[2], f.W = d[3], f.np = st == 0 ? nb_np(d[1]) : 0;
  return st;
}

inline void nb_filter_build(NbFilter& f) {
  const double base = sinc_base(f.orig, f.nw);
  f.first.resize((size_t)f.nw);
  f.w.resize((size_t)f.nw * f.W);
  for (int32_t ph = 0; ph < f.nw; ++ph) {
    const int32_t i0 = f.first[(size_t)ph] = sinc_first_tap(ph, f.orig, f.nw, f.width, base);
    for (int32_t d = 0; d < f.W; ++d) f.w[(size_t)ph * f.W + d] = sinc_weight(ph, i0 + d, f.orig, f.nw, f.width, base);
  }
}

// input samples under `region` consecutive outputs of the down filter, at most (start is ascending: build checks it)
inline int32_t nb_in_span(const NbPlan& p, int32_t region) {
  int32_t span = 0;
  for (int32_t p0 = 0; p0 < p.down.nw; ++p0) span = std::max(span, p.down.start((int64_t)p0 + region - 1) - p.down.start(p0) + p.down.W);
  return span;
}

// the LDS map of a tile size; false: beyond kNbMaxLds
inline bool nb_map(NbPlan& p, int32_t M) {
  p.M = M;
  const int32_t region = M + p.halo_lo + p.halo_hi;
  const int64_t outs = (int64_t)M * p.up.nw / p.up.orig + 2;  // outputs of a tile
  p.span_cap = (int32_t)((std::max<int64_t>(nb_in_span(p, region) + 3, outs) + 3) / 4 * 4);
  p.off_wd = 0;
  p.off_wu = p.down.W * p.down.np;
  p.off_sd = p.off_wu + p.up.W * p.up.np;
  p.off_su = p.off_sd + p.down.np;
  p.table_floats = p.off_su + p.up.np;
  p.off_x = p.table_floats;
  p.off_q = p.off_x + p.span_cap;
  p.lds_bytes = 4 * ((int64_t)p.off_q + (region + 3) / 4 * 4);
  return p.lds_bytes <= kNbMaxLds;
}

// with_weights = false: geometry and LDS map alone (first taps are built, weights are not)
inline NbPlan build_nb_plan(int32_t rate, bool with_weights, std::vector<float>* blob) {
  if (rate <= 0) return nb_refuse(1, "narrowband: a source rate of %lld Hz", rate);
  NbPlan p;
  p.rate = rate;
  if (rate == kNbRate) {  // the codec alone: a tile is M samples in, M samples out
    p.passthrough = true;
    p.M = kNbTileMax;
    p.span_cap = 0;
    p.off_q = 0;
    p.lds_bytes = 4 * kNbTileMax;
    return p;
  }
  if (rate < kNbRate)
    return nb_refuse(3, "narrowband: a source rate of %lld Hz is not served (the kernel's second filter has the 16 taps of 8000 Hz -> a higher rate)", rate);
  const int st_d = nb_filter_dims(rate, kNbRate, p.down), st_u = nb_filter_dims(kNbRate, rate, p.up);
  if (st_d != 0 || st_u != 0 || p.up.W != kNbUpTaps)
    return nb_refuse(3, "narrowband: a source rate of %lld Hz needs a window of %lld taps per phase, more than the kernel holds", rate, p.down.W);
  // the smallest map (M = 256, halos of 9) must fit before anything of new x W floats is built
  const int64_t least = 4 * ((int64_t)p.down.W * p.down.np + (int64_t)p.up.W * p.up.np + p.down.np + p.up.np);
  if (least > kNbMaxLds)
    return nb_refuse(3, "narrowband: the filter tables of a source rate of %lld Hz take %lld bytes of LDS, more than 160 KB", rate, least);
  const double base_d = sinc_base(p.down.orig, p.down.nw), base_u = sinc_base(p.up.orig, p.up.nw);
  if (with_weights) {
    nb_filter_build(p.down), nb_filter_build(p.up);
  } else {
    p.down.first.resize((size_t)p.down.nw), p.up.first.resize((size_t)p.up.nw);
    for (int32_t ph = 0; ph < p.down.nw; ++ph) p.down.first[(size_t)ph] = sinc_first_tap(ph, p.down.orig, p.down.nw, p.down.width, base_d);
    for (int32_t ph = 0; ph < p.up.nw; ++ph) p.up.first[(size_t)ph] = sinc_first_tap(ph, p.up.orig, p.up.nw, p.up.width, base_u);
  }
  for (const NbFilter* f : {&p.down, &p.up})
    for (int32_t q = 0; q < f->nw; ++q)
      if (f->start(q + 1) < f->start(q)) return nb_refuse(3, "narrowband: the windows of a source rate of %lld Hz do not ascend with the phase", rate);
  for (int32_t ph = 0; ph < p.up.nw; ++ph) {
    const int32_t pos = (int32_t)((int64_t)ph * p.up.orig / p.up.nw), s = p.up.start(ph);
    p.halo_lo = std::max(p.halo_lo, pos - s);
    p.halo_hi = std::max(p.halo_hi, s + kNbUpTaps - 1 - pos);
  }
  int32_t M = kNbTileMax;
  while (!nb_map(p, M) && M > kNbTileMin) M /= 2;
  if (p.lds_bytes > kNbMaxLds)
    return nb_refuse(3, "narrowband: a source rate of %lld Hz needs %lld bytes of LDS for its tables and a tile of 256 samples, more than 160 KB", rate, p.lds_bytes);
  if (blob && with_weights) {
    blob->assign((size_t)p.table_floats, 0.0f);
    int32_t* ints = reinterpret_cast<int32_t*>(blob->data());
    const NbFilter* fs[2] = {&p.down, &p.up};
    const int32_t off_w[2] = {p.off_wd, p.off_wu}, off_s[2] = {p.off_sd, p.off_su};
    for (int k = 0; k < 2; ++k)
      for (int32_t q = 0; q < fs[k]->np; ++q) {
        ints[off_s[k] + q] = fs[k]->start(q);
        for (int32_t d = 0; d < fs[k]->W; ++d) (*blob)[(size_t)off_w[k] + (size_t)d * fs[k]->np + q] = fs[k]->w[(size_t)(q % fs[k]->nw) * fs[k]->W + d];
      }
  }
  return p;
}

}  // namespace hipfeat
