// Host-side constant tables of the specialised kernels: what hipfeat_plan_create uploads for the kernel family that claims a plan.
// Pure C++ (no HIP): also compiled by tests/native/plan_tables_capi.cpp and checked on the CPU (tests/test_plan_tables.py).
//
// A table layout is a contract with a hand-written kernel, so every layout is written once, as a piece that appends to a table; one
// builder per kernel family puts the pieces together and returns the tables with the offsets, counts and LDS bytes the plan keeps.  The
// kernels' geometry constants live next to their device code (kernel_*.hpp): the builders take them as arguments.  `fits == false`:
// the filterbank does not fit the family's schedule, nothing else of the result is meaningful.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "mel4_schedule.hpp"

namespace hipfeat {

// What hipfeat_plan_create was given, as far as the tables depend on it.
struct PlanInputs {
  int N = 0, shift = 0, K = 0;    // frame length, frame shift, bins (fft / 2 + 1)
  int M = 0, C = 0;               // filters (0: none), cepstral coefficients (0: not MFCC)
  const float* window = nullptr;  // [N]
  const float* mel = nullptr;     // [K][M]
  const float* dct = nullptr;     // [M][C]
  const float* lifter = nullptr;  // [C]; nullptr: no liftering
};

// --------------------------------------------------------------------------------------
// pieces
// --------------------------------------------------------------------------------------
// the constant image of a workgroup is copied to LDS in whole 256-byte rows
inline void align64(std::vector<float>& t) { t.resize((t.size() + 63) & ~(size_t)63, 0.0f); }

// window/2 as (even, odd) sample pairs per (row n1, lane q): sample 2 lanes n1 + 2 q + e, zero from N on
inline void append_window_halves(std::vector<float>& t, const float* window, int N, int nrows, int lanes) {
  for (int i = 0; i < 2 * lanes * nrows; ++i) t.push_back(i < N ? 0.5f * window[i] : 0.0f);
}

// pass twiddles W_order^(q k1) = (cos a, sin a), a = -2 pi q k1 / order, per (row k1 = row0 .. row0 + rows - 1, lane q)
inline void append_pass_twiddles(std::vector<float>& t, int rows, int lanes, int order, int row0 = 0) {
  for (int k1 = row0; k1 < row0 + rows; ++k1)
    for (int q = 0; q < lanes; ++q) {
      const double a = -2.0 * M_PI * (double)(q * k1) / (double)order;
      t.push_back((float)std::cos(a));
      t.push_back((float)std::sin(a));
    }
}

// Bin k of the first operand of split step s in lane q.  Plain: q + lanes s.  Lane0Extra (fft1024c; Folded: fft2048c, whose lanes above
// lanes / 2 take bin 2 lanes - q): a step covers 2 lanes bins, lanes >= 1 hold q + 2 lanes s for s < 16 and idle (k = 0) in step 16; lane 0
// holds 2 lanes s (s <= 8), lanes + 2 lanes (s - 9) (s <= 15) and 15 lanes (s = 16)
enum class SplitRule { Plain, Lane0Extra, Lane0ExtraFolded };
inline int split_bin(SplitRule rule, int lanes, int s, int q) {
  if (rule == SplitRule::Plain) return q + lanes * s;
  if (q == 0) return s <= 8 ? 2 * lanes * s : lanes + 2 * lanes * (std::min(s, 16) - 9);
  if (s >= 16) return 0;
  return (rule == SplitRule::Lane0ExtraFolded && q > lanes / 2 ? 2 * lanes - q : q) + 2 * lanes * s;
}

// split-step twiddles w = -i W_order^k = (sin a, -cos a), a = -2 pi k / order, per (step, lane); `rotated` appends (-w.y, w.x) per (step, lane)
inline void append_split_twiddles(std::vector<float>& t, int order, int steps, int lanes, SplitRule rule, bool rotated = false) {
  const size_t at = t.size();
  for (int s = 0; s < steps; ++s)
    for (int q = 0; q < lanes; ++q) {
      const double a = -2.0 * M_PI * (double)split_bin(rule, lanes, s, q) / (double)order;
      t.push_back((float)std::sin(a));
      t.push_back((float)(-std::cos(a)));
    }
  for (size_t i = at, end = t.size(); rotated && i < end; i += 2) {
    t.push_back(-t[i + 1]);
    t.push_back(t[i]);
  }
}

// whisper: twiddles (cos th, -sin th), th = 2 pi (l k2 mod 400) / 400, per (row k2 < 13, lane l < 16) of the 16 x 25 FFT
inline void append_whisper_twiddles(std::vector<float>& t) {
  for (int k2 = 0; k2 < 13; ++k2)
    for (int l = 0; l < 16; ++l) {
      const double th = 2.0 * M_PI * (double)((l * k2) % 400) / 400.0;
      t.push_back((float)std::cos(th));
      t.push_back((float)-std::sin(th));
    }
}

// lifter of the MFCC epilogues: 64 coefficients, ones where none applies (layers.py:681-695)
inline void append_lifter(std::vector<float>& t, const PlanInputs& in) {
  for (int cc = 0; cc < 64; ++cc) t.push_back((in.lifter && cc < in.C) ? in.lifter[cc] : 1.0f);
}

// --------------------------------------------------------------------------------------
// wave-autonomous kernels (fft512c, fft256c, fft1024c, fft2048c, whisper3): one LDS image, the 4x4-block filterbank tables behind it
// --------------------------------------------------------------------------------------
struct WaveAutoGeom {
  int prow_stride, max_sets, max_steps;  // power row stride; accumulator sets and MFMA steps per set of the filterbank schedule
  int waves, region;                     // waves per workgroup, floats of a wave's exchange / power region
};

struct WaveAutoTables {
  bool fits = false;
  std::vector<float> image;  // LDS image: FFT constants | filterbank weights | lane tables, whole rows of 64 floats
  std::vector<float> dct;    // fft512c MFCC: DCT operands | lifter
  std::vector<float> twp;    // fft2048c: [32][32] v2 W_1024^(q k1), read from global memory
  int nrows = 0, mode = 0;   // window rows; fft512c: 0 = 2 sets x 16 steps, 1 = 1 set x 32 steps, 2 / 3 = MFCC with up to 40 / 24 filters
  bool fixed = false, w12 = false;  // the schedule is the one `fixed_steps` names (fixed-schedule instance); fft2048c: its 12-wave layout
  int waves = 0;
  int wtab_off = 0, ltab_off = 0, shared_floats = 0, xs_floats = 0, tws_off = 0, tw32_off = 0;
  int w_nsets = 0, w_steps[4] = {}, w_step0[4] = {};  // fft1024c / fft2048c: the sets the kernel walks
  int sch_nsets = 0, sch_steps = 0;                   // the schedule as built: sets x total steps (kernel name)
  int sch_set_steps[4] = {};                          // the schedule as built: steps of every set (fft512c: the instance with them compiled in)
  size_t lds = 0;
};

// How the tables of a Mel4Schedule go behind the image.  Fixed: the kernel runs `tsets` sets of `tsteps` steps unconditionally, the
// tables are padded (weights 0, no output column).  Steps8: the kernel runs two accumulation chains per set over chunks of 4 steps,
// every set's steps are padded to a multiple of 8 (zero weights; the power-row reads stay inside the wave's region) and the sets the
// kernel walks are the padded ones.  AsIs: the sets as scheduled.
enum class Mel4Pad { Fixed, Steps8, AsIs };
inline void append_mel4(WaveAutoTables& t, const Mel4Schedule& sch, Mel4Pad pad, int tsets = 0, int tsteps = 0) {
  std::vector<float>& img = t.image;
  t.wtab_off = (int)img.size();
  t.sch_nsets = sch.nsets;
  int step0 = 0;
  for (int s2 = 0; s2 < sch.nsets; ++s2) {
    const int padded = pad == Mel4Pad::Fixed ? tsteps : (pad == Mel4Pad::Steps8 ? (sch.steps[s2] + 7) & ~7 : sch.steps[s2]);
    const float* w = sch.wtab.data() + (size_t)sch.step0[s2] * 64;
    img.insert(img.end(), w, w + (size_t)sch.steps[s2] * 64);
    img.resize(img.size() + (size_t)(padded - sch.steps[s2]) * 64, 0.0f);
    if (pad != Mel4Pad::Fixed) t.w_steps[s2] = padded, t.w_step0[s2] = step0, t.w_nsets = sch.nsets;
    t.sch_steps += pad == Mel4Pad::Steps8 ? padded : sch.steps[s2];
    t.sch_set_steps[s2] = sch.steps[s2];
    step0 += padded;
  }
  if (pad == Mel4Pad::Fixed) img.resize((size_t)t.wtab_off + (size_t)tsets * tsteps * 64, 0.0f);
  t.ltab_off = (int)img.size();
  img.insert(img.end(), sch.ltab.begin(), sch.ltab.end());
  float none;
  std::memcpy(&none, &kMel4NoColumn, 4);
  for (int i = sch.nsets * 64; pad == Mel4Pad::Fixed && i < tsets * 64; ++i) img.insert(img.end(), {0.0f, none, 0.0f, 0.0f});
}

// fft2048c: a wave carries TWO frames: rows 2 and 3 of every 4 x 4 block read the power rows of frames 0 and 1 again (their results are dropped)
inline void mel4_two_frames_per_wave(Mel4Schedule& sch, int prow_stride) {
  for (size_t i = 0; i < sch.ltab.size(); i += 4)
    if (((i / 4) & 3) >= 2) {
      int v;
      std::memcpy(&v, &sch.ltab[i], 4);
      v -= 2 * prow_stride;
      std::memcpy(&sch.ltab[i], &v, 4);
    }
}

// closes the image: `waves` waves of `wave_floats` floats (+ `tail_floats`) behind it in LDS
inline void close_image(WaveAutoTables& t, int waves, int wave_floats, int tail_floats = 0) {
  align64(t.image);
  t.shared_floats = (int)t.image.size();
  t.waves = waves;
  t.lds = ((size_t)t.shared_floats + (size_t)waves * wave_floats + tail_floats) * sizeof(float);
  t.fits = true;
}

// fft512c.  Image: window/2 pairs per (row n1, lane q) | W_256^(q k1) per (row k1, lane q) | -i W_512^(q + 16 k2) per (row k2 < 8, lane q) |
// filterbank tables.  MFCC: DCT operands in matrix-core lane order [chunk of 4 filters][lane = cepstral coefficient][filter in the chunk] | lifter
inline WaveAutoTables build_fft512c_tables(const PlanInputs& in, int nrows, const WaveAutoGeom& g, int dct_chunks, int dct_chunks_small) {
  WaveAutoTables t;
  const bool mfcc = in.C > 0;
  Mel4Schedule sch;
  t.mode = mfcc ? (in.M <= 4 * dct_chunks_small ? 3 : 2) : 0;  // 3: 6 chunks of DCT operands + split-step twiddles in registers
  if (mfcc || !build_mel4_schedule(in.mel, in.M, in.K, g.prow_stride, g.max_sets, g.max_steps, sch)) {  // many narrow filters: sets x steps
    if (!build_mel4_schedule(in.mel, in.M, in.K, g.prow_stride, 1, 2 * g.max_steps, sch)) return t;     // few, wide filters: 1 set x twice the steps
    if (!mfcc) t.mode = 1;
  }
  t.nrows = nrows;
  append_window_halves(t.image, in.window, in.N, nrows, 16);
  append_pass_twiddles(t.image, 16, 16, 256);
  append_split_twiddles(t.image, 512, 8, 16, SplitRule::Plain);
  append_mel4(t, sch, Mel4Pad::Fixed, t.mode == 0 ? g.max_sets : 1, t.mode == 0 ? g.max_steps : 2 * g.max_steps);
  t.xs_floats = (3 * in.shift + 32 * nrows + 3) & ~3;
  close_image(t, g.waves, t.xs_floats + g.region);
  if (mfcc) {
    const int dch = t.mode == 3 ? dct_chunks_small : dct_chunks;
    t.dct.assign((size_t)dch * 256, 0.0f);
    for (int m = 0; m < in.M; ++m)
      for (int cc = 0; cc < in.C; ++cc) t.dct[((size_t)(m / 4) * 64 + cc) * 4 + (m & 3)] = in.dct[(size_t)m * in.C + cc];
    append_lifter(t.dct, in);
  }
  return t;
}

// fft256c.  Image: window/2 pairs per (row n1, lane q < 8) | W_128^(q k1) per (row k1, lane q) | -i W_256^(q + 8 j) per (row j < 8, lane q) | tables
inline WaveAutoTables build_fft256c_tables(const PlanInputs& in, int nrows, const WaveAutoGeom& g) {
  WaveAutoTables t;
  Mel4Schedule sch;
  if (!build_mel4_schedule(in.mel, in.M, in.K, g.prow_stride, g.max_sets, g.max_steps, sch)) return t;
  t.nrows = nrows;
  append_window_halves(t.image, in.window, in.N, nrows, 8);
  append_pass_twiddles(t.image, 16, 8, 128);
  append_split_twiddles(t.image, 256, 8, 8, SplitRule::Plain);
  append_mel4(t, sch, Mel4Pad::Fixed, g.max_sets, g.max_steps);
  t.xs_floats = (7 * in.shift + 16 * nrows + 3) & ~3;
  close_image(t, g.waves, t.xs_floats + g.region);
  return t;
}

// fft1024c.  Image: window/2 pairs per (row n1, lane q) | W_512^(q k1) per (row k1 < 32, lane q) | `split_steps` rows of split twiddles | tables.
// fixed_steps: the 3-set schedule a fixed-schedule instance of this configuration has compiled in (nullptr: there is none); such an
// instance runs `waves_fixed` waves whose span buffer aliases the exchange / power region.
inline WaveAutoTables build_fft1024c_tables(const PlanInputs& in, int nrows, const WaveAutoGeom& g, int split_steps, int waves_fixed, const int* fixed_steps) {
  WaveAutoTables t;
  Mel4Schedule sch;
  if (!build_mel4_schedule(in.mel, in.M, in.K, g.prow_stride, g.max_sets, g.max_steps, sch)) return t;
  t.nrows = nrows;
  append_window_halves(t.image, in.window, in.N, nrows, 16);
  append_pass_twiddles(t.image, 32, 16, 512);
  append_split_twiddles(t.image, 1024, split_steps, 16, SplitRule::Lane0Extra);
  append_mel4(t, sch, Mel4Pad::Steps8);
  t.xs_floats = (3 * in.shift + 32 * nrows + 3) & ~3;
  t.fixed = fixed_steps && t.w_nsets == 3 && std::equal(fixed_steps, fixed_steps + 3, t.w_steps) && t.xs_floats <= g.region;
  close_image(t, t.fixed ? waves_fixed : g.waves, t.fixed ? g.region : t.xs_floats + g.region);
  return t;
}

// fft2048c.  Image: window/2 pairs per (row n1, lane q < 32) | split twiddles | butterfly twiddles of pass 2: row 0 = ones (even outputs),
// row 1 = W_32^n (odd outputs) | tables.  As many waves (at most g.waves) as `lds_budget` holds; w12_want: the fixed-schedule instance
// runs `waves_fixed` waves without a span prefetch, the span buffer aliasing the region, when that fits.
inline WaveAutoTables build_fft2048c_tables(const PlanInputs& in, int nrows, const WaveAutoGeom& g, int split_steps, int waves_fixed, const int* fixed_steps,
                                            bool w12_want, size_t lds_budget) {
  WaveAutoTables t;
  Mel4Schedule sch;
  if (!build_mel4_schedule(in.mel, in.M, in.K, g.prow_stride, g.max_sets, g.max_steps, sch)) return t;
  t.nrows = nrows;
  append_window_halves(t.image, in.window, in.N, nrows, 32);
  t.tws_off = (int)t.image.size();
  append_split_twiddles(t.image, 2048, split_steps, 32, SplitRule::Lane0ExtraFolded);
  t.tw32_off = (int)t.image.size();
  for (int n = 0; n < 16; ++n) t.image.insert(t.image.end(), {1.0f, 0.0f});
  append_pass_twiddles(t.image, 1, 16, 32, 1);
  mel4_two_frames_per_wave(sch, g.prow_stride);
  append_mel4(t, sch, Mel4Pad::AsIs);
  append_pass_twiddles(t.twp, 32, 32, 1024);
  t.xs_floats = (in.shift + 64 * nrows + 3) & ~3;
  t.fixed = fixed_steps && t.w_nsets == 3 && std::equal(fixed_steps, fixed_steps + 3, t.w_steps);
  align64(t.image);
  t.w12 = t.fixed && w12_want && t.xs_floats <= g.region && (t.image.size() + (size_t)waves_fixed * g.region) * sizeof(float) <= lds_budget;
  const int wave_floats = t.w12 ? g.region : t.xs_floats + g.region;
  int waves = t.w12 ? waves_fixed : g.waves;
  while (waves > 0 && (t.image.size() + (size_t)waves * wave_floats) * sizeof(float) > lds_budget) --waves;
  close_image(t, waves, wave_floats);
  return t;
}

// whisper3.  Image: window | whisper twiddles | tables; the kernel runs 2 or 3 sets of g.max_steps steps
inline WaveAutoTables build_whisper3_tables(const PlanInputs& in, const WaveAutoGeom& g, int span_floats, int tail_floats) {
  WaveAutoTables t;
  Mel4Schedule sch;
  if (!build_mel4_schedule(in.mel, in.M, in.K, g.prow_stride, g.max_sets, g.max_steps, sch)) return t;
  t.image.assign(in.window, in.window + in.N);
  append_whisper_twiddles(t.image);
  t.w_nsets = sch.nsets <= 2 ? 2 : 3;
  append_mel4(t, sch, Mel4Pad::Fixed, t.w_nsets, g.max_steps);
  close_image(t, g.waves, span_floats + g.region, tail_floats);
  return t;
}

// --------------------------------------------------------------------------------------
// tile kernels (fft512 "b": 16 lanes per row, fft256 "b": 8): banded 16x16x4 matrix-core mel GEMM, MFCC as a second GEMM
// --------------------------------------------------------------------------------------
struct WaveWork {  // mel work of one wave: up to two (tile, band) segments
  int32_t tile0, bin0, ngroups0, tile1, bin1, ngroups1, pad0, pad1;
};

struct TileGeom {
  int lanes, prow_stride, max_groups0, max_groups1;  // lanes per row; power row stride; 8-bin MFMA groups of a wave's first / second mel tile
  int tile_frames, wave_region;
  bool rotated_split;  // the split-step twiddles are followed by their rotated copy
};

struct TileTables {
  bool fits = false;
  std::vector<float> consts;  // LDS constants: window/2 pairs | pass twiddles | split-step twiddles (fft256: | their rotated copy)
  std::vector<float> mel_a;   // [4 waves][steps][64 lanes] MFMA A operands
  std::vector<float> mel_a4;  // the same as 16-byte vectors: [wave][step / 4][lane][step % 4]
  std::vector<float> dct;     // MFCC: DCT^T as MFMA A operands | lifter
  WaveWork work[4] = {};
  int nrows = 0, xs_floats = 0, lm_stride = 0, dct_groups = 0;
  size_t lds = 0;
};

// Mel work split: band of every 16-mel tile in 8-bin groups, assigned to the 4 waves, and the MFMA A operands in lane order.
// Returns false when the filterbank does not fit the static schedule.
inline bool build_mel_schedule(const float* h_mel, int M, int K, const TileGeom& g, int ntiles, WaveWork (&work)[4], std::vector<float>& mel_a) {
  const int regs = 2 * (g.max_groups0 + g.max_groups1);
  struct Seg { int tile, bin, ng; };
  std::vector<Seg> segs;
  for (int t = 0; t < ntiles; ++t) {
    MelBand b = mel_band(h_mel, M, K, 16 * t, 16 * t + 16);
    if (b.hi == 0) b.hi = 1;
    int lo2 = b.lo & ~1;
    int ng = (b.hi - lo2 + 7) / 8;
    if (lo2 + 8 * ng > g.prow_stride) lo2 = (g.prow_stride - 8 * ng) & ~1;  // keep reads inside the padded row
    if (lo2 < 0 || ng > g.max_groups0) return false;
    segs.push_back({t, lo2, ng});
  }
  // the four widest tiles become the waves' first segment, the rest go to the least loaded waves
  std::sort(segs.begin(), segs.end(), [](const Seg& a, const Seg& b) { return a.ng > b.ng; });
  std::memset(work, 0, sizeof(work));
  int load[4] = {0, 0, 0, 0};
  bool has1[4] = {false, false, false, false};
  for (size_t i = 0; i < segs.size(); ++i) {
    const Seg& sg = segs[i];
    if (i < 4) {
      work[i].tile0 = sg.tile; work[i].bin0 = sg.bin; work[i].ngroups0 = sg.ng;
      load[i] = sg.ng;
      continue;
    }
    if (sg.ng > g.max_groups1) return false;
    int best = -1;
    for (int w = 0; w < 4; ++w)
      if (!has1[w] && (best < 0 || load[w] < load[best])) best = w;
    if (best < 0) return false;
    work[best].tile1 = sg.tile; work[best].bin1 = sg.bin; work[best].ngroups1 = sg.ng;
    has1[best] = true;
    load[best] += sg.ng;
  }
  // MFMA A operands: lane (i = lane & 15, kk = lane >> 4) of step (2*gi + r) holds
  // W[bin + 8*gi + 2*kk + r][16*tile + i]; the second segment's steps start at 2*max_groups0
  mel_a.assign((size_t)4 * regs * 64, 0.0f);
  for (int w = 0; w < 4; ++w)
    for (int sgm = 0; sgm < 2; ++sgm) {
      const int tile = sgm ? work[w].tile1 : work[w].tile0, bin = sgm ? work[w].bin1 : work[w].bin0;
      const int ng = sgm ? work[w].ngroups1 : work[w].ngroups0;
      for (int g2 = 0; g2 < ng; ++g2)
        for (int r = 0; r < 2; ++r)
          for (int lane = 0; lane < 64; ++lane) {
            const int i = lane & 15, kk = lane >> 4;
            const int b = bin + 8 * g2 + 2 * kk + r, m = 16 * tile + i;
            const int step = 2 * ((sgm ? g.max_groups0 : 0) + g2) + r;
            if (b < K && m < M) mel_a[((size_t)w * regs + step) * 64 + lane] = h_mel[(size_t)b * M + m];
          }
    }
  return true;
}

// [wave][step][lane] -> 16-byte vectors [wave][step / 4][lane][step % 4]
inline std::vector<float> reorder_mel_a4(const std::vector<float>& mel_a, int regs) {
  std::vector<float> mel_a4(mel_a.size());
  for (int w = 0; w < 4; ++w)
    for (int st = 0; st < regs; ++st)
      for (int lane = 0; lane < 64; ++lane) mel_a4[(((size_t)w * (regs / 4) + st / 4) * 64 + lane) * 4 + (st & 3)] = mel_a[((size_t)w * regs + st) * 64 + lane];
  return mel_a4;
}

// DCT^T as MFMA A operands + lifter (MFCC stage of the tile kernels): lane (i = lane & 15, kk = lane >> 4) of group g,
// half r holds dct[mel = 8 g + 2 kk + r][ceps = 16 ct + i]  (Wav2MFCC._dct, layers.py:697-706)
inline std::vector<float> build_dct_operands(const PlanInputs& in, int dct_groups) {
  const int M = in.M, C = in.C, nct = (C + 15) / 16;
  std::vector<float> da((size_t)nct * dct_groups * 64 * 2, 0.0f);
  for (int ct = 0; ct < nct; ++ct)
    for (int g2 = 0; g2 < dct_groups; ++g2)
      for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < 2; ++r) {
          const int i = lane & 15, kk = lane >> 4, m = 8 * g2 + 2 * kk + r, cc = 16 * ct + i;
          if (m < M && cc < C) da[(((size_t)ct * dct_groups + g2) * 64 + lane) * 2 + r] = in.dct[(size_t)m * C + cc];
        }
  append_lifter(da, in);
  return da;
}

// fft512 "b" (lanes = 16, fft = 512) and fft256 "b" (lanes = 8, fft = 256, with the rotated split twiddles); in.M == 0: spectrogram
inline TileTables build_tile_tables(const PlanInputs& in, int nrows, const TileGeom& g) {
  TileTables t;
  const int ntiles = (in.M + 15) / 16, regs = 2 * (g.max_groups0 + g.max_groups1);
  if (!build_mel_schedule(in.mel, in.M, in.K, g, ntiles, t.work, t.mel_a)) return t;
  t.mel_a4 = reorder_mel_a4(t.mel_a, regs);
  t.nrows = nrows;
  append_window_halves(t.consts, in.window, in.N, nrows, g.lanes);
  append_pass_twiddles(t.consts, 16, g.lanes, 16 * g.lanes);
  append_split_twiddles(t.consts, 32 * g.lanes, 8, g.lanes, SplitRule::Plain, g.rotated_split);
  t.xs_floats = ((g.tile_frames - 1) * in.shift + 2 * g.lanes * nrows + 255) & ~255;  // whole 1 KiB LDS-DMA chunks
  size_t lds_floats = (size_t)t.xs_floats + t.consts.size() + 4 * (size_t)g.wave_region;
  if (in.C > 0) {
    t.dct_groups = (in.M + 7) / 8;
    t.lm_stride = ntiles <= 2 ? 36 : (ntiles <= 4 ? 68 : 132);  // 4 mod 32: conflict-free 8-byte reads of the log-mel tile; 36 keeps MFCC-13 at 4 workgroups/CU
    t.dct = build_dct_operands(in, t.dct_groups);
    lds_floats += (size_t)g.tile_frames * t.lm_stride + t.dct.size();
  }
  t.lds = lds_floats * sizeof(float);
  t.fits = true;
  return t;
}

// --------------------------------------------------------------------------------------
// wave-per-frame kernel
// --------------------------------------------------------------------------------------
// Filterbank blob = [M] int4 {lo rounded down to a multiple of 4, offset of the filter's weights, number of float4 groups, 0} followed
// by the weights themselves, each filter zero-padded to whole float4 groups
inline std::vector<float> build_wave_blob(const float* h_mel, int M, int K) {
  std::vector<int32_t> desc((size_t)4 * M, 0);
  std::vector<float> wts;
  for (int j = 0; j < M; ++j) {
    const MelBand b = mel_band(h_mel, M, K, j, j + 1);
    const int lo4 = b.lo & ~3;
    const int groups = b.hi > b.lo ? (b.hi - lo4 + 3) / 4 : 0;
    desc[(size_t)4 * j] = lo4;
    desc[(size_t)4 * j + 1] = (int32_t)wts.size();
    desc[(size_t)4 * j + 2] = groups;
    for (int k = lo4; k < lo4 + 4 * groups; ++k) wts.push_back(k < K ? h_mel[(size_t)k * M + j] : 0.0f);
  }
  std::vector<float> blob((size_t)4 * M + wts.size());
  std::memcpy(blob.data(), desc.data(), desc.size() * sizeof(int32_t));
  std::memcpy(blob.data() + 4 * M, wts.data(), wts.size() * sizeof(float));
  return blob;
}

struct WaveTables {
  std::vector<float> blob;  // empty: no filterbank (spectrogram kinds)
  bool dct_in_lds = false;
  size_t lds = 0;
};

// H = fft / 2.  LDS: twiddles W_2H^k + 4 padded wave buffers + window + twiddles W_H^m + filterbank blob (+ DCT matrix when it is small)
inline WaveTables build_wave_tables(const PlanInputs& in, int H) {
  WaveTables t;
  if (in.M > 0) t.blob = build_wave_blob(in.mel, in.M, in.K);
  t.dct_in_lds = in.C > 0 && (size_t)in.M * in.C <= 2560;
  auto up4 = [](size_t v) { return (v + 3) & ~(size_t)3; };
  t.lds = ((size_t)2 * H + 4 * ((size_t)144 * (H / 64) + 8) + up4((size_t)in.N) + (size_t)2 * H + up4(t.blob.size()) + (t.dct_in_lds ? (size_t)in.M * in.C : 0)) * sizeof(float);
  return t;
}

// --------------------------------------------------------------------------------------
// whisper2: 400 = 16 x 25 mixed-radix FFT + banded mel GEMM
// --------------------------------------------------------------------------------------
struct Whisper2Tables {
  std::vector<float> cs;       // [12][12] v2 DFT-25 coefficients (cos th, -sin th), th = 2 pi (j k mod 25) / 25, j, k = 1 .. 12 (whisper3 reads it too)
  std::vector<float> tw;       // whisper twiddles
  std::vector<float> mel;      // per 16-filter tile: chunks of 4 k-steps (16 bins) x 64 lanes x 4, zero weights pad the band
  std::vector<int32_t> sched;  // [4 waves][2 slots] {tile (-1: none), first bin, chunks, offset of the tile's chunks}
  int load[4] = {0, 0, 0, 0};  // chunks per wave
};

inline Whisper2Tables build_whisper2_tables(const PlanInputs& in) {
  Whisper2Tables t;
  const int M = in.M, nmt = (M + 15) / 16;
  for (int j = 1; j <= 12; ++j)
    for (int k = 1; k <= 12; ++k) {
      const double th = 2.0 * M_PI * (double)((j * k) % 25) / 25.0;
      t.cs.push_back((float)std::cos(th));
      t.cs.push_back((float)-std::sin(th));
    }
  append_whisper_twiddles(t.tw);
  std::vector<int> k0(nmt), steps(nmt), off(nmt), order(nmt);
  for (int mt = 0; mt < nmt; ++mt) {
    const MelBand b = mel_band(in.mel, M, in.K, 16 * mt, 16 * mt + 16);
    k0[mt] = b.lo & ~3;
    steps[mt] = b.hi > b.lo ? (b.hi - k0[mt] + 15) / 16 : 0;
    off[mt] = (int)(t.mel.size() / 256);
    order[mt] = mt;
    for (int ch = 0; ch < steps[mt]; ++ch)
      for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r) {
          const int bin = k0[mt] + 16 * ch + 4 * r + (l >> 4), m = 16 * mt + (l & 15);
          t.mel.push_back((bin < in.K && m < M) ? in.mel[(size_t)bin * M + m] : 0.0f);
        }
  }
  if (t.mel.empty()) t.mel.assign(256, 0.0f);
  // deal the mel tiles to the four waves: longest first, always to the least loaded wave (at most two tiles each)
  t.sched.assign(32, 0);
  for (int e = 0; e < 8; ++e) t.sched[(size_t)4 * e] = -1;
  int cnt[4] = {0, 0, 0, 0};
  std::sort(order.begin(), order.end(), [&](int a, int b) { return steps[a] > steps[b]; });
  for (int mt : order) {
    int best = -1;
    for (int wv = 0; wv < 4; ++wv)
      if (cnt[wv] < 2 && (best < 0 || t.load[wv] < t.load[best])) best = wv;
    int32_t* e = &t.sched[(size_t)(best * 2 + cnt[best]++) * 4];
    e[0] = mt, e[1] = k0[mt], e[2] = steps[mt], e[3] = off[mt];
    t.load[best] += steps[mt];
  }
  return t;
}

}  // namespace hipfeat
