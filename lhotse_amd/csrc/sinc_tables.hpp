// Host side of sinc_kernel (kernel_sinc.hpp), the resampler WITHOUT a filter bank: the geometry of a rate pair, the window of taps a
// phase needs, the weight formula itself, the workgroup table of a launch and the support rule -- what hipfeat_sinc_plan validates and
// builds, once per plan.  Pure C++ (no HIP; the functions the kernel shares carry SINC_HD, which is empty here): also compiled by
// tests/native/sinc_tables_capi.cpp and checked on the CPU (tests/test_sinc_tables.py).
//
// Reference: _get_sinc_resample_kernel (lhotse/augmentation/resample.py:184-283) builds, for orig : new reduced by their gcd, a dense
// bank K[new][2 * width + orig], width = ceil(6 * orig / base), base = min(orig, new) * 0.99, every entry in float64:
//     t = ((float)(-ph) / (float)new  +  (i - width) / orig) * base        (the phase term is a float32 division, :253-257)
//     t = clamp(t, -6, 6);  window = cos(t * pi / 6 / 2)^2;  t *= pi
//     K[ph][i] = (float)((t == 0 ? 1 : sin(t) / t) * (window * (base / orig)))
// Behind the clamp |t| = 6 the window is cos(pi / 2)^2 ~ 4e-33 and sin(6 pi) / (6 pi) ~ 4e-17: the product underflows to +-0 in float32.
// So per phase only the taps with unclamped |t| < 6 carry weight.  They are consecutive, and there are at most 2 * width of them (an
// open interval of 12 * orig / base <= 2 * width taps).  The WINDOW of phase ph is the W = 2 * width + 2 taps from i0(ph) = (first tap
// with unclamped |t| < 6) - 1 on: every live tap and at least one clamped tap on either side.  The formula, clamp included, is evaluated
// on every tap of the window: clamped taps come out as +-0 by the reference's own arithmetic, and nothing has to decide whether a tap
// is live.  (Window taps below 0 or from 2 * width + orig on do not exist in the reference; here they are clamped taps: weight +-0.)
//
// A launch resamples R ROWS of one arena, each with its own orig : new.  A WORKGROUP takes one row, a tile of kSincPhases consecutive
// phases and a chunk of kSincHops hops (hop j = output samples [j * new, (j + 1) * new)): a lane owns one phase, evaluates its W
// weights once and walks the chunk's hops.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define SINC_HD __host__ __device__
#else
#define SINC_HD
#endif

namespace hipfeat {

constexpr int kSincPhases = 256;  // phases of a workgroup = its lanes
// Hops of a workgroup.  A tuning constant that nothing measured backs: the rate pairs this kernel is for have thousands of phases and a
// few hops per second of audio (8000:4673 -> two hops per second), so that all hops of a cut fall into one chunk and every weight is
// evaluated once; rows with few phases and many hops (441:160: 100 hops per second) are cut into chunks to have workgroups at all.
constexpr int kSincHops = 64;
// The W cap: the weights of a workgroup live in LDS as [W][kSincPhases] float32, 1 KiB per tap.  96 taps = 96 KiB of the 160 KiB a CU
// has; width 47.  (48000 -> 7000 Hz, the low end of LowpassUsingResampling's default cutoffs at 48 kHz, needs width 42, W = 86.)
constexpr int kSincMaxW = 96;
constexpr int32_t kSincMaxRate = 1 << 24;  // reduced rates: (float)ph and (float)new are exact, as in the reference

constexpr double kSincPi = 3.141592653589793;  // math.pi
constexpr double kSincZeros = 6.0;             // lowpass_filter_width
constexpr double kSincRolloff = 0.99;

inline double sinc_base(int32_t orig, int32_t nw) { return (double)std::min(orig, nw) * kSincRolloff; }
inline int64_t sinc_width(int32_t orig, int32_t nw) { return (int64_t)std::ceil(6.0 * (double)orig / sinc_base(orig, nw)); }  // resample.py:239

// float32 division, correctly rounded (the device's `/` may be compiled to a reciprocal)
SINC_HD inline float sinc_fdiv(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}

// the unclamped t of (phase, tap): resample.py:246-258
SINC_HD inline double sinc_t(int32_t ph, int32_t i, int32_t orig, int32_t nw, int32_t width, double base) {
  const double phase = (double)sinc_fdiv((float)(-ph), (float)nw);
  return (phase + (double)(i - width) / (double)orig) * base;
}

SINC_HD inline bool sinc_live(int32_t ph, int32_t i, int32_t orig, int32_t nw, int32_t width, double base) {
  const double t = sinc_t(ph, i, orig, nw, width, base);
  return t > -kSincZeros && t < kSincZeros;
}

// i0(ph): one tap below the first live tap.  An estimate from the rates, then corrected with the predicate itself, so that host and
// device agree whatever the estimate's rounding was (t ascends with the tap: the corrections end, within a step or two).
SINC_HD inline int32_t sinc_first_tap(int32_t ph, int32_t orig, int32_t nw, int32_t width, double base) {
  int32_t i = width + (int32_t)floor((double)orig * ((double)ph / (double)nw - kSincZeros / base)) + 1;
  while (sinc_t(ph, i - 1, orig, nw, width, base) > -kSincZeros) --i;
  while (sinc_t(ph, i, orig, nw, width, base) <= -kSincZeros) ++i;
  return i - 1;
}

// K[ph][i] of the reference, any integer i (resample.py:246-281)
SINC_HD inline float sinc_weight(int32_t ph, int32_t i, int32_t orig, int32_t nw, int32_t width, double base) {
  double t = sinc_t(ph, i, orig, nw, width, base);
  t = t < -kSincZeros ? -kSincZeros : (t > kSincZeros ? kSincZeros : t);
  const double c = cos(t * kSincPi / kSincZeros / 2.0);
  const double window = c * c;
  t = t * kSincPi;
  const double scale = base / (double)orig;
  const double k = t == 0.0 ? 1.0 : sin(t) / t;
  return (float)(k * (window * scale));
}

// resample.py:309: torch.ceil(torch.as_tensor(new * length / orig)), the quotient a Python float stored as float32 (= hipfeat_resampled_length)
inline int64_t sinc_out_len(int64_t n, int32_t orig, int32_t nw) { return (int64_t)std::ceil((float)((double)nw * (double)n / (double)orig)); }

struct SincRow {
  int64_t in_off, out_off;  // arena offsets
  int32_t in_len, out_len;
  int32_t orig, nw, width;  // reduced rates; W = 2 * width + 2
  int32_t tiles;            // phase tiles: ceil(min(nw, out_len) / kSincPhases)
  int32_t hops;             // ceil(out_len / nw)
  int32_t wg_first;         // exclusive prefix sum of the rows' workgroups (tiles * ceil(hops / kSincHops))
  double base;              // min(orig, nw) * 0.99
  int64_t pad;
};
static_assert(sizeof(SincRow) == 64, "descriptor size");

inline int64_t sinc_chunks(const SincRow& r) { return ((int64_t)r.hops + kSincHops - 1) / kSincHops; }
inline int64_t sinc_row_workgroups(const SincRow& r) { return (int64_t)r.tiles * sinc_chunks(r); }

struct SincPlan {
  int status = 0;       // 0 OK, 1 INVALID, 3 UNSUPPORTED (hipfeat_status)
  std::string message;  // of a refusal
  std::vector<SincRow> rows;      // the rows that have output samples, in the caller's order
  std::vector<int64_t> out_len;   // of every row of the caller
  int64_t workgroups = 0, arena_need = 0;
  int32_t max_w = 0;
};

inline SincPlan sinc_refuse(int status, const char* fmt, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
  SincPlan p;
  char buf[256];
  std::snprintf(buf, sizeof(buf), fmt, a, b, c, d);
  p.status = status;
  p.message = buf;
  return p;
}

// THE support rule of a rate pair (unreduced rates): 0 served, 1 INVALID, 3 UNSUPPORTED; dims (may be NULL) = {orig, new, width, W}
inline int sinc_supported(int64_t src_rate, int64_t dst_rate, int32_t* dims) {
  if (dims) dims[0] = dims[1] = dims[2] = dims[3] = 0;
  if (src_rate <= 0 || dst_rate <= 0 || src_rate == dst_rate) return 1;
  const int64_t g = std::gcd(src_rate, dst_rate);
  const int64_t orig = src_rate / g, nw = dst_rate / g;
  if (orig > kSincMaxRate || nw > kSincMaxRate) return 3;
  const int64_t width = sinc_width((int32_t)orig, (int32_t)nw), W = 2 * width + 2;
  if (dims) dims[0] = (int32_t)orig, dims[1] = (int32_t)nw, dims[2] = (int32_t)std::min<int64_t>(width, INT32_MAX / 4), dims[3] = (int32_t)std::min<int64_t>(W, INT32_MAX / 2);
  return W > kSincMaxW ? 3 : 0;
}

inline SincPlan build_sinc_plan(int64_t num_rows, const int64_t* h_in_offset, const int64_t* h_in_len, const int32_t* h_src_rate, const int32_t* h_dst_rate,
                                const int64_t* h_out_offset, int64_t arena_floats) {
  constexpr int64_t kMaxLen = INT32_MAX / 2;
  if (num_rows < 0 || num_rows > 65535) return sinc_refuse(1, "bad batch arguments (0 ... 65535 rows)");
  if (arena_floats < 0) return sinc_refuse(1, "an arena of %lld floats", arena_floats);
  if (num_rows > 0 && (!h_in_offset || !h_in_len || !h_src_rate || !h_dst_rate || !h_out_offset)) return sinc_refuse(1, "NULL argument");
  SincPlan p;
  p.out_len.assign((size_t)num_rows, 0);
  struct Range {
    int64_t lo, hi, row;
  };
  std::vector<Range> ins, outs;
  for (int64_t i = 0; i < num_rows; ++i) {
    const int64_t io = h_in_offset[i], n = h_in_len[i], oo = h_out_offset[i], src = h_src_rate[i], dst = h_dst_rate[i];
    if (src <= 0 || dst <= 0) return sinc_refuse(1, "row %lld: rates %lld -> %lld, both must be positive", i, src, dst);
    if (src == dst) return sinc_refuse(1, "row %lld: equal rates %lld -> %lld (nothing to resample: leave the row out)", i, src, dst);
    if (io < 0 || oo < 0) return sinc_refuse(1, "row %lld: negative offset (input %lld, output %lld)", i, io, oo);
    if (n < 0 || n > kMaxLen) return sinc_refuse(1, "row %lld: %lld samples, must be 0 ... %lld", i, n, kMaxLen);
    int32_t dims[4];
    if (sinc_supported(src, dst, dims) != 0 && dims[3] == 0)
      return sinc_refuse(3, "row %lld: %lld -> %lld: the rates reduced by their gcd must not exceed 2^24", i, src, dst);
    if (sinc_supported(src, dst, dims) != 0)
      return sinc_refuse(3, "row %lld: %lld -> %lld needs a window of %lld taps per phase, more than the kernel holds", i, src, dst, dims[3]);
    const int64_t out_len = sinc_out_len(n, dims[0], dims[1]);
    if (out_len > kMaxLen) return sinc_refuse(1, "row %lld: %lld samples come out, must be 0 ... %lld", i, out_len, kMaxLen);
    if (io > arena_floats - n) return sinc_refuse(1, "row %lld: the input %lld + %lld lies past the arena of %lld floats", i, io, n, arena_floats);
    if (oo > arena_floats - out_len) return sinc_refuse(1, "row %lld: the output %lld + %lld lies past the arena of %lld floats", i, oo, out_len, arena_floats);
    p.out_len[(size_t)i] = out_len;
    if (out_len == 0) continue;  // (n == 0: nothing is read, nothing is written)
    SincRow r;
    r.in_off = io;
    r.out_off = oo;
    r.in_len = (int32_t)n;
    r.out_len = (int32_t)out_len;
    r.orig = dims[0];
    r.nw = dims[1];
    r.width = dims[2];
    r.tiles = (int32_t)((std::min<int64_t>(r.nw, out_len) + kSincPhases - 1) / kSincPhases);
    r.hops = (int32_t)((out_len + r.nw - 1) / r.nw);
    r.wg_first = (int32_t)p.workgroups;
    r.base = sinc_base(r.orig, r.nw);
    r.pad = 0;
    p.workgroups += sinc_row_workgroups(r);
    if (p.workgroups > INT32_MAX - (1 << 24)) return sinc_refuse(1, "batch too large for one launch");
    p.max_w = std::max(p.max_w, dims[3]);
    p.arena_need = std::max(p.arena_need, std::max(io + n, oo + out_len));
    p.rows.push_back(r);
    ins.push_back({io, io + n, i});
    outs.push_back({oo, oo + out_len, i});
  }
  // no output range may meet an input range (a workgroup reads inputs while another writes outputs) or another output range
  auto by_lo = [](const Range& a, const Range& b) { return a.lo < b.lo; };
  std::sort(ins.begin(), ins.end(), by_lo);
  std::sort(outs.begin(), outs.end(), by_lo);
  for (size_t k = 1; k < outs.size(); ++k)
    if (outs[k - 1].hi > outs[k].lo) return sinc_refuse(1, "rows %lld and %lld: their outputs overlap", outs[k - 1].row, outs[k].row);
  std::vector<int64_t> in_hi_max(ins.size());  // running maximum of the inputs' ends, in order of their starts
  for (size_t k = 0; k < ins.size(); ++k) in_hi_max[k] = std::max(ins[k].hi, k ? in_hi_max[k - 1] : INT64_MIN);
  for (const Range& o : outs) {
    // inputs that start in front of the output's end; one of them ends behind the output's start <=> the running maximum does
    const size_t n_before = (size_t)(std::partition_point(ins.begin(), ins.end(), [&](const Range& r) { return r.lo < o.hi; }) - ins.begin());
    if (n_before == 0 || in_hi_max[n_before - 1] <= o.lo) continue;
    size_t k = 0;
    while (!(ins[k].lo < o.hi && ins[k].hi > o.lo)) ++k;  // (exists)
    return sinc_refuse(1, "row %lld: its output %lld + %lld overlaps the input of row %lld", o.row, o.lo, o.hi - o.lo, ins[k].row);
  }
  return p;
}

}  // namespace hipfeat
