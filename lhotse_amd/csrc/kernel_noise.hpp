// Gaussian noise on a batch of waveforms (RandomizedSmoothing, lhotse/dataset/signal_transforms.py:63-118) in one launch, gfx950 only:
//
//   out[b, t] = clip( x[b, t] + a[b, t] * n(seed, key_b, t) ),    a[b, t] = sigma[b] if t < lengths[b] else 0
//
// THE CONTRACT (stated here and in include/hipfeat.h; tests/_noise_ref.py is its float64 statement):
//   generator   Philox4x32-10 as published (Salmon et al., SC'11): multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and
//               0xBB67AE85, key (seed & 0xffffffff, seed >> 32), counter (q & 0xffffffff, q >> 32, key_b & 0xffffffff, key_b >> 32) with
//               q = t / 4 counted from the row's first sample.
//   normals     the four words r0 ... r3 of counter q are the normals of samples 4 q ... 4 q + 3, by two Box-Muller pairs (r0, r1) and
//               (r2, r3) on exactly representable uniforms:  u1 = ((r >> 8) + 1) 2^-24,  u2 = (r' >> 8) 2^-24,
//               n_even = sqrt(-2 ln u1) cos(2 pi u2),  n_odd = sqrt(-2 ln u1) sin(2 pi u2).
//   arithmetic  float32; float16 / bfloat16 samples convert exactly; product and sum are ONE fmaf(a, n, x); one rounding to nearest even
//               into the output type; the clip passes NaN on; a sample with a == 0 is clip(x) bit for bit (no product is formed).
// A sample's noise is a pure function of (seed, key_b, t): the same bits for any batch composition, row stride and alignment.
//
// sqrt(-2 ln u1) = v_sqrt(-2 ln 2 * v_log(u1)) (1 ulp each; u1 >= 2^-24 is never subnormal, and u1 == 1 gives 0).  The angle never exists
// as a float: u2 = k 2^-24 is cut in integers into a quadrant (k >> 22) and a 22-bit rest m, the rest is folded at the eighth of a turn
// (m > 2^21 -> 2^22 - m, sine and cosine trade places), and f = m 2^-22 in [0, 1/2], exact, goes through two polynomials in z = f * f:
//   sin(pi/2 f) = f (pi/2 + z S(z)),  cos(pi/2 f) = C(z)
// (Chebyshev interpolants; over all 2^21 + 1 values of f both are within 1.4 * 2^-24 of the truth, RELATIVE -- a cosine next to its
// zero is the sine of an exact small f).  The quadrant then sets signs and order.  No range reduction error, no table, no LDS.
//
// Work split: a row of the output is cut at the 16-byte boundaries of its own addresses into a head (< one group), G whole 16-byte
// groups and a tail.  Every row gets the same number of slots, cols / EPG + 2 (EPG = elements per group): slot s < G is group s, the
// last two slots are head and tail, the ones between are idle (at most one per row).  The launch runs over the flat list rows * slots
// with 64-bit indices, kNoiseSlotsPerLane slots per lane a workgroup's width apart (a wave stores 1 KiB on end per step); the division
// by slots is made once per workgroup, a lane corrects it by a compare (or a 32-bit division where rows are shorter than the
// workgroup's span).  A group whose first sample is no multiple of four (the row's head is not) straddles one counter more than an
// aligned one: it makes one more Philox call and picks its normals by the row's phase -- the "two calls" route; an aligned row pays nothing.
// Rows with sigma == 0 and groups behind lengths[b] make no call at all.  No atomics, no scratch, no memset, no workspace; nothing
// behind `cols` of a row is read or written; x may be the output itself (a lane reads what it overwrites before it does).
#pragma once
#include "common.hpp"

namespace hipfeat {

constexpr int kNoiseThreads = 256;
constexpr int kNoiseSlotsPerLane = 4;
constexpr int kNoiseSpan = kNoiseThreads * kNoiseSlotsPerLane;  // slots per workgroup

struct NoiseParams {
  const void* in;
  void* out;
  const float* sigma;      // [rows]
  const int64_t* keys;     // [rows] or null: the row index
  const int64_t* lengths;  // [rows] or null: cols
  int64_t rows, cols, in_row, out_row;  // strides in elements
  uint64_t slots;                       // per row
  uint32_t seed_lo, seed_hi;
  float lo, hi;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  r[0] = c0, r[1] = c1, r[2] = c2, r[3] = c3;
}

// One Box-Muller pair: (sqrt(-2 ln u1) cos(2 pi u2), sqrt(-2 ln u1) sin(2 pi u2))
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& even, float& odd) {
  const float u1 = (float)((ra >> 8) + 1u) * 0x1p-24f;
  const float rad = __builtin_amdgcn_sqrtf(-1.38629436111989062f * __builtin_amdgcn_logf(u1));  // -2 ln 2 * log2(u1)
  const uint32_t k = rb >> 8, quad = k >> 22, m = k & 0x3FFFFFu;
  const bool fold = m > 0x200000u;
  const float f = (float)(fold ? 0x400000u - m : m) * 0x1p-22f;
  const float z = f * f;
  float s = fmaf(fmaf(fmaf(-0x1.2d9b40p-8f, z, 0x1.465ec4p-4f), z, -0x1.4abbbap-1f), z, -0x1.777a5cp-25f);  // z S(z) + (pi/2 - float(pi/2))
  s = fmaf(f, 0x1.921fb6p+0f, f * s);
  const float c = fmaf(fmaf(fmaf(fmaf(0x1.d9c2e8p-11f, z, -0x1.55c57ap-6f), z, 0x1.03c1dcp-2f), z, -0x1.3bd3ccp+0f), z, 1.0f);
  const bool trade = fold != ((quad & 1u) != 0);  // the odd quadrants trade sine and cosine once more
  const float sn = trade ? c : s, cs = trade ? s : c;
  even = __uint_as_float(__float_as_uint(cs) ^ (((quad + 1u) & 2u) << 30)) * rad;
  odd = __uint_as_float(__float_as_uint(sn) ^ ((quad & 2u) << 30)) * rad;
}

struct NoiseRow {
  uint32_t key_lo, key_hi, seed_lo, seed_hi;
};

// the normals of samples 4 q ... 4 q + 3 of a row
__device__ __forceinline__ void noise_normals4(const NoiseRow& row, uint64_t q, float* n) {
  uint32_t r[4];
  philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), row.key_lo, row.key_hi, row.seed_lo, row.seed_hi, r);
  box_muller(r[0], r[1], n[0], n[1]);
  box_muller(r[2], r[3], n[2], n[3]);
}

__device__ __forceinline__ float noise_pick(float a, float b, float c, float d, int phase) {
  return phase == 0 ? a : phase == 1 ? b : phase == 2 ? c : d;
}

// float32, binary16 and bfloat16 samples: exact widening, one rounding to nearest even on the way back
template <class T>
__device__ __forceinline__ float noise_widen(T v) {
  return (float)v;
}
template <class T>
__device__ __forceinline__ T noise_narrow(float v) {
  return (T)v;
}

__device__ __forceinline__ float noise_sample(float x, float a, float n, float lo, float hi) {
  const float v = a == 0.0f ? x : fmaf(a, n, x);
  return v < lo ? lo : (v > hi ? hi : v);  // NaN fails both comparisons and passes through
}

// samples [t0, t1) of a row one by one: the head in front of the row's first 16-byte boundary and the tail behind its last
template <class T>
__device__ __forceinline__ void noise_span(const T* x, T* o, int64_t t0, int64_t t1, int64_t len, float sigma, const NoiseRow& row,
                                           float lo, float hi) {
  float n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int64_t have = -1;
  for (int64_t t = t0; t < t1; ++t) {
    const float a = t < len ? sigma : 0.0f;
    if (a != 0.0f && (t >> 2) != have) {
      have = t >> 2;
      noise_normals4(row, (uint64_t)have, n);
    }
    o[t] = noise_narrow<T>(noise_sample(noise_widen(x[t]), a, noise_pick(n[0], n[1], n[2], n[3], (int)(t & 3)), lo, hi));
  }
}

// one 16-byte group of the output: samples [t0, t0 + EPG) of the row, o + t0 on a 16-byte boundary
template <class T>
__device__ __forceinline__ void noise_group(const T* x, T* o, int64_t t0, int64_t len, float sigma, const NoiseRow& row, float lo,
                                            float hi) {
  constexpr int EPG = 16 / (int)sizeof(T), CPG = EPG / 4;
  union Pack {
    uint4 q;
    T e[EPG];
  } in, out;
  if ((((uintptr_t)(x + t0)) & 15) == 0) {
    in.q = *reinterpret_cast<const uint4*>(x + t0);
  } else {  // the input row sits at another phase of the 16 bytes than the output row
#pragma unroll
    for (int j = 0; j < EPG; ++j) in.e[j] = x[t0 + j];
  }
  float n[4 * CPG + 4];
#pragma unroll
  for (int j = 0; j < 4 * CPG + 4; ++j) n[j] = 0.0f;
  const int phase = (int)(t0 & 3);
  if (sigma != 0.0f && t0 < len) {
    const uint64_t q0 = (uint64_t)t0 >> 2;
#pragma unroll
    for (int c = 0; c < CPG; ++c) noise_normals4(row, q0 + c, n + 4 * c);
    if (phase) noise_normals4(row, q0 + CPG, n + 4 * CPG);
  }
#pragma unroll
  for (int j = 0; j < EPG; ++j) {
    const float a = t0 + j < len ? sigma : 0.0f;
    out.e[j] = noise_narrow<T>(noise_sample(noise_widen(in.e[j]), a, noise_pick(n[j], n[j + 1], n[j + 2], n[j + 3], phase), lo, hi));
  }
  *reinterpret_cast<uint4*>(o + t0) = out.q;
}

template <class T>
__global__ __launch_bounds__(kNoiseThreads) void noise_kernel(const NoiseParams p) {
  constexpr int EPG = 16 / (int)sizeof(T);
  const uint64_t start = (uint64_t)blockIdx.x * kNoiseSpan;
  const uint64_t row0 = start / p.slots, slot0 = start - row0 * p.slots;  // uniform: once per workgroup
#pragma unroll 1
  for (int k = 0; k < kNoiseSlotsPerLane; ++k) {
    uint64_t b = row0, slot = slot0 + (uint32_t)(k * kNoiseThreads) + threadIdx.x;
    if (p.slots >= (uint64_t)kNoiseSpan) {  // at most one row boundary inside the workgroup's span
      if (slot >= p.slots) slot -= p.slots, ++b;
    } else {  // slot < 2 * kNoiseSpan
      const uint32_t d = (uint32_t)slot / (uint32_t)p.slots;
      b += d, slot -= (uint64_t)d * p.slots;
    }
    if (b >= (uint64_t)p.rows) return;
    const T* x = static_cast<const T*>(p.in) + (int64_t)b * p.in_row;
    T* o = static_cast<T*>(p.out) + (int64_t)b * p.out_row;
    const int64_t head = min((int64_t)(((0 - (uintptr_t)o) & 15) / sizeof(T)), p.cols);
    const int64_t groups = (p.cols - head) / EPG;
    if (slot >= (uint64_t)groups && slot < p.slots - 2) continue;  // the idle slot of a row whose head is not empty
    const float sigma = p.sigma[b];
    const uint64_t key = p.keys ? (uint64_t)p.keys[b] : b;
    const int64_t len = p.lengths ? min(max(p.lengths[b], (int64_t)0), p.cols) : p.cols;
    const NoiseRow row{(uint32_t)key, (uint32_t)(key >> 32), p.seed_lo, p.seed_hi};
    if (slot < (uint64_t)groups)
      noise_group<T>(x, o, head + (int64_t)slot * EPG, len, sigma, row, p.lo, p.hi);
    else if (slot == p.slots - 2)
      noise_span<T>(x, o, 0, head, len, sigma, row, p.lo, p.hi);
    else
      noise_span<T>(x, o, head + groups * EPG, p.cols, len, sigma, row, p.lo, p.hi);
  }
}

}  // namespace hipfeat
