// Narrowband(codec="mulaw") on a batch of waveforms in one launch, gfx950 only (lhotse/augmentation/torchaudio.py:337-378):
//
//   d = ResampleTensor(rate -> 8000)(x)            L8 = ceil((float)(new * n / orig)) samples (resample.py:309), zeros outside the row
//   u = (sign(d) * log1p(255 |d|) / log1p(255) + 1) / 2 * 255 + 0.5;  c = trunc(u) (no clamp);  v = c / 255 * 2 - 1
//   q = sign(v) * (exp(|v| * log1p(255)) - 1) / 255                   MuLawEncoding(256) then MuLawDecoding(256), float32
//   z = ResampleTensor(8000 -> rate)(q) cut to n samples              (restore; q is 0.0 outside [0, L8), not q(0))
//
// The 8 kHz signal exists in LDS only.  One workgroup of 256 threads = one row and a run of consecutive TILES of M 8 kHz samples
// (narrowband_tables.hpp: the tables, the tile geometry and the LDS map; M, the halos and every offset come in NbArgs).  The plan's blob
// [wt_down | wt_up | start_down | start_up] is copied into LDS once per workgroup with 16-byte loads, then per tile:
//   stage    the input span under the tile's 8 kHz region goes to LDS in 16-byte loads where a group of four lies inside the row and on a
//            16-byte boundary of the row's own address, sample by sample at the row's edges; positions outside [0, n) are 0.0 (what
//            lies behind lengths[b] is never used)
//   phase 1  d over [m0 - halo_lo, m0 + M + halo_hi) from LDS, the codec in registers (log1pf, expf, a correctly rounded division, the
//            cast toward zero), q to LDS; 8 kHz positions outside [0, L8) are 0.0
//   phase 2  the outputs o with floor(o * 8000 / rate) in [m0, m0 + M) from q in LDS, 16 taps, into the staging area (the input span is dead)
//   store    the staging area to the row in 16-byte stores where a group lies on a 16-byte boundary of the output row, +0.0 behind
//            the row's length up to the row width
// with a barrier between the steps.  restore == 0: no halo, no phase 2, the store copies q.  rate == 8000: phase 1 reads x directly.
//
// A FIR sample is the chain of sinc_kernel (kernel_sinc.hpp): acc = 0, one fmaf per tap, taps ascending over the window of W taps.
//
// REGISTER BLOCKING.  In both phases a lane owns K = 3 CONSECUTIVE outputs and a wave 192.  The windows of consecutive outputs start
// e_k = start[p + k] - start[p] samples apart (e_2 <= 3 in phase 2, <= ceil(2 orig / new) + 1 in phase 1) and overlap in all but those,
// so the lane walks the union once -- i = 0 ... W + e_2 - 1, one LDS read of the sample -- and feeds it to each of its outputs at tap
// t = i - e_k where 0 <= t < W: one sample read per (up to) three fmaf.  i ascends, so every output sees its taps in ascending order.
// K = 3 because K must be odd for the weight reads below, 5 costs 2 x 64 more table columns per tap (the 44.1 kHz tables then pass 160 KB
// at every tile size), and the input reuse is already 3 W / (W + e_2).  The weights are read once per fmaf: consecutive outputs have
// different phases and no weight is shared.
//
// BANKS (64 banks of 4 bytes).  wt is tap-major with a row of np floats, np a multiple of 64, at an LDS offset that is a multiple of 64
// floats: the weight of (tap t, phase p) sits in bank p mod 64 WHATEVER t is.  Lane l of a wave reads phase p0 + 3 l + k (p0: the phase
// of the wave's first output, k: the same for all lanes; the table continues the phases periodically up to np, so there is no wrap):
// bank (p0 + k + 3 l) mod 64.  3 is odd, so l -> 3 l mod 64 is a bijection on 0 ... 63: the 64 lanes hit 64 different banks although
// their taps t = i - e_k differ from lane to lane.  start[] is read the same way (p0 + 3 l + k: 64 banks).  The SAMPLE reads are not
// conflict free: lane l reads address start[p0 + 3 l] + i, a lane stride of about 3 orig / new floats -- below 3 in phase 2 (neighbours
// share addresses, which is a broadcast; a wave spans < 192 floats: at most three lanes per bank), 6 at 16 kHz and 16.5 at 44.1 kHz in
// phase 1 (up to 16 lanes per bank).  They are one read in four of the inner loop.
#pragma once
#include "common.hpp"
#include "narrowband_tables.hpp"

namespace hipfeat {

struct NbArgs {
  const float* x;
  float* out;
  const int64_t* lengths;  // [rows] or null: cols
  const float* tables;     // the plan's blob (null: rate == 8000)
  int64_t cols, out_cols, in_row, out_row;
  int32_t tiles, tiles_per_wg, wgs_per_row, restore, passthrough;
  int32_t orig_d, new_d, W_d, np_d, orig_u, new_u, np_u;
  int32_t M, halo_lo, halo_hi, span_cap;
  int32_t off_wd, off_wu, off_sd, off_su, off_x, off_q, table_floats;
};

constexpr float kNbMu = 255.0f;
constexpr float kNbLog1pMu = 5.545177459716797f;  // (float)log1p(255)

__device__ __forceinline__ float nb_sign(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }

// MuLawEncoding(256) then MuLawDecoding(256) in torch's float32 order of operations
__device__ __forceinline__ float nb_codec(float d) {
  const float e = __fdiv_rn(nb_sign(d) * log1pf(kNbMu * fabsf(d)), kNbLog1pMu);
  const float u = __fadd_rn(__fmul_rn(__fdiv_rn(e + 1.0f, 2.0f), kNbMu), 0.5f);  // (no contraction into an fma: torch rounds the product)
  const float c = (float)(int32_t)u;  // toward zero; |u| < 2^12 for every finite d
  const float v = __fdiv_rn(c, kNbMu) * 2.0f - 1.0f;
  return __fdiv_rn(nb_sign(v) * (expf(fabsf(v) * kNbLog1pMu) - 1.0f), kNbMu);
}

// resample.py:309 on the device (= sinc_out_len)
__device__ __forceinline__ int32_t nb_out_len(int32_t n, int32_t orig, int32_t nw) {
  return (int32_t)ceilf((float)((double)nw * (double)n / (double)orig));
}

// Outputs [s_lo, s_hi) of one FIR (outputs counted along the row), each codec'ed or not, to dst[s - dst_s0]: a wave takes chunks of
// 64 K outputs, a lane K consecutive ones.  src[i - src_i0] is input sample i; wt / st: the filter's LDS tables.
template <bool kCodec>
__device__ __forceinline__ void nb_fir(const float* __restrict__ src, int32_t src_i0, float* __restrict__ dst, int32_t dst_s0, int32_t s_lo, int32_t s_hi,
                                       const float* __restrict__ wt, const int32_t* __restrict__ st, int32_t np, int32_t W, int32_t orig, int32_t nw) {
  constexpr int K = kNbBlock;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int32_t s_w = s_lo + wave * 64 * K; s_w < s_hi; s_w += (kNbThreads / 64) * 64 * K) {
    const int32_t j0 = s_w / nw, p = s_w - j0 * nw + K * lane;  // p + k < nw + 64 K - 1 <= np
    const int32_t s = s_w + K * lane;
    if (s >= s_hi) continue;
    const int32_t valid = min(K, s_hi - s);
    const int32_t start0 = st[p];
    int32_t e[K];
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = k < valid ? st[p + k] - start0 : (k ? e[k - 1] : 0);
    const float* __restrict__ xs = src + (j0 * orig + start0 - src_i0);
    const float* __restrict__ w = wt + p;
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0f;
    const int32_t n = W + e[K - 1];
    for (int32_t i = 0; i < n; ++i) {
      const float xv = xs[i];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int32_t t = i - e[k];
        if ((uint32_t)t < (uint32_t)W) acc[k] = fmaf(xv, w[t * np + k], acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (k < valid) dst[s + k - dst_s0] = kCodec ? nb_codec(acc[k]) : acc[k];
  }
}

__global__ __launch_bounds__(kNbThreads) void narrowband_kernel(const NbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float nb_lds[];
  HF_POISON_LDS(nb_lds);
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / a.wgs_per_row;
  const int32_t g = blockIdx.x - (int32_t)b * a.wgs_per_row;
  const float* __restrict__ x = a.x + b * a.in_row;
  float* __restrict__ out = a.out + b * a.out_row;
  const int32_t cols = (int32_t)a.cols, out_cols = (int32_t)a.out_cols;
  const int32_t n = a.lengths ? (int32_t)min(max(a.lengths[b], (int64_t)0), a.cols) : cols;
  const bool filtered = !a.passthrough, up = filtered && a.restore;
  const int32_t L8 = filtered ? nb_out_len(n, a.orig_d, a.new_d) : n;
  const int32_t n_out = up ? n : L8;  // samples of the output row that carry signal
  const int32_t halo_lo = up ? a.halo_lo : 0, halo_hi = up ? a.halo_hi : 0;
  const int32_t t0 = g * a.tiles_per_wg, t1 = min(t0 + a.tiles_per_wg, a.tiles);
  float* __restrict__ xs = nb_lds + a.off_x;
  float* __restrict__ q = nb_lds + a.off_q;
  const float* wd = nb_lds + a.off_wd;
  const float* wu = nb_lds + a.off_wu;
  const int32_t* sd = reinterpret_cast<const int32_t*>(nb_lds + a.off_sd);
  const int32_t* su = reinterpret_cast<const int32_t*>(nb_lds + a.off_su);
  if (filtered && (int64_t)t0 * a.M < L8) {  // (a workgroup behind the row's end only writes zeros)
    const float4* __restrict__ src = reinterpret_cast<const float4*>(a.tables);
    float4* dst = reinterpret_cast<float4*>(nb_lds);
    for (int32_t i = tid; i < a.table_floats / 4; i += kNbThreads) dst[i] = src[i];
  }
  const int32_t ax = (int32_t)(((uintptr_t)x >> 2) & 3), ao = (int32_t)(((uintptr_t)out >> 2) & 3);  // the rows' phases of the 16 bytes
  for (int32_t tile = t0; tile < t1; ++tile) {
    const int32_t m0 = tile * a.M;
    // the outputs of the tile: [o_lo, o_hi) of the output row
    int32_t o_lo = m0, o_hi = min(m0 + a.M, out_cols);
    if (up) {
      o_lo = (int32_t)(((int64_t)m0 * a.new_u + a.orig_u - 1) / a.orig_u);
      o_hi = (int32_t)min(((int64_t)(m0 + a.M) * a.new_u + a.orig_u - 1) / a.orig_u, (int64_t)out_cols);
    }
    const bool live = m0 < L8;
    const int32_t q0 = m0 - halo_lo, q1 = m0 + a.M + halo_hi;  // q[] holds 8 kHz positions [q0, q1)
    const int32_t c_lo = max(q0, 0), c_hi = min(q1, L8);        // ... of which these are inside the row
    __syncthreads();  // the tables are in LDS; the previous tile's store has read the staging area
    if (live && filtered) {
      const int32_t in_lo = (c_lo / a.new_d) * a.orig_d + sd[c_lo % a.new_d];
      const int32_t in_hi = ((c_hi - 1) / a.new_d) * a.orig_d + sd[(c_hi - 1) % a.new_d] + a.W_d;
      const int32_t xb = ((in_lo + ax) & ~3) - ax;  // x + xb lies on a 16-byte boundary; xb > in_lo - 4
      for (int32_t i = xb + 4 * tid; i < in_hi; i += 4 * kNbThreads) {
        float4 v;
        if (i >= 0 && i + 4 <= n) {
          v = *reinterpret_cast<const float4*>(x + i);
        } else {
          v.x = (i >= 0 && i < n) ? x[i] : 0.0f;
          v.y = (i + 1 >= 0 && i + 1 < n) ? x[i + 1] : 0.0f;
          v.z = (i + 2 >= 0 && i + 2 < n) ? x[i + 2] : 0.0f;
          v.w = (i + 3 >= 0 && i + 3 < n) ? x[i + 3] : 0.0f;
        }
        *reinterpret_cast<float4*>(xs + (i - xb)) = v;  // (i - xb) is a multiple of 4, below span_cap
      }
      __syncthreads();
      nb_fir<true>(xs, xb, q, q0, c_lo, c_hi, wd, sd, a.np_d, a.W_d, a.orig_d, a.new_d);
    } else if (live) {
      for (int32_t s = c_lo + tid; s < c_hi; s += kNbThreads) q[s - q0] = nb_codec(x[s]);
    }
    if (live) {
      for (int32_t s = q0 + tid; s < q1; s += kNbThreads)
        if (s < 0 || s >= L8) q[s - q0] = 0.0f;
      __syncthreads();
      if (up) {
        nb_fir<false>(q, q0, xs, o_lo, o_lo, min(o_hi, n), wu, su, a.np_u, kNbUpTaps, a.orig_u, a.new_u);
        __syncthreads();
      }
    }
    // store [o_lo, o_hi): groups of four on the 16-byte boundaries of the output row, single samples at the edges
    const float* __restrict__ from = up ? xs : q;  // index o - o_lo
    const int32_t ob = ((o_lo + ao) & ~3) - ao;
    for (int32_t o = ob + 4 * tid; o < o_hi; o += 4 * kNbThreads) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = (live && o + k >= o_lo && o + k < min(o_hi, n_out)) ? from[o + k - o_lo] : 0.0f;
      if (o >= o_lo && o + 4 <= o_hi) {
        *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (o + k >= o_lo && o + k < o_hi) out[o + k] = v[k];
      }
    }
  }
}

}  // namespace hipfeat
