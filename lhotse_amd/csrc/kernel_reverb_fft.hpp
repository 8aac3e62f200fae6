// Reverberation by partitioned FFT convolution on the device: the opt-in second route of hipfeat_reverb (the direct form is
// kernel_reverb.hpp and stays the default).
//
// Reference: ReverbWithImpulseResponse.__call__ (lhotse/augmentation/rir.py:78-153) convolves through three float32 FFTs of size
// next_fast_len(N + L - 1) (convolve1d, lhotse/augmentation/utils.py:49-75).  Here the same product is taken block by block: uniformly
// partitioned overlap-save with block B = 1024 and transform size 2 B = 2048 -- the largest size of the wave-private transform
// (fft3_frame<16>, kernel_wave.hpp: 1024 complex points in three register passes, and the split step of kernel_stft.hpp; the way back is
// the adjoint real FFT of kernel_grad.hpp: the same passes on conjugated data).  One WAVE runs one transform and never synchronises with
// the rest of its workgroup behind the table load.  The geometry (partitions, input blocks, output blocks, the workspace formula) is in
// reverb_fft_tables.hpp.
//
// PRECISION.  The spectra are float32 and so is the accumulation; the input blocks are transformed in float32.  Two transforms run in
// float64 (fft3_frame_f64 and the split steps with a float64 W_2048^k table, kernel_grad.hpp) and round once, to float32, at their end: the
// RIR partitions (few, and every output passes through them) and the inverse transform.  Measured: with all three transforms in float32 a
// single-sample item (N = 1: the output is h[shift] x[0], which the reference's FFT of one sample returns almost exactly) was one ulp off
// and 1.18 x over the suite's bar; a numpy statement of the scheme put float32 transforms at up to 1.38 x on the N = 1 items of the test
// grid, float64 RIR spectra alone still at 1.38 x, float64 RIR spectra and inverse at 0.32 x (and the N >= 1023 items at 0.37 x, from 0.62 x).
//
// Four launches, stream-ordered, nothing visits the host in between:
//   * R, RIR spectra (rf_rir_*).  Work item w < rir_work: partition p of a distinct RIR, the taps hs[p B, (p + 1) B) zero-padded to 2048,
//     transformed in float64, stored as float32 in the layout of launch A.
//   * A, spectra (rf_spectra_*).  Work item rir_work <= w < a_work: input block i of an item, x[(i - 1) B, (i + 1) B), zeros outside
//     [0, N).  The 2048 real samples are the 1024 complex numbers
//     z[n] = v[2n] + i v[2n + 1]; fft3_frame and the split step give bins 0 ... 1024, unscaled; bin 0 is stored as (Re X_0, Re X_1024).
//     The spectrum leaves through the wave's LDS buffer as 16-byte stores.  Side output of an input block: the float64 sum of squares of
//     its NEW samples x[i B, (i + 1) B) -- a lane adds its 16 squares in ascending index order (fma), lanes -> wave by the fixed tree of
//     wave_sum_f64 -- one plain store to partials[w - rir_work].
//   * B, accumulate and invert (rf_output_*).  Work item = output block j of an item.  ACCUMULATION ORDER (part of the contract), float32:
//         Y = 0;  for p ascending over the p with 0 <= p < P and 0 <= j - p < nx, with h = H_p[k], x = X_{j-p}[k]:
//             Y.re = fmaf(-h.im, x.im, fmaf(h.re, x.re, Y.re));   Y.im = fmaf(h.im, x.re, fmaf(h.re, x.im, Y.im))          (bins 1 ... 1023)
//             Y.re = fmaf(h.re, x.re, Y.re);                      Y.im = fmaf(h.im, x.im, Y.im)       (bin 0: the two real bins 0 and 1024)
//     then the inverse real transform in float64 (adjoint split step, fft3_frame_f64 on the conjugate), one multiply by 2^-11, ONE
//     rounding to float32, and of its upper
//     1024 samples -- yf[j B, (j + 1) B) -- those inside [s, s + N) are stored at out[j B + t - s]: positions are counted from the
//     16-byte boundary at or below the block's first output, a lane owns whole 16-byte groups, a group inside the kept range is one 16-byte
//     store and the groups its ends cut are stored element by element.  Side output: the float64 sum of squares of what the block stored
//     -- a lane adds its squares in ascending position order, lanes -> wave by wave_sum_f64 -- to partials[x_total + work item].
//   * gain (rf_gain_*): a work item = kRvBlock (2048) outputs of an item; one lane adds the item's nx input partials and then its ny output
//     partials, each in index order (float64), g = (float)sqrt((Sx / N) / (Sy / N)), the workgroup scales its outputs in place with one
//     rounded multiply.  Items without normalisation, or with Sy <= 0, are left alone -- the statement of reverb_gain_body.
// An item's output depends on its own x, hs, N, L and shift alone: not on its neighbours, the grid, or the route its table took.  No
// atomics, no scratch; all element indexing is 64-bit.
//
// Work distribution and tables as kernel_reverb.hpp: flat lists of work items over a capped grid (launches A and B: kRfWaves = 4
// consecutive work items per workgroup trip, one per wave, over at most kRfGridSlots workgroups), the owner found by bisection over
// prefix sums; the table blob (RfItem[num_items] | RfRir[num_rirs]) in the kernel arguments when it fits kMbInlineBytes, through the
// shared staging slot otherwise.
#pragma once
#include "common.hpp"
#include "fft_common.hpp"
#include "kernel_grad.hpp"
#include "kernel_minibatch.hpp"
#include "kernel_stft.hpp"
#include "kernel_wave.hpp"
#include "reverb_fft_tables.hpp"

namespace hipfeat {

constexpr int kRfN1 = 16;                              // 64 x 16 = 1024 complex points
constexpr int kRfH = 64 * kRfN1;
constexpr int kRfBufFloats = 144 * kRfN1 + 8;          // per wave: the padded FFT buffer (and bin 1024 behind the natural-order spectrum)
constexpr size_t kRfMaxTableLds = kMbLdsTableBytes;    // dynamic LDS of the staged kernels at the most (with the static 53 KB: above 64 KB)
constexpr int kRfBuf64 = 72 * kRfN1 + 4;               // per wave, float64 kernels: the padded FFT buffer in complex doubles (bin 1024 included)
constexpr size_t kRfLds64 = sizeof(double) * 2 * (size_t)(kRfWaves * kRfBuf64 + kRfH);  // float64 kernels: four wave buffers + W_2048^k, dynamic

struct RfHeader {
  float* arena;
  double* partials;             // [x_total + b_work]
  const unsigned char* tables;  // staged blob (nullptr = inline)
  const float2* tw;             // W_2048^k, k < 1024
  const double2* tw64;          // the same in float64
  int32_t num_items, num_rirs, table_bytes, rir_work;
  int32_t a_work, b_work, g_work, x_total;
};
struct RfInlineArgs {
  RfHeader h;
  alignas(16) unsigned char blob[kMbInlineBytes];
};
static_assert(offsetof(RfInlineArgs, blob) % 16 == 0 && sizeof(RfInlineArgs) <= 3584, "kernel-argument layout");

template <typename T>
__device__ __forceinline__ T rf_uniform(const T* p) {  // every dword through v_readfirstlane (the index was wave-uniform)
  constexpr int W = (int)(sizeof(T) / sizeof(int));
  const int* w = reinterpret_cast<const int*>(p);
  union {
    int w[W];
    T t;
  } u;
#pragma unroll
  for (int i = 0; i < W; ++i) u.w[i] = __builtin_amdgcn_readfirstlane(w[i]);
  return u.t;
}

// the twiddles of both transforms to LDS, once per workgroup
__device__ __forceinline__ void rf_load_twiddles(const RfHeader& h, float2* tw, v2* twh) {
  for (int i = threadIdx.x; i < kRfH; i += 256) {
    tw[i] = h.tw[i];
    twh[i] = twiddle_h(h.tw, i, kRfH);
  }
  __syncthreads();
}

__device__ __forceinline__ void rf_spectra_body(const RfHeader& h, const unsigned char* tb, float* bufs, const float2* tw, const v2* twh) {
  const RfItem* its = reinterpret_cast<const RfItem*>(tb);
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* buf = bufs + wv * kRfBufFloats;
  v2* zf = reinterpret_cast<v2*>(buf);
  for (int64_t g = blockIdx.x; kRfWaves * g < h.x_total; g += gridDim.x) {
    const int w = h.rir_work + (int)(kRfWaves * g) + wv;  // (the work items below rir_work are launch R's)
    if (w >= h.a_work) break;  // (wave-uniform; no workgroup barrier behind this point)
    // the transform's 2048 samples: arena[s0 + m] for lo <= m < hi, zero elsewhere
    const RfItem it = rf_uniform(its + mb_owner(&its[0].a_first, (int)(sizeof(RfItem) / sizeof(int32_t)), h.num_items, w));
    const int i = w - it.a_first;
    const int64_t start = ((int64_t)i - 1) * kRfBlock;  // x index of sample 0
    const int64_t s0 = it.src_off + start, dst = it.xspec_off + (int64_t)i * kRfSpecFloats;
    const int lo = (int)max((int64_t)0, -start), hi = (int)min((int64_t)(2 * kRfBlock), (int64_t)it.n - start);
    double* sxp = h.partials + (w - h.rir_work);
    const float* __restrict__ src = h.arena;
    v2 xp[kRfN1];
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kRfN1; ++q) {
      const int m0 = 2 * (lane + 64 * q);
      v2 v = {0.f, 0.f};
      if (m0 >= lo && m0 + 2 <= hi) {
        __builtin_memcpy(&v, src + (s0 + m0), sizeof(v2));  // 4-byte aligned 8-byte load
      } else {
        if (m0 >= lo && m0 < hi) v.x = src[s0 + m0];
        if (m0 + 1 >= lo && m0 + 1 < hi) v.y = src[s0 + m0 + 1];
      }
      xp[q] = v;
      if (q >= kRfN1 / 2) {  // the block's new samples
        s = fma((double)v.x, (double)v.x, s);
        s = fma((double)v.y, (double)v.y, s);
      }
    }
    {
      const double total = wave_sum_f64(s);
      if (lane == 0) *sxp = total;
    }
    wave_lds_sync();  // the previous transform's readers of this wave's buffer are done
    fft3_frame<kRfN1>(zf, twh, lane, xp);
    // split step in place (kernel_stft.hpp): the lane that owns k reads and rewrites bins k and H - k; bin 0 becomes (X_0, X_H)
#pragma unroll
    for (int q = 0; q <= kRfN1 / 2; ++q) {
      const int k = lane + 64 * q;
      if (k <= kRfH / 2) {
        const v2 a = zf[k], b = zf[(kRfH - k) & (kRfH - 1)];
        const float ex = 0.5f * (a.x + b.x), ey = 0.5f * (a.y - b.y);
        const float ox = 0.5f * (a.y + b.y), oy = -0.5f * (a.x - b.x);
        const float2 wk = tw[k];
        const float tx = wk.x * ox - wk.y * oy, ty = wk.x * oy + wk.y * ox;
        const v2 first = {ex + tx, ey + ty}, second = {ex - tx, ty - ey};
        if (k == 0) {
          zf[0] = v2{first.x, second.x};
        } else {
          zf[k] = first;
          if (k < kRfH / 2) zf[kRfH - k] = second;
        }
      }
    }
    wave_lds_sync();
    float* __restrict__ out = h.arena + dst;
#pragma unroll
    for (int pp = 4 * lane; pp < kRfSpecFloats; pp += 256) *reinterpret_cast<f32x4*>(out + pp) = *reinterpret_cast<const f32x4*>(buf + pp);
  }
}

// Launch R: the spectra of the RIR partitions, in float64, rounded once.  bufs: kRfWaves x kRfBuf64 complex doubles; tw64: W_2048^k in LDS
__device__ __forceinline__ void rf_rir_body(const RfHeader& h, const unsigned char* tb, cd* bufs, const double2* tw64) {
  const RfRir* rirs = reinterpret_cast<const RfRir*>(tb + (size_t)h.num_items * sizeof(RfItem));
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  cd* zf = bufs + wv * kRfBuf64;
  for (int64_t g = blockIdx.x; kRfWaves * g < h.rir_work; g += gridDim.x) {
    const int w = (int)(kRfWaves * g) + wv;
    if (w >= h.rir_work) break;  // (wave-uniform; no workgroup barrier behind this point)
    const RfRir r = rf_uniform(rirs + mb_owner(&rirs[0].first, (int)(sizeof(RfRir) / sizeof(int32_t)), h.num_rirs, w));
    const int p = w - r.first;
    const float* __restrict__ src = h.arena + (r.rir_off + (int64_t)p * kRfBlock);
    const int hi = min(kRfBlock, r.taps - p * kRfBlock);  // taps of this partition; the samples from hi on are zeros
    cd xp[kRfN1];
#pragma unroll
    for (int q = 0; q < kRfN1; ++q) {
      const int m0 = 2 * (lane + 64 * q);
      xp[q] = cd{m0 < hi ? (double)src[m0] : 0.0, m0 + 1 < hi ? (double)src[m0 + 1] : 0.0};
    }
    wave_lds_sync();  // the previous transform's readers of this wave's buffer are done
    fft3_frame_f64<kRfN1>(zf, tw64, lane, xp);
    // split step in place, as in launch A: the lane that owns k reads and rewrites bins k and H - k; bin 0 becomes (X_0, X_H)
#pragma unroll
    for (int q = 0; q <= kRfN1 / 2; ++q) {
      const int k = lane + 64 * q;
      if (k <= kRfH / 2) {
        const cd a = zf[k], b = zf[(kRfH - k) & (kRfH - 1)];
        const double ex = 0.5 * (a.x + b.x), ey = 0.5 * (a.y - b.y);
        const double ox = 0.5 * (a.y + b.y), oy = -0.5 * (a.x - b.x);
        const double2 wk = tw64[k];
        const double tx = wk.x * ox - wk.y * oy, ty = wk.x * oy + wk.y * ox;
        const cd first = {ex + tx, ey + ty}, second = {ex - tx, ty - ey};
        if (k == 0) {
          zf[0] = cd{first.x, second.x};
        } else {
          zf[k] = first;
          if (k < kRfH / 2) zf[kRfH - k] = second;
        }
      }
    }
    wave_lds_sync();
    float* __restrict__ out = h.arena + (r.spec_off + (int64_t)p * kRfSpecFloats);
#pragma unroll
    for (int t = 0; t < kRfN1 / 2; ++t) {
      const int k0 = 2 * (lane + 64 * t);
      const cd u = zf[k0], v = zf[k0 + 1];
      *reinterpret_cast<f32x4*>(out + 2 * k0) = f32x4{(float)u.x, (float)u.y, (float)v.x, (float)v.y};
    }
  }
}

// Launch B.  bufs: kRfWaves x kRfBuf64 complex doubles; tw64: W_2048^k in LDS
__device__ __forceinline__ void rf_output_body(const RfHeader& h, const unsigned char* tb, cd* bufs, const double2* tw64) {
  const RfItem* its = reinterpret_cast<const RfItem*>(tb);
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  cd* zf = bufs + wv * kRfBuf64;
  for (int64_t g = blockIdx.x; kRfWaves * g < h.b_work; g += gridDim.x) {
    const int w = (int)(kRfWaves * g) + wv;
    if (w >= h.b_work) break;  // (wave-uniform)
    const RfItem it = rf_uniform(its + mb_owner(&its[0].b_first, (int)(sizeof(RfItem) / sizeof(int32_t)), h.num_items, w));
    const int j = it.j0 + (w - it.b_first);
    const int p_lo = max(0, j - it.nx + 1), p_hi = min(it.parts - 1, j);
    f32x4 acc[kRfN1 / 2];  // bins 2 (lane + 64 r) and the next one
#pragma unroll
    for (int r = 0; r < kRfN1 / 2; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int p = p_lo; p <= p_hi; ++p) {
      const f32x4* __restrict__ hp = reinterpret_cast<const f32x4*>(h.arena + (it.hspec_off + (int64_t)p * kRfSpecFloats));
      const f32x4* __restrict__ xq = reinterpret_cast<const f32x4*>(h.arena + (it.xspec_off + (int64_t)(j - p) * kRfSpecFloats));
#pragma unroll
      for (int r = 0; r < kRfN1 / 2; ++r) {
        const f32x4 a = hp[lane + 64 * r], b = xq[lane + 64 * r];
        const float re0 = fmaf(a.x, b.x, acc[r].x);
        const bool packed = r == 0 && lane == 0;  // bin 0 holds the two real bins 0 and 1024
        acc[r].x = packed ? re0 : fmaf(-a.y, b.y, re0);
        acc[r].y = packed ? fmaf(a.y, b.y, acc[r].y) : fmaf(a.y, b.x, fmaf(a.x, b.y, acc[r].y));
        acc[r].z = fmaf(-a.w, b.w, fmaf(a.z, b.z, acc[r].z));
        acc[r].w = fmaf(a.w, b.z, fmaf(a.z, b.w, acc[r].w));
      }
    }
    // ---- the inverse real transform (kernel_grad.hpp's adjoint with Y_k = the bins themselves): Y into LDS, Q_k from Y_k and Y_{H-k} ----
    wave_lds_sync();  // the previous block's readers of this wave's buffer are done
    // (float64 from here to the one rounding of the output)
#pragma unroll
    for (int r = 0; r < kRfN1 / 2; ++r) {
      const f32x4 y = acc[r];
      const int k0 = 2 * (lane + 64 * r);
      if (r == 0 && lane == 0) {
        zf[kRfH] = cd{(double)y.y, 0.0};
        zf[0] = cd{(double)y.x, 0.0};
      } else {
        zf[k0] = cd{(double)y.x, (double)y.y};
      }
      zf[k0 + 1] = cd{(double)y.z, (double)y.w};
    }
    wave_lds_sync();
    cd qc[kRfN1];
#pragma unroll
    for (int q = 0; q < kRfN1; ++q) {
      const int k = lane + 64 * q;
      const cd a = zf[k], b0 = zf[kRfH - k];
      const cd b = {b0.x, -b0.y};
      const double2 wk = tw64[k];  // e^{+i pi k / H} = (wk.x, -wk.y)
      const double c = wk.x, s = -wk.y;
      const double dx = a.x - b.x, dy = a.y - b.y;
      const double qx = a.x + b.x - (c * dy + s * dx), qy = a.y + b.y + (c * dx - s * dy);
      qc[q] = cd{qx, -qy};
    }
    wave_lds_sync();  // every lane has read Y
    fft3_frame_f64<kRfN1>(zf, tw64, lane, qc);
    // zf[n] = 2048 (v[2n] - i v[2n + 1]).  v[B + t] = yf[j B + t] goes to out[d0 + t] where 0 <= d0 + t < N.
    const int64_t d0 = (int64_t)j * kRfBlock - it.shift;
    const int head = (int)(d0 & 3);  // out is 16-byte aligned: d0 + t sits on a 16-byte boundary when (t + head) % 4 == 0
    float* __restrict__ out = h.arena + it.out_off;
    constexpr double kScale = 1.0 / (double)(2 * kRfBlock);
    double sy = 0.0;
    for (int pp = 4 * lane; pp < head + kRfBlock; pp += 256) {
      float e[4];
      bool ok[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = pp + i - head;
        const int64_t o = d0 + t;
        ok[i] = t >= 0 && t < kRfBlock && o >= 0 && o < (int64_t)it.n;
        const cd z = zf[(kRfBlock + (ok[i] ? t : 0)) >> 1];
        e[i] = (float)(((t & 1) ? -z.y : z.x) * kScale);
        if (ok[i]) sy = fma((double)e[i], (double)e[i], sy);
      }
      const int64_t o0 = d0 + (pp - head);
      if (ok[0] && ok[1] && ok[2] && ok[3]) {
        *reinterpret_cast<f32x4*>(out + o0) = f32x4{e[0], e[1], e[2], e[3]};
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (ok[i]) out[o0 + i] = e[i];
      }
    }
    const double total = wave_sum_f64(sy);
    if (lane == 0) h.partials[(int64_t)h.x_total + w] = total;
  }
}

// p[0] + p[1] + ... in index order, by one lane; the loads are issued eight at a time so that their latencies overlap (a 200 000-sample
// item has ~400 partials, and every one of its ~100 gain work items adds them all)
__device__ __forceinline__ double rf_ordered_sum(const double* __restrict__ p, int n) {
  double s = 0.0;
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = p[k + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v[i];
  }
  for (; k < n; ++k) s += p[k];
  return s;
}

__device__ __forceinline__ void rf_gain_body(const RfHeader& h, const unsigned char* tb, float* gain) {
  const RfItem* its = reinterpret_cast<const RfItem*>(tb);
  const int tid = threadIdx.x;
  for (int item = blockIdx.x; item < h.g_work; item += gridDim.x) {
    const int i = mb_owner(&its[0].g_first, (int)(sizeof(RfItem) / sizeof(int32_t)), h.num_items, item);
    const RfItem it = rf_uniform(its + i);
    if (!it.normalize) continue;  // (workgroup-uniform)
    __syncthreads();              // the previous work item's gain has been read
    if (tid == 0) {
      const double* __restrict__ px = h.partials + (it.a_first - h.rir_work);
      const double* __restrict__ py = h.partials + ((int64_t)h.x_total + it.b_first);
      const double sx = rf_ordered_sum(px, it.nx), sy = rf_ordered_sum(py, it.ny);
      // (rir.py:148-151; P_out <= 0 or not a number: the samples stay as they are)
      gain[0] = sy > 0.0 ? (float)sqrt((sx / (double)it.n) / (sy / (double)it.n)) : 1.0f;
      gain[1] = sy > 0.0 ? 1.0f : 0.0f;
    }
    __syncthreads();
    if (gain[1] == 0.0f) continue;
    const float g = gain[0];
    const int n0 = (item - it.g_first) * kRvBlock + kRvLane * tid;
    float* __restrict__ out = h.arena + it.out_off;
    if (n0 + kRvLane <= it.n) {
      float4 a = reinterpret_cast<float4*>(out + n0)[0], b = reinterpret_cast<float4*>(out + n0)[1];
      a = make_float4(__fmul_rn(a.x, g), __fmul_rn(a.y, g), __fmul_rn(a.z, g), __fmul_rn(a.w, g));
      b = make_float4(__fmul_rn(b.x, g), __fmul_rn(b.y, g), __fmul_rn(b.z, g), __fmul_rn(b.w, g));
      reinterpret_cast<float4*>(out + n0)[0] = a;
      reinterpret_cast<float4*>(out + n0)[1] = b;
    } else {
#pragma unroll
      for (int j = 0; j < kRvLane; ++j)
        if (n0 + j < it.n) out[n0 + j] = __fmul_rn(out[n0 + j], g);
    }
  }
}

// LDS of launches A and B: four wave buffers, the two twiddle tables, then the tables
#define RF_TRANSFORM_LDS                                                  \
  __shared__ __attribute__((aligned(16))) float bufs[kRfWaves * kRfBufFloats]; \
  __shared__ __attribute__((aligned(16))) float2 tw[kRfH];                 \
  __shared__ __attribute__((aligned(16))) v2 twh[kRfH]

__global__ __launch_bounds__(256, 2) void rf_spectra_inline_kernel(const RfInlineArgs a) {
  RF_TRANSFORM_LDS;
  __shared__ __attribute__((aligned(16))) unsigned char tb[kMbInlineBytes];
  mb_inline_tables(tb, a.h.table_bytes, offsetof(RfInlineArgs, blob));
  rf_load_twiddles(a.h, tw, twh);
  rf_spectra_body(a.h, tb, bufs, tw, twh);
}

__global__ __launch_bounds__(256, 2) void rf_spectra_kernel(const RfHeader h) {
  RF_TRANSFORM_LDS;
  extern __shared__ __attribute__((aligned(16))) unsigned char rf_tb_dyn[];
  const unsigned char* tb = mb_staged_tables(h.tables, h.table_bytes, rf_tb_dyn);
  rf_load_twiddles(h, tw, twh);
  rf_spectra_body(h, tb, bufs, tw, twh);
}

#undef RF_TRANSFORM_LDS

// The float64 launches (R and B).  Their LDS is dynamic: kRfLds64 bytes (four wave buffers of kRfBuf64 complex doubles, then W_2048^k in
// float64), and behind them the staged table when it is searched in LDS.
__device__ __forceinline__ const double2* rf_load_tw64(const RfHeader& h, unsigned char* dyn) {
  double2* tw64 = reinterpret_cast<double2*>(dyn + sizeof(cd) * kRfWaves * kRfBuf64);
  for (int i = threadIdx.x; i < kRfH; i += 256) tw64[i] = h.tw64[i];
  __syncthreads();
  return tw64;
}

__global__ __launch_bounds__(256, 1) void rf_rir_inline_kernel(const RfInlineArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rf_tb_dyn[];
  __shared__ __attribute__((aligned(16))) unsigned char tb[kMbInlineBytes];
  mb_inline_tables(tb, a.h.table_bytes, offsetof(RfInlineArgs, blob));
  const double2* tw64 = rf_load_tw64(a.h, rf_tb_dyn);
  rf_rir_body(a.h, tb, reinterpret_cast<cd*>(rf_tb_dyn), tw64);
}

__global__ __launch_bounds__(256, 1) void rf_rir_kernel(const RfHeader h) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rf_tb_dyn[];
  const unsigned char* tb = mb_staged_tables(h.tables, h.table_bytes, rf_tb_dyn + kRfLds64);
  const double2* tw64 = rf_load_tw64(h, rf_tb_dyn);
  rf_rir_body(h, tb, reinterpret_cast<cd*>(rf_tb_dyn), tw64);
}

__global__ __launch_bounds__(256, 1) void rf_output_inline_kernel(const RfInlineArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rf_tb_dyn[];
  __shared__ __attribute__((aligned(16))) unsigned char tb[kMbInlineBytes];
  mb_inline_tables(tb, a.h.table_bytes, offsetof(RfInlineArgs, blob));
  const double2* tw64 = rf_load_tw64(a.h, rf_tb_dyn);
  rf_output_body(a.h, tb, reinterpret_cast<cd*>(rf_tb_dyn), tw64);
}

__global__ __launch_bounds__(256, 1) void rf_output_kernel(const RfHeader h) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rf_tb_dyn[];
  const unsigned char* tb = mb_staged_tables(h.tables, h.table_bytes, rf_tb_dyn + kRfLds64);
  const double2* tw64 = rf_load_tw64(h, rf_tb_dyn);
  rf_output_body(h, tb, reinterpret_cast<cd*>(rf_tb_dyn), tw64);
}

__global__ __launch_bounds__(256) void rf_gain_inline_kernel(const RfInlineArgs a) {
  __shared__ float gain[2];
  __shared__ __attribute__((aligned(16))) unsigned char tb[kMbInlineBytes];
  mb_inline_tables(tb, a.h.table_bytes, offsetof(RfInlineArgs, blob));
  rf_gain_body(a.h, tb, gain);
}

__global__ __launch_bounds__(256) void rf_gain_kernel(const RfHeader h) {
  __shared__ float gain[2];
  extern __shared__ __attribute__((aligned(16))) unsigned char rf_tb_dyn[];
  rf_gain_body(h, mb_staged_tables(h.tables, h.table_bytes, rf_tb_dyn), gain);
}

}  // namespace hipfeat
