// Reverberation with a recorded room impulse response on the device, in front of the mix and the feature launch.
//
// Reference: ReverbWithImpulseResponse.__call__ (lhotse/augmentation/rir.py:78-153) scales the RIR by 2^-15, convolves the whole signal
// with it through three float32 FFTs of size next_fast_len(N + L - 1) (convolve1d, lhotse/augmentation/utils.py:49-75), keeps the N samples
// from shift = argmax(rir) on ("shift output") and, with normalize_output, scales them so that the power of the input is kept.
//
// One (input channel, RIR channel) pair is an ITEM {source, N, RIR (already scaled, hs = rir * 2^-15), L, shift, normalise flag}:
//   y[n] = sum_k hs[k] * x[n + shift - k],  0 <= n < N, over the k with 0 <= n + shift - k < N
//   normalise:  Sx = sum x^2, Sy = sum y^2 (float64);  if Sy > 0:  y *= (float)sqrt((Sx / N) / (Sy / N))
//
// Two launches, stream-ordered, nothing visits the host in between:
//   * convolution: a work item = kRvBlock (2048) consecutive outputs of one item; every lane owns kRvLane (8) CONSECUTIVE outputs
//     n = base + 8 * lane + j and keeps their sums in registers.  The taps are taken in chunks of kRvChunk (256) consecutive taps
//     [256 c, 256 c + 256): per chunk the workgroup stages the x window the block's outputs need for these taps (2048 + 255 samples,
//     zero outside [0, N)) and the chunk's taps (zero behind L) in LDS, then every lane runs over the taps in ascending order, 8 at a
//     time: two ds_read_b128 of x (a 16-sample register window slides down by 8 per step; the upper half is the previous step's lower
//     half, so it is not read again), two broadcast ds_read_b128 of taps (wave-uniform address), 64 v_fma_f32.
//     SUMMATION ORDER (part of the contract, the accuracy bar depends on it), all float32:
//         q_s = 0;  for k = 16 s ... 16 s + 15 ascending:  q_s = fmaf(hs[k], x[n + shift - k], q_s)   (a term outside the signal or behind L
//                                                                                                       is fmaf(., 0, q) or fmaf(0, ., q) = q)
//         p_c = 0;  for s = 16 c ... 16 c + 15 ascending:  p_c = p_c + q_s                              (the 256 taps [256 c, 256 c + 256))
//         y = 0;    for c = 0, 1, ... ascending:           y = y + p_c
//     i.e. partial sums of 256 consecutive taps, added in ascending order, each of them the ascending sum of its 16 runs of 16 taps.  Measured
//     against the exact float64 convolution on the grid of tests/test_gpu_reverb.py (tests/_reverb_ref.py states the same order in numpy): one
//     chain per 256 taps is up to 1.9 x the suite's max-abs bar at N, L <= 256, where the reference's FFT is small and accurate; the runs of 16
//     bring that to <= 0.7 x for one v_add_f32 per 16 v_fma_f32; one serial chain over all L taps is 3-16 x less accurate than the reference.
//     The result of an output depends on its item's x, hs, N, L and shift alone.
//     Side outputs: the block's sums of squares of its x segment and of its y segment (float64, squares of float32 are exact in it), lanes
//     -> wave by a fixed shuffle tree, waves -> workgroup in index order, two plain stores to partials[2 * work item + {0, 1}]; no atomics.
//   * gain: a work item = the same 2048 outputs; one lane adds the item's partials in index order (float64), rounds the gain to float32,
//     the workgroup scales its outputs in place (one rounded multiply).  Items without normalisation, or with Sy <= 0, are left alone.
//
// Work distribution and tables as kernel_mix.hpp / kernel_minibatch.hpp: one flat list of work items over a grid of a few workgroups per
// CU, the owner of a work item found by bisection over the prefix sums (RvItem::item_first) in LDS; the table (RvItem[num_items]) travels
// in the kernel arguments when it fits kMbInlineBytes (69 items) and through pinned memory otherwise.
#pragma once
#include "common.hpp"
#include "kernel_minibatch.hpp"
#include "reverb_tables.hpp"

namespace hipfeat {

struct RvHeader {
  float* arena;
  double* partials;             // [2 * work_items]: {sum x^2, sum y^2} per work item
  const unsigned char* tables;  // staged blob (nullptr = inline)
  int32_t num_items, work_items, table_bytes, pad;
};
struct RvInlineArgs {
  RvHeader h;
  alignas(16) unsigned char blob[kMbInlineBytes];
};
static_assert(offsetof(RvInlineArgs, blob) % 16 == 0 && sizeof(RvInlineArgs) <= 3584, "kernel-argument layout");

__device__ __forceinline__ RvItem rv_uniform(const RvItem* p) {  // every dword through v_readfirstlane (the index was workgroup-uniform)
  const int* w = reinterpret_cast<const int*>(p);
  union {
    int w[12];
    RvItem t;
  } u;
#pragma unroll
  for (int i = 0; i < 12; ++i) u.w[i] = __builtin_amdgcn_readfirstlane(w[i]);
  return u.t;
}

// 8 taps t[0..7] = hs[k .. k + 7] against the 16-sample window {lo, hi}: output j, tap k + i reads window[j - i + 7]
__device__ __forceinline__ void rv_mac(float (&p)[kRvLane], const float4& lo0, const float4& lo1, const float4& hi0, const float4& hi1, const float4& t0,
                                       const float4& t1) {
  const float w[16] = {lo0.x, lo0.y, lo0.z, lo0.w, lo1.x, lo1.y, lo1.z, lo1.w, hi0.x, hi0.y, hi0.z, hi0.w, hi1.x, hi1.y, hi1.z, hi1.w};
  const float t[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < kRvLane; ++j) p[j] = fmaf(t[i], w[j - i + 7], p[j]);
}

// lanes -> wave (fixed tree), waves -> workgroup (index order): the same order in every run
__device__ __forceinline__ double rv_block_sum(double v, double* red) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  __syncthreads();  // red's previous readers are done
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// xs: kRvWindow floats, hs: kRvChunk floats (both 16-byte aligned), red: 4 doubles
__device__ __forceinline__ void reverb_conv_body(const RvHeader& h, const unsigned char* tb, float* xs, float* hs, double* red) {
  const RvItem* its = reinterpret_cast<const RvItem*>(tb);
  const int tid = threadIdx.x;
  for (int item = blockIdx.x; item < h.work_items; item += gridDim.x) {
    const int i = mb_owner(&its[0].item_first, (int)(sizeof(RvItem) / sizeof(int32_t)), h.num_items, item);
    const RvItem it = rv_uniform(its + i);
    const int base = (item - it.item_first) * kRvBlock;
    const float* __restrict__ x = h.arena + it.src_off;
    const float* __restrict__ r = h.arena + it.rir_off;
    float y[kRvLane];
#pragma unroll
    for (int j = 0; j < kRvLane; ++j) y[j] = 0.0f;
    const int chunks = (it.taps + kRvChunk - 1) / kRvChunk;
    for (int c = 0; c < chunks; ++c) {
      const int k0 = c * kRvChunk;
      const int w0 = base + it.shift - k0 - (kRvChunk - 1);  // the sample xs[0] holds: output base, tap k0 + 255
      __syncthreads();                                       // the previous chunk (or work item) has been read
#pragma unroll
      for (int q = tid; q < kRvWindow; q += 256) {
        const int xi = w0 + q;
        xs[q] = ((unsigned)xi < (unsigned)it.n) ? x[xi] : 0.0f;
      }
      hs[tid] = (k0 + tid < it.taps) ? r[k0 + tid] : 0.0f;
      __syncthreads();
      const int pairs = (min(kRvChunk, it.taps - k0) + 15) >> 4;  // 16 taps per trip; the taps behind L are zeros
      float p[kRvLane];
#pragma unroll
      for (int j = 0; j < kRvLane; ++j) p[j] = 0.0f;
      // lane's window for taps k0 + 8 g ... + 7 = xs[8 tid + 248 - 8 g ... + 15]
      const float4* xw = reinterpret_cast<const float4*>(xs + kRvLane * tid);
      const float4* tw = reinterpret_cast<const float4*>(hs);
      float4 h0 = xw[64], h1 = xw[65], a0, a1;
      for (int g = 0; g < 2 * pairs; g += 2) {
        float q[kRvLane];  // the run of 16 taps
#pragma unroll
        for (int j = 0; j < kRvLane; ++j) q[j] = 0.0f;
        a0 = xw[62 - 2 * g], a1 = xw[63 - 2 * g];
        rv_mac(q, a0, a1, h0, h1, tw[2 * g], tw[2 * g + 1]);
        h0 = xw[60 - 2 * g], h1 = xw[61 - 2 * g];
        rv_mac(q, h0, h1, a0, a1, tw[2 * g + 2], tw[2 * g + 3]);
#pragma unroll
        for (int j = 0; j < kRvLane; ++j) p[j] = __fadd_rn(p[j], q[j]);
      }
#pragma unroll
      for (int j = 0; j < kRvLane; ++j) y[j] = __fadd_rn(y[j], p[j]);
    }
    const int n0 = base + kRvLane * tid;
    float* __restrict__ out = h.arena + it.out_off;
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int j = 0; j < kRvLane; ++j)
      if (n0 + j < it.n) {
        const double xv = (double)x[n0 + j], yv = (double)y[j];
        sx = fma(xv, xv, sx);
        sy = fma(yv, yv, sy);
      }
    if (n0 + kRvLane <= it.n) {
      reinterpret_cast<float4*>(out + n0)[0] = make_float4(y[0], y[1], y[2], y[3]);
      reinterpret_cast<float4*>(out + n0)[1] = make_float4(y[4], y[5], y[6], y[7]);
    } else {
#pragma unroll
      for (int j = 0; j < kRvLane; ++j)
        if (n0 + j < it.n) out[n0 + j] = y[j];
    }
    const double bx = rv_block_sum(sx, red);
    const double by = rv_block_sum(sy, red);
    if (tid == 0) {
      h.partials[2 * (int64_t)item] = bx;
      h.partials[2 * (int64_t)item + 1] = by;
    }
  }
}

__device__ __forceinline__ void reverb_gain_body(const RvHeader& h, const unsigned char* tb, float* gain) {
  const RvItem* its = reinterpret_cast<const RvItem*>(tb);
  const int tid = threadIdx.x;
  for (int item = blockIdx.x; item < h.work_items; item += gridDim.x) {
    const int i = mb_owner(&its[0].item_first, (int)(sizeof(RvItem) / sizeof(int32_t)), h.num_items, item);
    const RvItem it = rv_uniform(its + i);
    if (!it.normalize) continue;  // (workgroup-uniform)
    __syncthreads();              // the previous work item's gain has been read
    if (tid == 0) {
      const int blocks = (it.n + kRvBlock - 1) / kRvBlock;
      const double* __restrict__ part = h.partials + 2 * (int64_t)it.item_first;
      double sx = 0.0, sy = 0.0;
      for (int k = 0; k < blocks; ++k) {
        sx += part[2 * k];
        sy += part[2 * k + 1];
      }
      // (rir.py:148-151; P_out <= 0 or not a number: the samples stay as they are)
      gain[0] = sy > 0.0 ? (float)sqrt((sx / (double)it.n) / (sy / (double)it.n)) : 1.0f;
      gain[1] = sy > 0.0 ? 1.0f : 0.0f;
    }
    __syncthreads();
    if (gain[1] == 0.0f) continue;
    const float g = gain[0];
    const int n0 = (item - it.item_first) * kRvBlock + kRvLane * tid;
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

__global__ __launch_bounds__(256) void reverb_conv_inline_kernel(const RvInlineArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[kRvWindow];
  __shared__ __attribute__((aligned(16))) float hs[kRvChunk];
  __shared__ double red[4];
  __shared__ __attribute__((aligned(16))) unsigned char tb[kMbInlineBytes];
  mb_inline_tables(tb, a.h.table_bytes, offsetof(RvInlineArgs, blob));
  reverb_conv_body(a.h, tb, xs, hs, red);
}

__global__ __launch_bounds__(256) void reverb_conv_kernel(const RvHeader h) {
  __shared__ __attribute__((aligned(16))) float xs[kRvWindow];
  __shared__ __attribute__((aligned(16))) float hs[kRvChunk];
  __shared__ double red[4];
  extern __shared__ __attribute__((aligned(16))) unsigned char reverb_tb_dyn[];
  reverb_conv_body(h, mb_staged_tables(h.tables, h.table_bytes, reverb_tb_dyn), xs, hs, red);
}

__global__ __launch_bounds__(256) void reverb_gain_inline_kernel(const RvInlineArgs a) {
  __shared__ float gain[2];
  __shared__ __attribute__((aligned(16))) unsigned char tb[kMbInlineBytes];
  mb_inline_tables(tb, a.h.table_bytes, offsetof(RvInlineArgs, blob));
  reverb_gain_body(a.h, tb, gain);
}

__global__ __launch_bounds__(256) void reverb_gain_kernel(const RvHeader h) {
  __shared__ float gain[2];
  extern __shared__ __attribute__((aligned(16))) unsigned char reverb_tb_dyn[];
  reverb_gain_body(h, mb_staged_tables(h.tables, h.table_bytes, reverb_tb_dyn), gain);
}

}  // namespace hipfeat
