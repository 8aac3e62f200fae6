// Level changes of cuts on the device (PerturbVolume, Clipping), between the speed pass, the reverb and the mix.
//
// Reference: Volume.__call__ (lhotse/augmentation/torchaudio.py:395-406) multiplies the float32 samples by (float)factor;
// Clipping.__call__ (lhotse/augmentation/clipping.py:28-61) takes p = np.max(np.abs(samples)), returns the samples as they are when
// p == 0 or 20 * log10(p) < -96, and otherwise computes, every step a float32 array operation,
//   [samples / p]  [* g]  np.clip(., -1, 1) | np.tanh  [/ g]  [* p]          g = (float)10^(gain_db / 20), used when |gain_db| >= 0.1.
//
// An ITEM (level_tables.hpp) is a run of samples with a PROGRAM of 1 ... 4 such ops, applied to every sample in order, at most one CLIP.
// Two launches, stream-ordered, nothing visits the host in between:
//   * peak: a work item = one tile of kLvBlock samples of an item whose program has a CLIP; it writes max |x| of the tile's SOURCE samples
//     to partials[work item] with a plain store.  A maximum does not depend on the order it is taken in, so any reduction shape gives
//     the same bits and a run repeats bit for bit.  Items without a CLIP are skipped.
//   * apply: a work item = the same tile.  The workgroup takes the maximum of its item's partials, then pushes it through the SCALE ops
//     in front of the CLIP with the same float32 multiplications the samples go through:  p = fl(fl(peak * |f1|) * |f2|).  This IS the
//     maximum of the scaled samples, exactly: x -> fl(x * f) is monotone in |x| (rounding to nearest is monotone) and odd
//     (fl(-x) = -fl(x)), so max_i |fl(x_i * f)| = fl(max_i |x_i| * |f|) -- no second pass over the samples is needed
//     (tests/test_level_reference.py checks the identity on random data).  Then every lane takes 4 x 4 consecutive samples through the
//     program and stores them.  Divisions are IEEE divisions (no reciprocal, no fast-math), products are rounded one by one, and the
//     soft clip is the float64 tanh rounded once to float32 (<= 0.5 ulp + 2^-53 relative: at least as close to the exact value as
//     any float32 evaluation).  A NaN sample does not raise the peak here (np.max would return NaN and spread it over the whole item).
//
// Tiles are counted from the 16-byte boundary at or below the item's source (the arena itself starts on one), so a group of 4 samples
// that lies wholly inside the item is read with one 16-byte load whatever the source offset is; it is stored with one 16-byte store
// when the destination has the same offset modulo 4 (always so in place), sample by sample otherwise.  The groups that the item's
// first and last sample cut are handled sample by sample: the scalar head and tail.  One long item spreads over many workgroups.
// In place every sample is read and written by the same lane of the same work item, after the peak launch has finished.
//
// Work distribution and tables as kernel_reverb.hpp / kernel_mix.hpp: one flat list of work items over a grid of a few workgroups per
// CU, the owner of a work item found by bisection over the prefix sums (LvItem::item_first) in LDS; the table (LvItem[num_items])
// travels in the kernel arguments when it fits kMbInlineBytes (52 items) and through pinned memory otherwise.
#pragma once
#include "common.hpp"
#include "kernel_minibatch.hpp"
#include "level_tables.hpp"

namespace hipfeat {

struct LvHeader {
  float* arena;
  float* partials;              // [work_items]: max |x| per work item (items with a CLIP)
  const unsigned char* tables;  // staged table (nullptr = inline)
  int32_t num_items, work_items, table_bytes, pad;
};
struct LvInlineArgs {
  LvHeader h;
  alignas(16) unsigned char blob[kMbInlineBytes];
};
static_assert(offsetof(LvInlineArgs, blob) % 16 == 0 && sizeof(LvInlineArgs) <= 3584, "kernel-argument layout");

__device__ __forceinline__ LvItem lv_uniform(const LvItem* p) {  // every dword through v_readfirstlane (the index was workgroup-uniform)
  const int* w = reinterpret_cast<const int*>(p);
  union {
    int w[16];
    LvItem t;
  } u;
#pragma unroll
  for (int i = 0; i < 16; ++i) u.w[i] = __builtin_amdgcn_readfirstlane(w[i]);
  return u.t;
}

// lanes -> wave -> workgroup; every lane returns the workgroup's maximum
__device__ __forceinline__ float lv_block_max(float v, float* red) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_down(v, d, 64));
  __syncthreads();  // red's previous readers are done
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__device__ __forceinline__ void level_peak_body(const LvHeader& h, const unsigned char* tb, float* red) {
  const LvItem* its = reinterpret_cast<const LvItem*>(tb);
  const int tid = threadIdx.x;
  for (int item = blockIdx.x; item < h.work_items; item += gridDim.x) {
    const int i = mb_owner(&its[0].item_first, (int)(sizeof(LvItem) / sizeof(int32_t)), h.num_items, item);
    const LvItem it = lv_uniform(its + i);
    if (it.clip_at < 0) continue;  // (workgroup-uniform)
    const int head = (int)(it.src_off & 3), end = head + it.len;  // the item is [head, end) counted from its 16-byte boundary
    const float* __restrict__ xb = h.arena + (it.src_off - head);
    const int v0 = (item - it.item_first) * kLvBlock;
    float m = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = v0 + 4 * (tid + 256 * k);
      if (v >= head && v + 3 < end) {
        const float4 q = *reinterpret_cast<const float4*>(xb + v);
        m = fmaxf(m, fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fmaxf(fabsf(q.z), fabsf(q.w))));
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (v + j >= head && v + j < end) m = fmaxf(m, fabsf(xb[v + j]));
      }
    }
    m = lv_block_max(m, red);
    if (tid == 0) h.partials[item] = m;
  }
}

// one sample through the program; p: the CLIP's peak, clip: whether the CLIP acts (its input is not silence)
__device__ __forceinline__ float lv_program(float v, const LvItem& it, float p, bool clip) {
#pragma unroll
  for (int k = 0; k < kLvMaxOps; ++k) {  // (unrolled: the descriptor stays in scalar registers; the trip count is wave-uniform)
    if (k >= it.nops) break;
    const float a = it.value[k];
    if ((it.op[k] & 255) == kLvScale) {
      v = __fmul_rn(v, a);
    } else if (clip) {
      const int flags = it.op[k] >> 8;
      if (flags & kLvNormalize) v = __fdiv_rn(v, p);
      if (flags & kLvUseGain) v = __fmul_rn(v, a);
      v = (flags & kLvHard) ? fminf(fmaxf(v, -1.0f), 1.0f) : (float)tanh((double)v);
      if (flags & kLvUseGain) v = __fdiv_rn(v, a);
      if (flags & kLvNormalize) v = __fmul_rn(v, p);
    }
  }
  return v;
}

__device__ __forceinline__ void level_apply_body(const LvHeader& h, const unsigned char* tb, float* red) {
  const LvItem* its = reinterpret_cast<const LvItem*>(tb);
  const int tid = threadIdx.x;
  for (int item = blockIdx.x; item < h.work_items; item += gridDim.x) {
    const int i = mb_owner(&its[0].item_first, (int)(sizeof(LvItem) / sizeof(int32_t)), h.num_items, item);
    const LvItem it = lv_uniform(its + i);
    const int head = (int)(it.src_off & 3), end = head + it.len;
    float p = 0.0f;
    if (it.clip_at >= 0) {  // (workgroup-uniform)
      const int blocks = (end + kLvBlock - 1) / kLvBlock;
      const float* __restrict__ part = h.partials + it.item_first;
      float m = 0.0f;
      for (int k = tid; k < blocks; k += 256) m = fmaxf(m, part[k]);
      p = lv_block_max(m, red);
#pragma unroll
      for (int k = 0; k < kLvMaxOps - 1; ++k)  // the ops in front of the CLIP are SCALEs
        if (k < it.clip_at) p = __fmul_rn(p, fabsf(it.value[k]));
    }
    const bool clip = !(p == 0.0f || p < kLvSilencePeak);  // (clipping.py:36)
    const float* __restrict__ xb = h.arena + (it.src_off - head);
    float* y = h.arena + it.dst_off;  // sample s of the item goes to y[s], s = v - head
    const bool vec_store = (int)(it.dst_off & 3) == head;
    const int v0 = (item - it.item_first) * kLvBlock;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = v0 + 4 * (tid + 256 * k);
      if (v >= head && v + 3 < end) {
        float4 q = *reinterpret_cast<const float4*>(xb + v);
        q.x = lv_program(q.x, it, p, clip);
        q.y = lv_program(q.y, it, p, clip);
        q.z = lv_program(q.z, it, p, clip);
        q.w = lv_program(q.w, it, p, clip);
        if (vec_store) {
          *reinterpret_cast<float4*>(y + (v - head)) = q;
        } else {
          y[v - head] = q.x;
          y[v - head + 1] = q.y;
          y[v - head + 2] = q.z;
          y[v - head + 3] = q.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (v + j >= head && v + j < end) y[v + j - head] = lv_program(xb[v + j], it, p, clip);
      }
    }
  }
}

__global__ __launch_bounds__(256) void level_peak_inline_kernel(const LvInlineArgs a) {
  __shared__ float red[4];
  __shared__ __attribute__((aligned(16))) unsigned char tb[kMbInlineBytes];
  mb_inline_tables(tb, a.h.table_bytes, offsetof(LvInlineArgs, blob));
  level_peak_body(a.h, tb, red);
}

__global__ __launch_bounds__(256) void level_peak_kernel(const LvHeader h) {
  __shared__ float red[4];
  extern __shared__ __attribute__((aligned(16))) unsigned char level_tb_dyn[];
  level_peak_body(h, mb_staged_tables(h.tables, h.table_bytes, level_tb_dyn), red);
}

__global__ __launch_bounds__(256) void level_apply_inline_kernel(const LvInlineArgs a) {
  __shared__ float red[4];
  __shared__ __attribute__((aligned(16))) unsigned char tb[kMbInlineBytes];
  mb_inline_tables(tb, a.h.table_bytes, offsetof(LvInlineArgs, blob));
  level_apply_body(a.h, tb, red);
}

__global__ __launch_bounds__(256) void level_apply_kernel(const LvHeader h) {
  __shared__ float red[4];
  extern __shared__ __attribute__((aligned(16))) unsigned char level_tb_dyn[];
  level_apply_body(h, mb_staged_tables(h.tables, h.table_bytes, level_tb_dyn), red);
}

}  // namespace hipfeat
