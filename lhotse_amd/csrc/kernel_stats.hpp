// Global feature statistics (GlobalMVN estimation) on the device: per-bin sum and unnormalised variance of the frames of many cuts.
//
// Reference: CutSet.compute_global_feature_stats (lhotse/cut/set.py:2533-2583) calls StatsAccumulator.update
// (lhotse/features/base.py:990-1033) once per cut: curr_sum = sum(x), curr_unnorm_var = np.var(x) * frames = sum((x - mean_cut)^2), and
//   total_unnorm_var = total_unnorm_var + curr_unnorm_var + (total_frames / curr_frames) / updated_total_frames
//                      * (total_sum / (total_frames / curr_frames) - curr_sum)^2        (the first cut into an empty state assigns)
//   total_sum = total_sum + curr_sum
// all in float64.  Here that is two stream-ordered launches without a floating-point atomic, so a run repeats bit for bit:
//   * partial: a work item = (block of kStBlockFrames frames of one cut, tile of 64 (float32) / 128 (binary16) bins).  The workgroup is
//     kStRowLanes x kStColLanes lanes; lane (r, c) owns the frames r, r + 16, r + 32, ... of the block and 4 / 8 neighbouring bins, which
//     it reads ONCE with one 16-byte load per frame (element by element where the base, the stride or the last bins of a frame do not
//     allow that: the same values reach the same registers) and keeps as read.  Pass 1 sums each bin in float64 (the lane's frames in
//     order, then the 16 lanes in order through LDS) and forms the block's mean = sum / frames; pass 2 sums (x - mean)^2 the same way.
//     Both go to the slab: slab[block][0][bin] = sum, slab[block][1][bin] = sum of squares about the block's own mean.  E[x^2] - E[x]^2
//     is never formed.  Products are rounded before they are added (never contracted).
//   * fold: one lane per bin.  For each cut in table order: the cut's blocks in block order, merged pairwise (Chan, Golub, LeVeque):
//       delta = sum_b / n_b - sum_a / n_a;  m2 = m2_a + m2_b + delta^2 * (n_a * n_b / (n_a + n_b));  sum = sum_a + sum_b
//     (n from the table), then the reference's update above on the state.  The order is the table's: the result does not depend on the
//     grid, the schedule, or how the cuts were grouped into updates.  This launch is a serial chain of one dependent float64 step per block
//     and per cut for every bin.
// Element indices are 64-bit (first_row * row_stride may exceed 2^31); padding rows and the gap behind a frame's last bin are not read.
#pragma once
#include <hip/hip_fp16.h>

#include "common.hpp"
#include "stats_tables.hpp"

namespace hipfeat {

struct StArgs {
  const void* feats;
  const StCut* cuts;  // device
  double* slab;       // [total_blocks][2][F]
  double* state;      // [2][F]: total_sum, total_unnorm_var
  int64_t row_stride, frames_before;
  int32_t num_cuts, feature_dim, items, col_tiles, vec_ok, pad;
};

typedef uint32_t st_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ StCut st_uniform_cut(const StCut* p) {  // every dword through v_readfirstlane (the index was workgroup-uniform)
  const int* w = reinterpret_cast<const int*>(p);
  union {
    int w[4];
    StCut c;
  } u;
#pragma unroll
  for (int i = 0; i < 4; ++i) u.w[i] = __builtin_amdgcn_readfirstlane(w[i]);
  return u.c;
}

// value j of a lane's 16 bytes: float32 number j of 4, or binary16 number j of 8 (widened exactly)
template <bool kF16>
__device__ __forceinline__ double st_value(const uint32_t (&raw)[4], int j) {
  if constexpr (kF16) {
    const uint32_t w = raw[j >> 1];
    const uint16_t h = (uint16_t)((j & 1) ? (w >> 16) : (w & 0xffffu));
    return (double)(float)__builtin_bit_cast(_Float16, h);
  } else {
    return (double)__builtin_bit_cast(float, raw[j]);
  }
}

// the reference's update of the running totals with one more matrix of n frames (base.py:1000-1019), operation for operation
__device__ __forceinline__ void st_update(int64_t tn, double& tsum, double& tvar, int64_t n, double s, double m2) {
  if (tn > 0) {
    const double ratio = (double)tn / (double)n;  // total_over_curr_frames
    const double d = tsum / ratio - s;
    tvar = __dadd_rn(__dadd_rn(tvar, m2), __dmul_rn(ratio / (double)(tn + n), __dmul_rn(d, d)));
  } else {
    tvar = m2;
  }
  tsum = __dadd_rn(tsum, s);
}

template <bool kF16>
__global__ __launch_bounds__(256) void stats_partial_kernel(const StArgs a) {
  constexpr int V = kF16 ? 8 : 4, kTileCols = kStColLanes * V, kPer = kStBlockFrames / kStRowLanes;
  static_assert(kStRowLanes * kStColLanes == 256 && kPer * kStRowLanes == kStBlockFrames, "workgroup shape");
  __shared__ double part[kStRowLanes][kTileCols];
  __shared__ double mean[kTileCols];
  const int tid = threadIdx.x, cl = tid % kStColLanes, rl = tid / kStColLanes, F = a.feature_dim;
  for (int item = blockIdx.x; item < a.items; item += gridDim.x) {
    const int bi = item / a.col_tiles, tile = item - bi * a.col_tiles;
    int lo = 0, hi = a.num_cuts - 1;  // the last cut whose first block is <= bi (cuts of no frames share their successor's)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (a.cuts[mid].block_first <= bi) lo = mid;
      else hi = mid - 1;
    }
    const StCut cd = st_uniform_cut(a.cuts + lo);
    const int f0 = (bi - cd.block_first) * kStBlockFrames;
    const int n = min(kStBlockFrames, cd.frames - f0);  // 1 ... kStBlockFrames
    const int col0 = tile * kTileCols + cl * V;
    const int64_t e0 = cd.first_elem + (int64_t)f0 * a.row_stride + col0;
    const bool vec = a.vec_ok && col0 + V <= F;
    uint32_t raw[kPer][4];  // the lane's 16 bytes of every frame it owns, as they were read
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int r = k * kStRowLanes + rl;
#pragma unroll
      for (int j = 0; j < 4; ++j) raw[k][j] = 0u;
      if (r < n) {
        const int64_t e = e0 + (int64_t)r * a.row_stride;
        if (vec) {
          const st_u4 v = kF16 ? *reinterpret_cast<const st_u4*>(static_cast<const uint16_t*>(a.feats) + e)
                               : *reinterpret_cast<const st_u4*>(static_cast<const uint32_t*>(a.feats) + e);
          raw[k][0] = v.x, raw[k][1] = v.y, raw[k][2] = v.z, raw[k][3] = v.w;
        } else if constexpr (kF16) {
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (col0 + j < F) raw[k][j >> 1] |= (uint32_t)static_cast<const uint16_t*>(a.feats)[e + j] << ((j & 1) * 16);
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j)
            if (col0 + j < F) raw[k][j] = static_cast<const uint32_t*>(a.feats)[e + j];
        }
      }
    }
    double acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.0;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (k * kStRowLanes + rl < n) {
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = __dadd_rn(acc[j], st_value<kF16>(raw[k], j));
      }
#pragma unroll
    for (int j = 0; j < V; ++j) part[rl][cl * V + j] = acc[j];
    __syncthreads();
    const int col = tile * kTileCols + tid;  // (of the lanes tid < kTileCols)
    double* slab = a.slab + (int64_t)bi * 2 * F;
    if (tid < kTileCols) {
      double t = part[0][tid];
#pragma unroll
      for (int r = 1; r < kStRowLanes; ++r) t = __dadd_rn(t, part[r][tid]);  // the 16 lanes in order
      if (col < F) slab[col] = t;
      mean[tid] = t / (double)n;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.0;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (k * kStRowLanes + rl < n) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const double d = st_value<kF16>(raw[k], j) - mean[cl * V + j];
          acc[j] = __dadd_rn(acc[j], __dmul_rn(d, d));
        }
      }
#pragma unroll
    for (int j = 0; j < V; ++j) part[rl][cl * V + j] = acc[j];
    __syncthreads();
    if (tid < kTileCols) {
      double t = part[0][tid];
#pragma unroll
      for (int r = 1; r < kStRowLanes; ++r) t = __dadd_rn(t, part[r][tid]);
      if (col < F) slab[F + col] = t;
    }
    __syncthreads();  // part and mean are free for the next item
  }
}

__global__ __launch_bounds__(64) void stats_fold_kernel(const StArgs a) {
  const int F = a.feature_dim, col = blockIdx.x * 64 + threadIdx.x;
  if (col >= F) return;
  double tsum = a.state[col], tvar = a.state[F + col];
  int64_t tn = a.frames_before;
  for (int c = 0; c < a.num_cuts; ++c) {
    const StCut cd = a.cuts[c];
    if (cd.frames == 0) continue;  // contributes nothing
    const double* p = a.slab + (int64_t)cd.block_first * 2 * F + col;
    const int nb = (cd.frames + kStBlockFrames - 1) / kStBlockFrames;
    double s = p[0], m2 = p[F];
    int n = min(kStBlockFrames, cd.frames);
    for (int k = 1; k < nb; ++k) {
      p += 2 * (int64_t)F;
      const int nk = min(kStBlockFrames, cd.frames - k * kStBlockFrames);
      const double sb = p[0], mb = p[F];
      const double delta = sb / (double)nk - s / (double)n;
      const double w = (double)n * (double)nk / (double)(n + nk);
      m2 = __dadd_rn(__dadd_rn(m2, mb), __dmul_rn(__dmul_rn(delta, delta), w));
      s = __dadd_rn(s, sb);
      n += nk;
    }
    st_update(tn, tsum, tvar, cd.frames, s, m2);
    tn += cd.frames;
  }
  a.state[col] = tsum;
  a.state[F + col] = tvar;
}

// another accumulator's state (other[0 : F] = its sum, other[F : 2F] = its unnormalised variance over `on` > 0 frames) into this one
__global__ __launch_bounds__(64) void stats_merge_kernel(double* state, const double* other, int F, int64_t tn, int64_t on) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= F) return;
  double tsum = state[col], tvar = state[F + col];
  st_update(tn, tsum, tvar, on, other[col], other[F + col]);
  state[col] = tsum;
  state[F + col] = tvar;
}

}  // namespace hipfeat
