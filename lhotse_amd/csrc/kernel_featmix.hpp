// Mixing and collating STORED features (PrecomputedFeatures + CutMix / .pad) on the device: the tracks of a mini-batch -> (B, Tmax, F).
//
// Reference: collate_features (lhotse/dataset/collation.py:115-145) calls cut.load_features() per padded cut; for a MixedCut that is
// either the copy of one cut with a padding value behind it (lhotse/cut/mixed.py:1223-1243) or the FeatureMixer fold of its tracks
// (mixed.py:1245-1307, lhotse/features/mixer.py) with Fbank.mix / Fbank.compute_energy (lhotse/features/kaldi/extractors.py:135-152):
// per added track, in the log domain, log(max(1e-10, exp(a) + gain * exp(b))), gain = E_ref * 10^(-snr/10) / sum(exp(b)).
//
// Two launches, stream-ordered, nothing visits the host in between:
//   * energy: a work item = kFmEnergyBlock elements of one track that needs an energy (a track with an SNR, a reference track); it
//     writes ONE partial sum of exp(x) (float64, exp taken in float64) to partials[item] with a plain store.  No atomics, the lanes'
//     sums are combined in a fixed order, so a run repeats bit for bit and a track's energy does not depend on the other cuts.
//   * fold-and-collate: a work item = one tile of kFmTile output elements of one cut's row of `out`; work item w belongs to row
//     w / tiles_per_row.  Tiles are counted from the 16-byte boundary at or below the ROW's first byte and a lane owns whole 16-byte
//     groups of the destination (4 float32), stored with one 16-byte store where the group lies wholly inside the row and element by
//     element where the row's first or last element cuts it (as kernel_collate.hpp).  A copy-form cut gets the bits of its one track
//     (binary16 widened exactly) and the cut's pad value behind them.  A fold-form cut: the workgroup first forms the gains of its
//     cut's tracks (one lane per track sums the track's and the reference track's partials in index order, float64, and rounds the
//     quotient to float32), then e = g_0 * exp(x_0) and, per later track in order, e = max(1e-10, e + g_t * exp(x_t)) in float32 over
//     ALL frames of the cut -- a frame a track does not cover adds 0 but is floored all the same, a later track of no frames is not
//     mixed at all (mixer.py:116-117) --, products rounded before the add (__fmul_rn / __fadd_rn: never contracted), and one log at
//     the end, taken in float64 and rounded once to float32 (the device's logf was measured 1.7 ulp off at log(1e-10), the value of
//     every padded frame, which is more than the bar leaves).  The mixed matrix exists only in registers.  Elements of the row outside
//     the cut's frames are written as float32(log(1e-10)); every element of out[0 : B * row_len] is written exactly once (no memset in
//     front).
// A track's values are read where they were stored: float32 at any 4-byte boundary, binary16 at any 2-byte boundary; F is arbitrary, so a
// group of 4 output elements may span frames and every element finds its own (frame, bin).  Element indices inside a row are 32-bit
// (the plan bounds a row to 2^30 elements), row starts and arena offsets 64-bit.
#pragma once
#include <hip/hip_fp16.h>

#include "common.hpp"
#include "featmix_tables.hpp"

namespace hipfeat {

struct FmArgs {
  const unsigned char* arena;
  float* out;
  const FmCut* cuts;      // device
  const FmTrack* tracks;  // device
  double* partials;
  int64_t row_len, tiles_per_row, fold_items;
  int32_t num_cuts, num_tracks, energy_items, num_features;
  float log_eps;  // float32(log(1e-10))
  int32_t pad;
};

typedef uint32_t fm_u4 __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ T fm_uniform(const T* p) {  // every dword through v_readfirstlane (the index was workgroup-uniform)
  constexpr int W = (int)(sizeof(T) / 4);
  const int* w = reinterpret_cast<const int*>(p);
  union {
    int w[W];
    T t;
  } u;
#pragma unroll
  for (int i = 0; i < W; ++i) u.w[i] = __builtin_amdgcn_readfirstlane(w[i]);
  return u.t;
}

// element i (0 <= i < frames * F) of a stored track, as float32 bits: a frame behind the stored rows repeats the last one
__device__ __forceinline__ uint32_t fm_load_bits(const unsigned char* __restrict__ arena, const FmTrack& tr, int F, int i) {
  if (i >= tr.rows * F) i -= F;
  if (tr.f16) {
    const _Float16 h = *reinterpret_cast<const _Float16*>(arena + tr.src_off + (int64_t)i * 2);
    return __builtin_bit_cast(uint32_t, (float)h);  // exact
  }
  return *reinterpret_cast<const uint32_t*>(arena + tr.src_off + (int64_t)i * 4);
}

__global__ __launch_bounds__(256) void featmix_energy_kernel(const FmArgs a) {
  __shared__ double red[4];
  const int tid = threadIdx.x, F = a.num_features;
  for (int item = blockIdx.x; item < a.energy_items; item += gridDim.x) {
    int lo = 0, hi = a.num_tracks - 1;  // the last track whose first partial is <= item (tracks without partials share their successor's)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (a.tracks[mid].part_first <= item) lo = mid;
      else hi = mid - 1;
    }
    const FmTrack tr = fm_uniform(a.tracks + lo);
    const int start = (item - tr.part_first) * kFmEnergyBlock;
    const int n = min(kFmEnergyBlock, tr.frames * F - start);
    double acc = 0.0;
    for (int k = tid; k < n; k += 256) acc += exp((double)__builtin_bit_cast(float, fm_load_bits(a.arena, tr, F, start + k)));
    // lanes -> wave (fixed tree), waves -> workgroup (index order): the same order in every run
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) a.partials[item] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
  }
}

__device__ __forceinline__ double fm_track_energy(const FmTrack& tr, int F, const double* __restrict__ partials) {
  if (tr.src_off < 0) return (double)tr.frames * (double)F * exp((double)tr.value);
  double s = 0.0;
  for (int k = 0; k < tr.part_count; ++k) s += partials[tr.part_first + k];
  return s;
}

__global__ __launch_bounds__(256) void featmix_fold_kernel(const FmArgs a) {
  __shared__ float gains[kFmMaxTracks];
  constexpr int kRounds = kFmTile / (4 * 256);
  static_assert(kRounds * 4 * 256 == kFmTile, "tile size");
  const int tid = threadIdx.x, F = a.num_features;
  for (int64_t w = blockIdx.x; w < a.fold_items; w += gridDim.x) {
    const int64_t c = w / a.tiles_per_row, tile = w - c * a.tiles_per_row;  // (workgroup-uniform)
    const FmCut cd = fm_uniform(a.cuts + c);
    float* rowp = a.out + c * a.row_len;
    // positions p are counted from the 16-byte boundary at or below the row's first element: element e of the row is p = head + e
    const int head = (int)((reinterpret_cast<uintptr_t>(rowp) / 4) & 3);
    const int row_len = (int)a.row_len;
    const int p0 = (int)tile * kFmTile;  // (tiles * kFmTile <= row_len + 3 + kFmTile: fits)
    if (p0 >= head + row_len) continue;
    const int lo = cd.dst_first * F, hi = lo + cd.num_frames * F;  // the cut's frames are the elements [lo, hi) of the row
    uint32_t v[kRounds][4];
    if (cd.form == kFmCopy) {
      const FmTrack tr = fm_uniform(a.tracks + cd.track_first);
      const int n = tr.frames * F;
      const uint32_t padv = __builtin_bit_cast(uint32_t, cd.pad_value), cst = __builtin_bit_cast(uint32_t, tr.value);
#pragma unroll
      for (int k = 0; k < kRounds; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = p0 + 4 * (tid + 256 * k) + j - head, i = e - lo;
          uint32_t x = padv;
          if ((unsigned)i < (unsigned)n) x = tr.src_off < 0 ? cst : fm_load_bits(a.arena, tr, F, i);
          v[k][j] = x;
        }
    } else {
      __syncthreads();  // the previous item's gains have been read
      for (int t = tid; t < cd.track_count; t += 256) {
        const FmTrack tr = a.tracks[cd.track_first + t];
        float g = 1.0f;
        if (tr.ratio >= 0.0 && cd.ref_track >= 0) {
          const double er = fm_track_energy(a.tracks[cd.ref_track], F, a.partials), et = fm_track_energy(tr, F, a.partials);
          if (er > 0.0 && et > 0.0) g = (float)(er * tr.ratio / et);  // (mixer.py:170-175, mixed.py:1951-1957)
        }
        gains[t] = g;
      }
      __syncthreads();
      // the cut has one frame more than the mix: its last frame repeats the mix's last one (mixed.py:1299-1300)
      const int rep = cd.num_frames > cd.mix_frames ? lo + cd.mix_frames * F : INT32_MAX;
      float acc[kRounds][4];
#pragma unroll
      for (int k = 0; k < kRounds; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[k][j] = 0.0f;
      const int e_lo = p0 - head, e_hi = e_lo + kFmTile;  // the tile's elements (before the repeated frame is mapped back)
      for (int t = 0; t < cd.track_count; ++t) {
        const FmTrack tr = fm_uniform(a.tracks + cd.track_first + t);
        if (t > 0 && tr.frames == 0) continue;  // not mixed at all
        const int a0 = lo + tr.first * F, n = tr.frames * F;
        // (a tile that holds the repeated frame reads up to F elements in front of itself)
        const bool reaches = n > 0 && a0 < e_hi && a0 + n > e_lo - (rep != INT32_MAX ? F : 0);
        if (reaches) {
          const float g = gains[t];
#pragma unroll
          for (int k = 0; k < kRounds; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              int e = e_lo + 4 * (tid + 256 * k) + j;
              if (e >= rep) e -= F;
              const int i = e - a0;
              if ((unsigned)i < (unsigned)n && e >= lo && e < hi) {
                const float x = tr.src_off < 0 ? tr.value : __builtin_bit_cast(float, fm_load_bits(a.arena, tr, F, i));
                acc[k][j] = __fadd_rn(acc[k][j], __fmul_rn(g, expf(x)));
              }
            }
        }
        if (t > 0) {
#pragma unroll
          for (int k = 0; k < kRounds; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[k][j] = fmaxf(1e-10f, acc[k][j]);
        }
      }
#pragma unroll
      for (int k = 0; k < kRounds; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[k][j] = __builtin_bit_cast(uint32_t, (float)log((double)acc[k][j]));  // (rounded once)
    }
    const uint32_t outside = __builtin_bit_cast(uint32_t, a.log_eps);
#pragma unroll
    for (int k = 0; k < kRounds; ++k) {
      const int e0 = p0 + 4 * (tid + 256 * k) - head;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j < lo || e0 + j >= hi) v[k][j] = outside;
      if (e0 >= 0 && e0 + 4 <= row_len) {
        *reinterpret_cast<fm_u4*>(rowp + e0) = fm_u4{v[k][0], v[k][1], v[k][2], v[k][3]};
      } else {  // the row's first or last element cuts the group (or the group lies outside the row)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (e0 + j >= 0 && e0 + j < row_len) rowp[e0 + j] = __builtin_bit_cast(float, v[k][j]);
      }
    }
  }
}

}  // namespace hipfeat
