// Mixing the tracks of MixedCuts (CutMix / CutSet.mix / .pad) on the device, in front of the feature launch.
//
// Reference: MixedCut.load_audio (lhotse/cut/mixed.py:1312-1409) loads every audible track, takes audio_energy = mean(x^2) of the tracks that
// need one (lhotse/audio/mixer.py:175-176), turns every SNR into a gain against the reference track's energy
// (AudioMixer.add_to_mix, mixer.py:138-172: gain = sqrt(E_ref * 10^(-snr/10) / E_track), 1 without an SNR or when an energy is not positive),
// materialises gain * audio in float32 and adds the tracks at their offsets in track order into a zero buffer (mixed_audio, mixer.py:104-119).
//
// Two launches, stream-ordered, nothing visits the host in between:
//   * energy: a work item = kMixEnergyBlock samples of one track that needs an energy; it writes ONE partial sum of squares (float64) to
//     partials[item] with a plain store.  float64 because the squares of float32 samples are exact in it and a sum of < 2^31 of them loses
//     nothing a float32 gain could see (the reference's own float32 pairwise np.average differs from it by ~1e-7 relative); no atomics, the
//     lanes' sums are combined in a fixed order, so a run repeats bit for bit.
//   * mix: a work item = kMixBlock output samples of one cut.  The workgroup first forms the gains of its cut's tracks (one lane per track
//     sums the track's and the reference track's partials in index order, float64, and rounds the gain to float32), then every lane
//     produces 4 x 4 consecutive samples: acc = acc + g * x over the tracks that cover the sample, in track order, the product rounded
//     before the add (__fmul_rn / __fadd_rn: never contracted into an FMA), and stores them 16 bytes at a time.  Samples no track covers
//     come out as 0 and are written (the arena's tail is uninitialised memory).  A padding track has no source and adds nothing.
//     Source reads are coalesced dword loads: a track's offset in its cut is an arbitrary sample count, so they are not 16-byte aligned
//     relative to the output.
//
// Work distribution and tables as kernel_minibatch.hpp: one flat item list over a grid of a few workgroups per CU, the owner of an item
// found by bisection over prefix sums in LDS; the tables (MixCut[num_cuts] | MixTrack[num_tracks]) travel in the kernel arguments when
// they fit kMbInlineBytes and through pinned memory otherwise.
#pragma once
#include "common.hpp"
#include "kernel_minibatch.hpp"
#include "mix_tables.hpp"

namespace hipfeat {

struct MixHeader {
  float* arena;
  double* partials;
  const unsigned char* tables;  // staged blob (nullptr = inline)
  int32_t num_cuts, num_tracks, energy_items, mix_items;
  int32_t table_bytes, pad;
};
struct MixInlineArgs {
  MixHeader h;
  alignas(16) unsigned char blob[kMbInlineBytes];
};
static_assert(offsetof(MixInlineArgs, blob) % 16 == 0 && sizeof(MixInlineArgs) <= 3584, "kernel-argument layout");

__device__ __forceinline__ void mix_energy_body(const MixHeader& h, const unsigned char* tb, double* red) {
  const MixTrack* trk = reinterpret_cast<const MixTrack*>(tb + (size_t)h.num_cuts * sizeof(MixCut));
  const int tid = threadIdx.x;
  for (int item = blockIdx.x; item < h.energy_items; item += gridDim.x) {
    const int t = mb_owner(&trk[0].part_first, (int)(sizeof(MixTrack) / sizeof(int32_t)), h.num_tracks, item);
    const MixTrack tr = mb_uniform32(trk + t);
    const int start = (item - tr.part_first) * kMixEnergyBlock;
    const int n = min(kMixEnergyBlock, tr.src_len - start);
    const float* __restrict__ x = h.arena + tr.src_off + start;
    double acc = 0.0;
#pragma unroll 8
    for (int k = tid; k < n; k += 256) {
      const double v = (double)x[k];
      acc = fma(v, v, acc);
    }
    // lanes -> wave (fixed tree), waves -> workgroup (index order): the same order in every run
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) h.partials[item] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
  }
}

__device__ __forceinline__ double mix_track_energy(const MixTrack& tr, const double* __restrict__ partials) {
  double s = 0.0;
  for (int k = 0; k < tr.part_count; ++k) s += partials[tr.part_first + k];
  return s / (double)tr.src_len;
}

__device__ __forceinline__ void mix_body(const MixHeader& h, const unsigned char* tb, float* gains) {
  const MixCut* cuts = reinterpret_cast<const MixCut*>(tb);
  const MixTrack* trk = reinterpret_cast<const MixTrack*>(tb + (size_t)h.num_cuts * sizeof(MixCut));
  const int tid = threadIdx.x;
  for (int item = blockIdx.x; item < h.mix_items; item += gridDim.x) {
    const int c = mb_owner(&cuts[0].item_first, (int)(sizeof(MixCut) / sizeof(int32_t)), h.num_cuts, item);
    const MixCut cd = mb_uniform32(cuts + c);
    __syncthreads();  // the previous item's gains have been read
    for (int t = tid; t < cd.track_count; t += 256) {
      const MixTrack tr = trk[cd.track_first + t];
      float g = 1.0f;
      if (tr.ratio >= 0.0 && cd.ref_track >= 0 && tr.src_off >= 0 && tr.part_count > 0) {
        const MixTrack ref = trk[cd.ref_track];
        if (ref.part_count > 0) {
          const double er = mix_track_energy(ref, h.partials), et = mix_track_energy(tr, h.partials);
          if (er > 0.0 && et > 0.0) g = (float)sqrt(er * tr.ratio / et);  // (mixer.py:160-165; rounded to float32 as gain * audio does)
        }
      }
      gains[t] = g;
    }
    __syncthreads();
    const int base = (item - cd.item_first) * kMixBlock;
    const int end = min(base + kMixBlock, cd.out_len);
    float acc[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[k][j] = 0.0f;
    for (int t = 0; t < cd.track_count; ++t) {
      const MixTrack* tp = trk + cd.track_first + t;
      const int64_t src_off = ((int64_t)__builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(tp)[1]) << 32) |
                              (uint32_t)__builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(tp)[0]);
      const int src_len = __builtin_amdgcn_readfirstlane(tp->src_len), dst_off = __builtin_amdgcn_readfirstlane(tp->dst_off);
      if (src_off < 0 || dst_off >= end || (int64_t)dst_off + src_len <= base) continue;  // padding track, or it does not reach this block
      const float g = gains[t];
      const float* __restrict__ x = h.arena + src_off;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i0 = base + 4 * (tid + 256 * k) - dst_off;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ((unsigned)(i0 + j) < (unsigned)src_len) ? x[i0 + j] : 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((unsigned)(i0 + j) < (unsigned)src_len) acc[k][j] = __fadd_rn(acc[k][j], __fmul_rn(g, v[j]));
      }
    }
    float* __restrict__ y = h.arena + cd.out_off;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int p = base + 4 * (tid + 256 * k);
      if (p + 3 < end) {
        *reinterpret_cast<float4*>(y + p) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (p + j < end) y[p + j] = acc[k][j];
      }
    }
  }
}

__global__ __launch_bounds__(256) void mix_energy_inline_kernel(const MixInlineArgs a) {
  __shared__ double red[4];
  __shared__ __attribute__((aligned(16))) unsigned char tb[kMbInlineBytes];
  mb_inline_tables(tb, a.h.table_bytes, offsetof(MixInlineArgs, blob));
  mix_energy_body(a.h, tb, red);
}

__global__ __launch_bounds__(256) void mix_energy_kernel(const MixHeader h) {
  __shared__ double red[4];
  extern __shared__ __attribute__((aligned(16))) unsigned char mix_tb_dyn[];
  mix_energy_body(h, mb_staged_tables(h.tables, h.table_bytes, mix_tb_dyn), red);
}

__global__ __launch_bounds__(256) void mix_inline_kernel(const MixInlineArgs a) {
  __shared__ float gains[kMixMaxTracks];
  __shared__ __attribute__((aligned(16))) unsigned char tb[kMbInlineBytes];
  mb_inline_tables(tb, a.h.table_bytes, offsetof(MixInlineArgs, blob));
  mix_body(a.h, tb, gains);
}

__global__ __launch_bounds__(256) void mix_kernel(const MixHeader h) {
  __shared__ float gains[kMixMaxTracks];
  extern __shared__ __attribute__((aligned(16))) unsigned char mix_tb_dyn[];
  mix_body(h, mb_staged_tables(h.tables, h.table_bytes, mix_tb_dyn), gains);
}

}  // namespace hipfeat
