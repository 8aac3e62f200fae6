// Host side of resample_mfma_kernel (kernel_resample.hpp): the tile geometry of a ratio and the padded, transposed filter bank that
// hipfeat_resampler_create uploads for it.  Pure C++ (no HIP): also compiled by tests/native/resample_tables_capi.cpp and checked on the
// CPU (tests/test_resample_tables.py).
//
// The kernel sees a cut as the GEMM  Y[j][ph] = sum_i X[j][i] * K[ph][i],  X[j][i] = xpad[j * orig + i]  (j = hop, ph < nw, i < kw =
// 2 * width + orig): a workgroup owns `hops_per_block` consecutive hops of one cut, its input span sits in LDS once, and a wave owns
// tiles of 16 hops x 16 phases.  The bank is stored tap-major, `kt[i][ph]`, zero-padded to kwp x nwp so that every trip of the tap loop (four
// 16x16x4 MFMAs) reads whole rows: taps behind kw and phases behind nw are zeros (a zero tap leaves the accumulator as it is, a padded phase is not stored).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hipfeat {

constexpr int kResMfmaTile = 16;          // hops and phases of one MFMA tile
constexpr int kResMfmaKStep = 16;         // taps of one trip of the kernel's tap loop: four MFMAs of 4 taps
constexpr int kResMfmaMaxHopTiles = 4;    // hop tiles of a workgroup = independent accumulators of a wave
constexpr int kResMfmaLdsBytes = 65536;   // LDS a workgroup may take for its input span

struct ResMfmaGeometry {
  int kw = 0, kwp = 0, nwp = 0;   // taps; taps padded to a multiple of 16; phases padded to a multiple of 16
  int hop_tiles = 0;              // 1, 2 or 4: the most whose span fits the LDS budget; 0: not even one tile fits
  int hops_per_block = 0;         // 16 * hop_tiles
  int outs_per_block = 0;         // hops_per_block * nw: a cut of out_len samples takes ceil(out_len / outs_per_block) workgroups
  int span_floats = 0;            // (hops_per_block - 1) * orig + kwp, rounded up to 4: the staged input of one workgroup
  size_t lds_bytes = 0;
  bool fits = false;
};

inline ResMfmaGeometry res_mfma_geometry(int orig, int nw, int width) {
  ResMfmaGeometry g;
  g.kw = 2 * width + orig;
  g.kwp = (g.kw + kResMfmaKStep - 1) / kResMfmaKStep * kResMfmaKStep;
  g.nwp = (nw + kResMfmaTile - 1) / kResMfmaTile * kResMfmaTile;
  for (int ht = kResMfmaMaxHopTiles; ht >= 1; ht >>= 1) {
    const int64_t span = ((int64_t)(kResMfmaTile * ht - 1) * orig + g.kwp + 3) & ~(int64_t)3;
    if (span * (int64_t)sizeof(float) > kResMfmaLdsBytes) continue;
    if ((int64_t)kResMfmaTile * ht * nw > INT32_MAX / 2) continue;
    g.hop_tiles = ht;
    g.hops_per_block = kResMfmaTile * ht;
    g.outs_per_block = g.hops_per_block * nw;
    g.span_floats = (int)span;
    g.lds_bytes = (size_t)span * sizeof(float);
    g.fits = true;
    break;
  }
  return g;
}

// Workgroups of a cut with `out_len` output samples.
inline int64_t res_mfma_blocks(const ResMfmaGeometry& g, int64_t out_len) {
  return g.fits ? (out_len + g.outs_per_block - 1) / g.outs_per_block : 0;
}

// The routing rule of hipfeat_resampler_create behind the compile-time instances: at least one full phase tile, and an odd hop
// (the A operand's LDS stride is `orig` floats over the 16 rows of a tile: an odd stride spreads them over the banks, an even one
// does not; even ratios such as 160:441 stay on the generic kernel).
inline bool res_mfma_routed(int orig, int nw, int width) {
  return nw >= kResMfmaTile && (orig & 1) && res_mfma_geometry(orig, nw, width).fits;
}

// kernel: [nw][kw] as the caller computed it  ->  kt: [kwp][nwp], kt[i][ph] = kernel[ph][i], zero elsewhere
inline std::vector<float> res_mfma_bank(const float* kernel, int nw, int kw, int kwp, int nwp) {
  std::vector<float> kt((size_t)kwp * nwp, 0.0f);
  for (int ph = 0; ph < nw; ++ph)
    for (int i = 0; i < kw; ++i) kt[(size_t)i * nwp + ph] = kernel[(size_t)ph * kw + i];
  return kt;
}

}  // namespace hipfeat
