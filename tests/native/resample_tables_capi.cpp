// Test shim (CPU only): C entry points around lhotse_amd/csrc/resample_tables.hpp so that tests/test_resample_tables.py can check the
// geometry and the padded bank of the matrix-core resampler against numpy.  With -DRESAMPLE_TABLES_MAIN it is a stand-alone program
// (also built with -fsanitize=address,undefined) that walks the same code over a set of ratios and checks the invariants the kernel
// relies on for its bounds.
#include "../../lhotse_amd/csrc/resample_tables.hpp"

#include <cstdio>
#include <cstring>

// out[0..9] = kw, kwp, nwp, hop_tiles, hops_per_block, outs_per_block, span_floats, lds_bytes, fits, routed
extern "C" void rt_geometry(int orig, int nw, int width, long long* out) {
  const hipfeat::ResMfmaGeometry g = hipfeat::res_mfma_geometry(orig, nw, width);
  const long long v[10] = {g.kw, g.kwp, g.nwp, g.hop_tiles, g.hops_per_block, g.outs_per_block, g.span_floats, (long long)g.lds_bytes,
                           g.fits, hipfeat::res_mfma_routed(orig, nw, width)};
  std::memcpy(out, v, sizeof(v));
}

extern "C" long long rt_blocks(int orig, int nw, int width, long long out_len) {
  return hipfeat::res_mfma_blocks(hipfeat::res_mfma_geometry(orig, nw, width), out_len);
}

// kt must hold kwp * nwp floats
extern "C" void rt_bank(const float* kernel, int nw, int kw, int kwp, int nwp, float* kt) {
  const std::vector<float> t = hipfeat::res_mfma_bank(kernel, nw, kw, kwp, nwp);
  std::memcpy(kt, t.data(), t.size() * sizeof(float));
}

#ifdef RESAMPLE_TABLES_MAIN
#define CHECK(c)                                                                   \
  do {                                                                             \
    if (!(c)) {                                                                    \
      std::printf("FAILED %s (orig %d nw %d width %d)\n", #c, orig, nw, width);    \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

int main() {
  const int ratios[][3] = {{441, 160, 17}, {441, 320, 8}, {441, 640, 7}, {147, 80, 12}, {160, 441, 6}, {9, 10, 7}, {1, 16, 7}, {20001, 16, 7}, {999, 17, 6}};
  for (const auto& r : ratios) {
    const int orig = r[0], nw = r[1], width = r[2];
    const hipfeat::ResMfmaGeometry g = hipfeat::res_mfma_geometry(orig, nw, width);
    CHECK(g.kw == 2 * width + orig && g.kwp >= g.kw && g.kwp % 16 == 0 && g.kwp - g.kw < 16);
    CHECK(g.nwp >= nw && g.nwp % 16 == 0 && g.nwp - nw < 16);
    if (!g.fits) {
      CHECK(hipfeat::res_mfma_blocks(g, 1000) == 0 && !hipfeat::res_mfma_routed(orig, nw, width));
      continue;
    }
    CHECK(g.hop_tiles == 1 || g.hop_tiles == 2 || g.hop_tiles == 4);
    // the last LDS float a lane reads: row 16 * hop_tiles - 1, tap kwp - 1
    CHECK((long long)(g.hops_per_block - 1) * orig + g.kwp - 1 < g.span_floats);
    CHECK(g.lds_bytes == (size_t)g.span_floats * 4 && g.lds_bytes <= 65536);
    std::vector<float> k((size_t)nw * g.kw);
    for (size_t i = 0; i < k.size(); ++i) k[i] = (float)(i + 1);
    const std::vector<float> kt = hipfeat::res_mfma_bank(k.data(), nw, g.kw, g.kwp, g.nwp);
    CHECK(kt.size() == (size_t)g.kwp * g.nwp);
    for (int i = 0; i < g.kwp; ++i)
      for (int ph = 0; ph < g.nwp; ++ph)
        CHECK(kt[(size_t)i * g.nwp + ph] == (i < g.kw && ph < nw ? k[(size_t)ph * g.kw + i] : 0.0f));
    for (long long n : {0LL, 1LL, (long long)g.outs_per_block - 1, (long long)g.outs_per_block, (long long)g.outs_per_block + 1, 2147483647LL})
      CHECK(hipfeat::res_mfma_blocks(g, n) * g.outs_per_block >= n && (hipfeat::res_mfma_blocks(g, n) - 1) * g.outs_per_block < n + (n == 0));
  }
  std::printf("ok\n");
  return 0;
}
#endif
