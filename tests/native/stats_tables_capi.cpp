// Test shim (CPU only): a C entry point around lhotse_amd/csrc/stats_tables.hpp -- the whole of what hipfeat_stats_update decides on the
// host -- so that tests/test_stats_host.py can check the table and every refusal without a device.  With -DSTATS_TABLES_MAIN it is a
// stand-alone program (also built with -fsanitize=address,undefined) that walks the same code over bin counts, strides and frame counts
// around the block boundary and checks the invariants the kernels rely on for their bounds.
#include "../../lhotse_amd/csrc/stats_tables.hpp"

#include <cstdio>
#include <cstring>

// returns the status; h_info[6] = {total frames, total blocks, column tiles, work items, 16-byte loads allowed, row stride}; h_cuts (may
// be NULL): the descriptors of 16 bytes; message: 256 bytes.  A refusal writes the message only.
extern "C" int st_plan(long long feature_dim, unsigned long long base, long long feats_elems, int dtype, long long num_cuts, const int64_t* h_first_row,
                       const int64_t* h_num_frames, long long row_stride, int64_t* h_info, void* h_cuts, char* message) {
  const hipfeat::StPlan p = hipfeat::build_stats_plan(feature_dim, base, feats_elems, dtype, num_cuts, h_first_row, h_num_frames, row_stride);
  std::snprintf(message, 256, "%s", p.message.c_str());
  if (p.status != 0) return p.status;
  h_info[0] = p.total_frames;
  h_info[1] = p.total_blocks;
  h_info[2] = p.col_tiles;
  h_info[3] = p.items;
  h_info[4] = p.vec_ok;
  h_info[5] = p.row_stride;
  if (h_cuts) std::memcpy(h_cuts, p.cuts.data(), p.cuts.size() * sizeof(hipfeat::StCut));
  return 0;
}

extern "C" int st_block_frames() { return hipfeat::kStBlockFrames; }
extern "C" int st_row_lanes() { return hipfeat::kStRowLanes; }
extern "C" int st_col_lanes() { return hipfeat::kStColLanes; }
extern "C" int st_max_cuts() { return hipfeat::kStMaxCuts; }
extern "C" int st_max_dim() { return hipfeat::kStMaxDim; }
extern "C" long long st_blocks_of(long long frames) { return hipfeat::st_blocks(frames); }
extern "C" long long st_tiles_of(long long F, int dtype) { return hipfeat::st_col_tiles(F, dtype); }

#ifdef STATS_TABLES_MAIN
#define CHECK(c)                                                                                                     \
  do {                                                                                                               \
    if (!(c)) {                                                                                                      \
      std::printf("FAILED %s (F %lld stride %lld frames %lld)\n", #c, (long long)F, (long long)stride, (long long)T); \
      return 1;                                                                                                      \
    }                                                                                                                \
  } while (0)

int main() {
  const long long B = hipfeat::kStBlockFrames;
  for (int64_t F : {1LL, 3LL, 4LL, 80LL, 257LL, 65535LL})
    for (int64_t gap : {0LL, 1LL, 3LL})
      for (int64_t T : {1LL, 2LL, B - 1, B, B + 1, 3 * B + 5})
        for (int dtype : {0, 1}) {
          const int64_t stride = F + gap;
          // cuts in descending row order with a cut of no frames in the middle; the last one starts past 2^40 elements
          const int64_t far = ((1LL << 40) + stride - 1) / stride;
          const int64_t first[4] = {far, 2 * T + 7, 5, 0}, frames[4] = {T, T, 0, 2};
          const int64_t elems = (far + T - 1) * stride + F;
          const hipfeat::StPlan p = hipfeat::build_stats_plan(F, 64, elems, dtype, 4, first, frames, stride);
          CHECK(p.status == 0 && p.cuts.size() == 4);
          CHECK(p.total_frames == 2 * T + 2 && p.total_blocks == 2 * hipfeat::st_blocks(T) + 1 && p.items == p.total_blocks * p.col_tiles);
          CHECK(p.col_tiles * hipfeat::st_tile_cols(dtype) >= F && (p.col_tiles - 1) * hipfeat::st_tile_cols(dtype) < F);
          int64_t blocks = 0;
          for (const hipfeat::StCut& c : p.cuts) {
            CHECK(c.block_first == blocks && c.first_elem >= 0);
            blocks += hipfeat::st_blocks(c.frames);
            // every block of the cut has 1 ... B frames and the cut's last element lies inside the buffer
            for (int64_t k = 0; k < hipfeat::st_blocks(c.frames); ++k) CHECK(c.frames - k * B >= 1);
            if (c.frames > 0) CHECK(c.first_elem + (int64_t)(c.frames - 1) * stride + F <= elems);
          }
          CHECK(p.cuts[0].first_elem == far * stride && p.cuts[0].first_elem >= (1LL << 40));
          CHECK(p.vec_ok == ((stride * (dtype ? 2 : 4)) % 16 == 0 ? 1 : 0));
          // one element short: refused, and packed cuts (no first rows) are laid back to back
          CHECK(hipfeat::build_stats_plan(F, 64, elems - 1, dtype, 4, first, frames, stride).status == 1);
          const hipfeat::StPlan q = hipfeat::build_stats_plan(F, 64 + (dtype ? 2 : 4), (2 * T + 2 - 1) * stride + F, dtype, 4, nullptr, frames, stride);
          CHECK(q.status == 0 && q.vec_ok == 0 && q.cuts[1].first_elem == T * stride && q.cuts[3].first_elem == 2 * T * stride);
        }
  std::printf("ok\n");
  return 0;
}
#endif
