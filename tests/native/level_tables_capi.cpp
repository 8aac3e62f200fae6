// Test shim (CPU only): a C entry point around lhotse_amd/csrc/level_tables.hpp -- the whole of what hipfeat_level_plan decides -- so that
// tests/test_level_abi.py can check the table and the plan-time errors without a device.  With -DLEVEL_TABLES_MAIN it is a stand-alone
// program (also built with -fsanitize=address,undefined) that walks the same code over offsets and lengths around the tile and group
// boundaries and checks the invariants the kernels rely on for their bounds.
#include "../../lhotse_amd/csrc/level_tables.hpp"

#include <cstdio>
#include <cstring>

// returns the status; h_info[4] as hipfeat_level_plan; h_items (may be NULL): num_items descriptors of 64 bytes; message: 256 bytes
extern "C" int lt_plan(long long num_items, const int64_t* h_src_offset, const int64_t* h_src_len, const int64_t* h_dst_offset, const int64_t* h_op_first,
                       const int32_t* h_op_kind, const float* h_op_value, const int32_t* h_op_flags, int64_t* h_info, void* h_items, char* message) {
  const hipfeat::LvPlan p = hipfeat::build_level_plan(num_items, h_src_offset, h_src_len, h_dst_offset, h_op_first, h_op_kind, h_op_value, h_op_flags);
  std::snprintf(message, 256, "%s", p.message.c_str());
  if (p.status != 0) return p.status;
  h_info[0] = 0;
  h_info[1] = p.arena_need;
  h_info[2] = p.peak_items;
  h_info[3] = p.work_items;
  if (h_items && !p.items.empty()) std::memcpy(h_items, p.items.data(), p.items.size() * sizeof(hipfeat::LvItem));
  return 0;
}

extern "C" float lt_silence_peak() { return hipfeat::kLvSilencePeak; }
extern "C" int lt_block() { return hipfeat::kLvBlock; }

#ifdef LEVEL_TABLES_MAIN
#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) {                                                                  \
      std::printf("FAILED %s (offset %lld len %lld)\n", #c, (long long)so, (long long)n); \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

int main() {
  for (int64_t so : {0LL, 1LL, 2LL, 3LL, 4LL, 4095LL, 4097LL, 1LL << 33})
    for (int64_t n : {1LL, 3LL, 4LL, 5LL, 4093LL, 4096LL, 4097LL, 70001LL, (long long)(INT32_MAX / 2)}) {
      const int64_t src[2] = {so, so + n + 5}, len[2] = {n, 7}, dst[2] = {so, so + n + 20}, first[3] = {0, 2, 3};
      const int32_t kind[3] = {hipfeat::kLvScale, hipfeat::kLvClip, hipfeat::kLvScale}, flags[3] = {0, hipfeat::kLvNormalize, 0};
      const float value[3] = {0.5f, 1.0f, -2.0f};
      const hipfeat::LvPlan p = hipfeat::build_level_plan(2, src, len, dst, first, kind, value, flags);
      CHECK(p.status == 0 && p.items.size() == 2);
      const hipfeat::LvItem& it = p.items[0];
      const int64_t head = so & 3, blocks = p.items[1].item_first;
      // every sample lies in exactly one tile, and no tile is empty: the tiles cover [0, head + n) counted from the 16-byte boundary
      CHECK(blocks * hipfeat::kLvBlock >= head + n && (blocks - 1) * hipfeat::kLvBlock < head + n);
      // the furthest sample a lane may touch: tile (blocks - 1), group 1023, sample 3 -- it is guarded by `< head + n`, and fits an int
      CHECK(blocks * hipfeat::kLvBlock + 3 <= INT32_MAX);
      CHECK(it.clip_at == 1 && it.nops == 2 && p.items[1].clip_at == -1 && p.peak_items == blocks);
      CHECK(p.arena_need == so + n + 27 && p.work_items == blocks + 1);
    }
  std::printf("ok\n");
  return 0;
}
#endif
