// Test shim (CPU only): a C entry point around lhotse_amd/csrc/reverb_tables.hpp -- the whole of what hipfeat_reverb_plan decides -- so
// that tests/test_reverb_abi.py can check the table and the plan-time errors without a device.  With -DREVERB_TABLES_MAIN it is a
// stand-alone program (also built with -fsanitize=address,undefined) that walks the same code over lengths around the block boundaries
// and checks the invariants the kernels rely on for their bounds.
#include "../../lhotse_amd/csrc/reverb_tables.hpp"

#include <cstdio>
#include <cstring>

// returns the status; h_out_offsets / h_info[4] as hipfeat_reverb_plan (ticket 0), untouched by a refusal; h_items (may be NULL): num_items
// descriptors of 48 bytes; message: 256 bytes
extern "C" int rt_plan(long long num_items, const int64_t* h_src_offset, const int64_t* h_src_len, const int64_t* h_rir_offset, const int64_t* h_rir_len,
                       const int64_t* h_shift, const int32_t* h_normalize, long long tail_start, int64_t* h_out_offsets, int64_t* h_info, void* h_items,
                       char* message) {
  const hipfeat::RvPlan p = hipfeat::build_reverb_plan(num_items, h_src_offset, h_src_len, h_rir_offset, h_rir_len, h_shift, h_normalize, tail_start);
  std::snprintf(message, 256, "%s", p.message.c_str());
  if (p.status != 0) return p.status;
  if (h_out_offsets)
    for (size_t i = 0; i < p.items.size(); ++i) h_out_offsets[i] = p.items[i].out_off;
  h_info[0] = 0;
  h_info[1] = p.arena_need;
  h_info[2] = p.work_items;
  h_info[3] = 2 * p.work_items;
  if (h_items) std::memcpy(h_items, p.items.data(), p.items.size() * sizeof(hipfeat::RvItem));
  return 0;
}

extern "C" int rt_block() { return hipfeat::kRvBlock; }
extern "C" int rt_lane() { return hipfeat::kRvLane; }

#ifdef REVERB_TABLES_MAIN
#define CHECK(c)                                                                     \
  do {                                                                               \
    if (!(c)) {                                                                      \
      std::printf("FAILED %s (samples %lld taps %lld)\n", #c, (long long)n, (long long)taps); \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

int main() {
  for (int64_t n : {1LL, 7LL, 8LL, 9LL, 2047LL, 2048LL, 2049LL, 70001LL, (long long)(INT32_MAX / 2)})
    for (int64_t taps : {1LL, 2LL, 255LL, 256LL, 257LL, 4097LL, (long long)(INT32_MAX / 2)}) {
      const int64_t far = 1LL << 33;
      const int64_t src[2] = {0, far}, len[2] = {n, 5}, rir[2] = {far + 5, far + 5}, rl[2] = {taps, taps}, shift[2] = {taps - 1, 0};
      const int32_t norm[2] = {1, 0};
      const int64_t tail_start = far + 5 + taps + 1;
      const hipfeat::RvPlan p = hipfeat::build_reverb_plan(2, src, len, rir, rl, shift, norm, tail_start);
      CHECK(p.status == 0 && p.items.size() == 2);
      const hipfeat::RvItem& it = p.items[0];
      const int64_t blocks = p.items[1].item_first;
      // every output lies in exactly one work item, and no work item is empty; the furthest output a lane may name fits an int
      CHECK(blocks * hipfeat::kRvBlock >= n && (blocks - 1) * hipfeat::kRvBlock < n && blocks * hipfeat::kRvBlock + hipfeat::kRvLane <= INT32_MAX);
      CHECK(it.n == n && it.taps == taps && it.shift == taps - 1 && it.normalize == 1 && p.items[1].normalize == 0 && it.item_first == 0);
      CHECK(it.out_off == ((tail_start + 3) & ~3LL) && p.items[1].out_off == it.out_off + ((n + 3) & ~3LL) && p.items[1].out_off % 4 == 0);
      CHECK(p.work_items == blocks + 1 && p.arena_need == p.items[1].out_off + 8);
      // a shift of `taps` is outside the impulse response
      const int64_t bad[2] = {taps, 0};
      CHECK(hipfeat::build_reverb_plan(2, src, len, rir, rl, bad, norm, tail_start).status == 1);
    }
  std::printf("ok\n");
  return 0;
}
#endif
