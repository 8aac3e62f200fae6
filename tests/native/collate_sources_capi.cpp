// Test shim (CPU only): a C entry point around build_collate_sources_plan (lhotse_amd/csrc/collate_tables.hpp) -- the whole of what
// hipfeat_collate_plan_sources decides -- and the ticket ring it shares with hipfeat_collate_plan, so that
// tests/test_collate_sources_abi.py can check the tables and the plan-time errors without a device.  With -DCOLLATE_SOURCES_MAIN it is a
// stand-alone program (also built with -fsanitize=address,undefined) that walks the same code over source counts and row lengths around
// the tile boundaries and checks the invariants the kernel relies on for its bounds.
#include "../../lhotse_amd/csrc/collate_tables.hpp"
#include "../../lhotse_amd/csrc/ticket_slots.hpp"

#include <cstdio>
#include <cstring>

// returns the status; h_info[4] as hipfeat_collate_plan_sources (ticket 0); h_rows (may be NULL): num_rows descriptors of 32 bytes;
// h_srcs (may be NULL): the staged source offsets, h_first[num_rows] entries; message: 256 bytes
extern "C" int cs_plan(long long num_rows, const int64_t* h_first, const int64_t* h_src_offset, const int64_t* h_src_len, const int64_t* h_dst_offset,
                       long long row_len, int out_type, int64_t* h_info, void* h_rows, int64_t* h_srcs, char* message) {
  const hipfeat::CoPlan p = hipfeat::build_collate_sources_plan(num_rows, h_first, h_src_offset, h_src_len, h_dst_offset, row_len, out_type);
  std::snprintf(message, 256, "%s", p.message.c_str());
  if (p.status != 0) return p.status;
  if (!p.sources) return -1;
  h_info[0] = 0;
  h_info[1] = p.arena_need;
  h_info[2] = p.out_need;
  h_info[3] = p.work_items;
  if (h_rows && !p.rows.empty()) std::memcpy(h_rows, p.rows.data(), p.rows.size() * sizeof(hipfeat::CoRow));
  if (h_srcs && !p.srcs.empty()) std::memcpy(h_srcs, p.srcs.data(), p.srcs.size() * sizeof(int64_t));
  return 0;
}

static hipfeat::TicketRing g_slots;
extern "C" void cs_slots_reset() { g_slots = hipfeat::TicketRing(); }
extern "C" long long cs_slots_plan() { return g_slots.take(); }
extern "C" int cs_slots_run(long long ticket) { return g_slots.release(ticket) ? 0 : 1; }

extern "C" int cs_max_sources() { return hipfeat::kCoMaxSources; }
extern "C" int cs_slots() { return hipfeat::kTicketSlots; }
extern "C" long long cs_first_source(long long pad) { return hipfeat::co_first_source(pad); }
extern "C" int cs_num_sources(long long pad) { return hipfeat::co_num_sources(pad); }
extern "C" long long cs_tiles(long long row_len, int out_type) { return hipfeat::co_tiles(row_len, out_type); }

#ifdef COLLATE_SOURCES_MAIN
#define CHECK(c)                                                                                        \
  do {                                                                                                  \
    if (!(c)) {                                                                                         \
      std::printf("FAILED %s (row_len %lld type %d k %d)\n", #c, (long long)row_len, (int)type, k);    \
      return 1;                                                                                         \
    }                                                                                                   \
  } while (0)

int main() {
  for (int32_t type : {hipfeat::kCoF32, hipfeat::kCoF16, hipfeat::kCoBF16})
    for (int64_t row_len : {1LL, 3LL, 4LL, 5LL, 8LL, 4095LL, 4096LL, 4097LL, 70001LL, 1LL << 33})
      for (int k : {0, 1, 2, 7, 32}) {
        // rows: k sources, none, k sources of no samples (far away: they read nothing)
        std::vector<int64_t> first = {0, k, k, 2 * k}, srcs;
        for (int c = 0; c < k; ++c) srcs.push_back(5 + c * (row_len + 3));
        for (int c = 0; c < k; ++c) srcs.push_back((1LL << 40) + c);
        const int64_t len[3] = {row_len, row_len, 0}, dst[3] = {0, 0, row_len};
        const hipfeat::CoPlan p = hipfeat::build_collate_sources_plan(3, first.data(), srcs.data(), len, dst, row_len, type);
        CHECK(p.status == 0 && p.sources && p.rows.size() == 3 && p.srcs == srcs);
        CHECK(p.work_items == 3 * hipfeat::co_tiles(row_len, type) && p.out_need == 3 * row_len);
        CHECK(p.arena_need == (k > 0 ? srcs[(size_t)k - 1] + row_len : 0));
        for (size_t r = 0; r < 3; ++r) {
          const hipfeat::CoRow& row = p.rows[r];
          const int64_t f = hipfeat::co_first_source(row.pad);
          const int n = hipfeat::co_num_sources(row.pad);
          CHECK(f == first[r] && n == first[r + 1] - first[r] && f + n <= (int64_t)p.srcs.size());
          CHECK(row.dst_off >= 0 && row.dst_off + row.len <= row_len);
          CHECK(n > 0 || row.len == 0);  // a row without sources is a row of padding: the kernel loads nothing for it
          for (int c = 0; c < n; ++c) CHECK(row.len == 0 || p.srcs[(size_t)(f + c)] + row.len <= p.arena_need);
          CHECK(n == 0 || row.src_off == p.srcs[(size_t)f]);
        }
      }
  std::printf("ok\n");
  return 0;
}
#endif
