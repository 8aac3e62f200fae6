// Test shim (CPU only): a C entry point around lhotse_amd/csrc/collate_tables.hpp and ticket_slots.hpp -- the whole of what
// hipfeat_collate_plan decides, the 16 ticket slots every ticketed handle shares included -- so that
// tests/test_collate_abi.py can check the table and the plan-time errors without a device.  With -DCOLLATE_TABLES_MAIN it is a stand-alone program (also built with -fsanitize=address,undefined) that walks the same code over row
// lengths around the tile and group boundaries and checks the invariants the kernel relies on for its bounds.
#include "../../lhotse_amd/csrc/collate_tables.hpp"
#include "../../lhotse_amd/csrc/ticket_slots.hpp"

#include <cstdio>
#include <cstring>

// returns the status; h_info[4] as hipfeat_collate_plan (ticket 0); h_rows (may be NULL): num_rows descriptors of 32 bytes; message: 256 bytes
extern "C" int ct_plan(long long num_rows, const int64_t* h_src_offset, const int64_t* h_src_len, const int64_t* h_dst_offset, long long row_len, int out_type,
                       int64_t* h_info, void* h_rows, char* message) {
  const hipfeat::CoPlan p = hipfeat::build_collate_plan(num_rows, h_src_offset, h_src_len, h_dst_offset, row_len, out_type);
  std::snprintf(message, 256, "%s", p.message.c_str());
  if (p.status != 0) return p.status;
  h_info[0] = 0;
  h_info[1] = p.arena_need;
  h_info[2] = p.out_need;
  h_info[3] = p.work_items;
  if (h_rows && !p.rows.empty()) std::memcpy(h_rows, p.rows.data(), p.rows.size() * sizeof(hipfeat::CoRow));
  return 0;
}

// the ticket ring (ticket_slots.hpp): ct_slots_plan takes the next ticket (-1: all kTicketSlots are planned and not yet run), ct_slots_run
// frees one (0: it was planned, 1: unknown ticket)
static hipfeat::TicketRing g_slots;
extern "C" void ct_slots_reset() { g_slots = hipfeat::TicketRing(); }
extern "C" long long ct_slots_plan() { return g_slots.take(); }
extern "C" int ct_slots_run(long long ticket) { return g_slots.release(ticket) ? 0 : 1; }

extern "C" int ct_tile() { return hipfeat::kCoTile; }
extern "C" int ct_slots() { return hipfeat::kTicketSlots; }
extern "C" long long ct_tiles(long long row_len, int out_type) { return hipfeat::co_tiles(row_len, out_type); }

#ifdef COLLATE_TABLES_MAIN
#define CHECK(c)                                                                              \
  do {                                                                                        \
    if (!(c)) {                                                                               \
      std::printf("FAILED %s (row_len %lld type %d)\n", #c, (long long)row_len, (int)type);   \
      return 1;                                                                               \
    }                                                                                         \
  } while (0)

int main() {
  for (int32_t type : {hipfeat::kCoF32, hipfeat::kCoF16, hipfeat::kCoBF16})
    for (int64_t row_len : {1LL, 3LL, 4LL, 7LL, 8LL, 9LL, 4088LL, 4089LL, 4093LL, 4096LL, 4097LL, 8192LL, 70001LL, 1LL << 33}) {
      const int64_t V = hipfeat::co_vec(type), tiles = hipfeat::co_tiles(row_len, type);
      // whatever the row's alignment (head = 0 ... V - 1 elements behind a 16-byte boundary), the tiles cover [0, head + row_len) and the
      // last one is not empty for the largest head
      for (int64_t head = 0; head < V; ++head) CHECK(tiles * hipfeat::kCoTile >= head + row_len);
      CHECK((tiles - 1) * hipfeat::kCoTile < (V - 1) + row_len);
      const int64_t src[3] = {5, 1LL << 40, 77}, len[3] = {row_len, 0, row_len > 1 ? row_len - 1 : 0}, dst[3] = {0, row_len, row_len > 1 ? 1 : 0};
      const hipfeat::CoPlan p = hipfeat::build_collate_plan(3, src, len, dst, row_len, type);
      CHECK(p.status == 0 && p.rows.size() == 3 && p.work_items == 3 * tiles && p.out_need == 3 * row_len);
      CHECK(p.arena_need == std::max<int64_t>(5 + row_len, len[2] > 0 ? 77 + len[2] : 0));  // (the row of padding at 2^40 reads nothing)
      for (const hipfeat::CoRow& r : p.rows) CHECK(r.dst_off >= 0 && r.dst_off + r.len <= row_len);
    }
  std::printf("ok\n");
  return 0;
}
#endif
