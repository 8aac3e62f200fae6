// Test shim (CPU only): a C entry point around lhotse_amd/csrc/featmix_tables.hpp and ticket_slots.hpp -- the whole of what
// hipfeat_featmix_plan decides, the 16 ticket slots every ticketed handle shares included -- so that tests/test_featmix_abi.py can check
// the tables and the plan-time errors without a device.  With -DFEATMIX_TABLES_MAIN it is a stand-alone program (also built with
// -fsanitize=address,undefined) that walks the same code over feature counts and frame counts around the tile and group boundaries and
// checks the invariants the kernels rely on for their bounds.
#include "../../lhotse_amd/csrc/featmix_tables.hpp"
#include "../../lhotse_amd/csrc/ticket_slots.hpp"

#include <cstdio>
#include <cstring>

// returns the status; h_info[4] as hipfeat_featmix_plan (ticket 0); h_cuts / h_tracks (may be NULL): the descriptors of 32 / 48 bytes;
// message: 256 bytes
extern "C" int ft_plan(long long num_cuts, const int64_t* h_track_first, const int32_t* h_form, const int64_t* h_num_frames, const double* h_pad_value,
                       const int64_t* h_dst_first, const int32_t* h_ref_track, const int64_t* h_src_offset, const int64_t* h_src_rows, const int64_t* h_frames,
                       const int32_t* h_dtype, const int64_t* h_first, const double* h_snr_db, const double* h_value, long long num_features, long long row_frames,
                       int64_t* h_info, void* h_cuts, void* h_tracks, char* message) {
  const hipfeat::FmPlan p = hipfeat::build_featmix_plan(num_cuts, h_track_first, h_form, h_num_frames, h_pad_value, h_dst_first, h_ref_track, h_src_offset,
                                                        h_src_rows, h_frames, h_dtype, h_first, h_snr_db, h_value, num_features, row_frames);
  std::snprintf(message, 256, "%s", p.message.c_str());
  if (p.status != 0) return p.status;
  h_info[0] = 0;
  h_info[1] = p.arena_need;
  h_info[2] = p.energy_items;
  h_info[3] = p.fold_items;
  if (h_cuts) std::memcpy(h_cuts, p.cuts.data(), p.cuts.size() * sizeof(hipfeat::FmCut));
  if (h_tracks && !p.tracks.empty()) std::memcpy(h_tracks, p.tracks.data(), p.tracks.size() * sizeof(hipfeat::FmTrack));
  return 0;
}

// the ticket ring (ticket_slots.hpp): ft_slots_plan takes the next ticket (-1: all kTicketSlots are planned and not yet run), ft_slots_run
// frees one (0: it was planned, 1: unknown ticket)
static hipfeat::TicketRing g_slots;
extern "C" void ft_slots_reset() { g_slots = hipfeat::TicketRing(); }
extern "C" long long ft_slots_plan() { return g_slots.take(); }
extern "C" int ft_slots_run(long long ticket) { return g_slots.release(ticket) ? 0 : 1; }

extern "C" int ft_tile() { return hipfeat::kFmTile; }
extern "C" int ft_energy_block() { return hipfeat::kFmEnergyBlock; }
extern "C" int ft_max_tracks() { return hipfeat::kFmMaxTracks; }
extern "C" int ft_slots() { return hipfeat::kTicketSlots; }
extern "C" long long ft_tiles(long long row_len) { return hipfeat::fm_tiles(row_len); }

#ifdef FEATMIX_TABLES_MAIN
#define CHECK(c)                                                                                \
  do {                                                                                          \
    if (!(c)) {                                                                                 \
      std::printf("FAILED %s (F %lld frames %lld)\n", #c, (long long)F, (long long)frames);     \
      return 1;                                                                                 \
    }                                                                                           \
  } while (0)

int main() {
  for (int64_t F : {1LL, 3LL, 4LL, 23LL, 80LL, 257LL, 4096LL, 4097LL})
    for (int64_t frames : {1LL, 2LL, 3LL, 51LL, 52LL, 77LL, 1024LL, 3000LL, 100000LL}) {
      const int64_t row_len = (frames + 2) * F, tiles = hipfeat::fm_tiles(row_len);
      // whatever the row's alignment (head = 0 ... 3 elements behind a 16-byte boundary), the tiles cover [0, head + row_len) and the last
      // one is not empty for the largest head
      for (int64_t head = 0; head < 4; ++head) CHECK(tiles * hipfeat::kFmTile >= head + row_len);
      CHECK((tiles - 1) * hipfeat::kFmTile < 3 + row_len);
      // cut 0: a copy of a binary16 track with one stored row too few; cut 1: a fold of a constant track, a float32 track with one row too
      // many and an SNR, and a track of no frames; the mix is one frame longer than the cut
      const int64_t first[3] = {0, 1, 4}, nf[2] = {frames + 1, frames}, dst[2] = {1, 2};
      const int32_t form[2] = {hipfeat::kFmCopy, hipfeat::kFmFold}, ref[2] = {-1, 1}, dtype[4] = {1, 0, 0, 0};
      const double pad[2] = {-23.0, 0.0}, snr[4] = {NAN, NAN, 10.0, 5.0}, val[4] = {0, -23.0, 0, 0};
      const int64_t so[4] = {6, -1, 1LL << 33, 12}, rows[4] = {frames > 1 ? frames - 1 : 1, 1, frames + 1, 0}, fr[4] = {frames, 1, frames, 0}, off[4] = {0, 0, 1, 5};
      const hipfeat::FmPlan p = hipfeat::build_featmix_plan(2, first, form, nf, pad, dst, ref, so, rows, fr, dtype, off, snr, val, F, frames + 2);
      CHECK(p.status == 0 && p.cuts.size() == 2 && p.tracks.size() == 4);
      CHECK(p.fold_items == 2 * tiles && p.out_need == 2 * row_len && p.row_len == row_len);
      CHECK(p.arena_need == (1LL << 33) + frames * F * 4);  // (the row too many is not read; the track of no frames reads nothing)
      CHECK(p.cuts[1].mix_frames == frames + 1 && p.cuts[1].ref_track == 2 && p.cuts[0].ref_track == -1);
      const int64_t parts = (frames * F + hipfeat::kFmEnergyBlock - 1) / hipfeat::kFmEnergyBlock;
      CHECK(p.energy_items == parts && p.tracks[2].part_count == parts && p.tracks[2].part_first == 0);
      CHECK(p.tracks[0].part_count == 0 && p.tracks[1].part_count == 0 && p.tracks[3].part_count == 0 && p.tracks[3].part_first == parts);
      for (const hipfeat::FmCut& c : p.cuts) CHECK(c.dst_first >= 0 && (int64_t)c.dst_first + c.num_frames <= frames + 2);
      for (const hipfeat::FmTrack& t : p.tracks) CHECK(t.rows >= t.frames - 1 && t.rows <= t.frames + 1 && (int64_t)(t.first + t.frames) * F <= INT32_MAX / 2);
    }
  std::printf("ok\n");
  return 0;
}
#endif
