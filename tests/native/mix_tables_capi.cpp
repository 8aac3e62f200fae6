// Test shim (CPU only): a C entry point around lhotse_amd/csrc/mix_tables.hpp -- the whole of what hipfeat_mix_plan decides -- so that
// tests/test_mix_abi.py can check the tables and the plan-time errors without a device.  With -DMIX_TABLES_MAIN it is a stand-alone
// program (also built with -fsanitize=address,undefined) that walks the same code over track lengths and offsets around the block
// boundaries and checks the invariants the kernels rely on for their bounds.
#include "../../lhotse_amd/csrc/mix_tables.hpp"

#include <cstdio>
#include <cstring>

// returns the status; h_out_offsets / h_out_num_samples / h_info[4] as hipfeat_mix_plan (ticket 0), untouched by a refusal; h_cuts, h_tracks
// (may be NULL): num_cuts and h_track_first[num_cuts] descriptors of 32 bytes; message: 256 bytes
extern "C" int mt_plan(long long num_cuts, const int64_t* h_track_first, const int64_t* h_src_offset, const int64_t* h_src_len, const int64_t* h_dst_offset,
                       const double* h_snr_db, const int32_t* h_ref_track, const int64_t* h_max_samples, long long tail_start, int64_t* h_out_offsets,
                       int64_t* h_out_num_samples, int64_t* h_info, void* h_cuts, void* h_tracks, char* message) {
  const hipfeat::MixPlan p =
      hipfeat::build_mix_plan(num_cuts, h_track_first, h_src_offset, h_src_len, h_dst_offset, h_snr_db, h_ref_track, h_max_samples, tail_start);
  std::snprintf(message, 256, "%s", p.message.c_str());
  if (p.status != 0) return p.status;
  for (size_t c = 0; c < p.cuts.size(); ++c) {
    if (h_out_offsets) h_out_offsets[c] = p.cuts[c].out_off;
    if (h_out_num_samples) h_out_num_samples[c] = p.cuts[c].out_len;
  }
  h_info[0] = 0;
  h_info[1] = p.arena_need;
  h_info[2] = p.energy_items;
  h_info[3] = p.mix_items;
  if (h_cuts) std::memcpy(h_cuts, p.cuts.data(), p.cuts.size() * sizeof(hipfeat::MixCut));
  if (h_tracks) std::memcpy(h_tracks, p.tracks.data(), p.tracks.size() * sizeof(hipfeat::MixTrack));
  return 0;
}

extern "C" int mt_block() { return hipfeat::kMixBlock; }
extern "C" int mt_energy_block() { return hipfeat::kMixEnergyBlock; }
extern "C" int mt_max_tracks() { return hipfeat::kMixMaxTracks; }

#ifdef MIX_TABLES_MAIN
#define CHECK(c)                                                                       \
  do {                                                                                 \
    if (!(c)) {                                                                        \
      std::printf("FAILED %s (len %lld offset %lld)\n", #c, (long long)n, (long long)off); \
      return 1;                                                                        \
    }                                                                                  \
  } while (0)

int main() {
  for (int64_t n : {1LL, 3LL, 4095LL, 4096LL, 4097LL, 16383LL, 16384LL, 16385LL, 70001LL, (long long)(INT32_MAX / 2) - 9})
    for (int64_t off : {0LL, 1LL, 3LL, 4LL, 5LL, 9LL}) {
      // cut 0: a reference track, a scaled track at `off`, a padding track of off + 2 samples; cut 1: one plain track of 7 samples
      const int64_t first[3] = {0, 3, 4}, src[4] = {0, n, -1, 1LL << 33}, len[4] = {n, n, off + 2, 7}, dst[4] = {0, off, 0, 0};
      const double snr[4] = {NAN, 10.0, NAN, NAN};
      const int32_t ref[2] = {0, -1};
      const int64_t tail_start = (1LL << 33) + 7;
      const hipfeat::MixPlan p = hipfeat::build_mix_plan(2, first, src, len, dst, snr, ref, nullptr, tail_start);
      CHECK(p.status == 0 && p.cuts.size() == 2 && p.tracks.size() == 4);
      const hipfeat::MixCut& cd = p.cuts[0];
      const int64_t total = std::max(off + n, off + 2), items = p.cuts[1].item_first, parts = (n + hipfeat::kMixEnergyBlock - 1) / hipfeat::kMixEnergyBlock;
      CHECK(cd.out_len == total && cd.out_off == ((tail_start + 3) & ~3LL) && cd.out_off % 4 == 0 && p.cuts[1].out_off % 4 == 0);
      // every output sample lies in exactly one mix item, and no item is empty; the furthest sample a lane may touch fits an int
      CHECK(items * hipfeat::kMixBlock >= total && (items - 1) * hipfeat::kMixBlock < total && items * hipfeat::kMixBlock + 3 <= INT32_MAX);
      // the reference and the scaled track each own `parts` consecutive partials that cover their samples; the others own none
      CHECK(p.tracks[0].part_first == 0 && p.tracks[0].part_count == parts && p.tracks[1].part_first == parts && p.tracks[1].part_count == parts);
      CHECK(parts * hipfeat::kMixEnergyBlock >= n && (parts - 1) * hipfeat::kMixEnergyBlock < n);
      CHECK(p.tracks[2].part_count == 0 && p.tracks[3].part_count == 0 && p.energy_items == 2 * parts && p.mix_items == items + 1);
      CHECK(p.tracks[1].ratio == std::pow(10.0, -1.0) && p.tracks[0].ratio == -1.0 && p.tracks[2].src_off == -1);
      CHECK(p.cuts[1].out_off == cd.out_off + ((total + 3) & ~3LL) && p.arena_need == p.cuts[1].out_off + 8);
    }
  std::printf("ok\n");
  return 0;
}
#endif
