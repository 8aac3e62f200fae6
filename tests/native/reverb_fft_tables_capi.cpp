// Test shim (CPU only): a C entry point around lhotse_amd/csrc/reverb_fft_tables.hpp -- the whole of what hipfeat_reverb_plan_method
// decides -- so that tests/test_reverb_fft_abi.py can check the tables and the plan-time errors without a device.  With
// -DREVERB_FFT_TABLES_MAIN it is a stand-alone program (also built with -fsanitize=address,undefined) that walks the same code over
// lengths, tap counts and shifts around the block boundaries and checks the invariants the kernels rely on for their bounds.
#include "../../lhotse_amd/csrc/reverb_fft_tables.hpp"

#include <cstdio>
#include <cstring>

// returns the status; h_out_offsets / h_info[8] as hipfeat_reverb_plan_method (ticket 0), untouched by a refusal; h_direct / h_fft / h_rirs
// (may be NULL): room for num_items descriptors each (48 / 80 / 32 bytes); h_counts[3] = how many of each were written; message: 256 bytes
extern "C" int rf_plan(long long num_items, const int64_t* h_src_offset, const int64_t* h_src_len, const int64_t* h_rir_offset, const int64_t* h_rir_len,
                       const int64_t* h_shift, const int32_t* h_normalize, long long tail_start, int method, long long min_fft_taps, int64_t* h_out_offsets,
                       int64_t* h_info, void* h_direct, void* h_fft, void* h_rirs, int64_t* h_counts, char* message) {
  const hipfeat::RvMethodPlan p =
      hipfeat::build_reverb_plan_method(num_items, h_src_offset, h_src_len, h_rir_offset, h_rir_len, h_shift, h_normalize, tail_start, method, min_fft_taps);
  std::snprintf(message, 256, "%s", p.message.c_str());
  if (p.status != 0) return p.status;
  if (h_out_offsets)
    for (size_t i = 0; i < p.out_offsets.size(); ++i) h_out_offsets[i] = p.out_offsets[i];
  h_info[0] = 0;
  h_info[1] = p.arena_need;
  h_info[2] = p.work_items;
  h_info[3] = 2 * p.work_items + p.fft_partials();
  h_info[4] = p.fft.a_work;
  h_info[5] = p.fft.b_work;
  h_info[6] = p.fft.g_work;
  h_info[7] = (int64_t)p.fft.rirs.size();
  if (h_direct) std::memcpy(h_direct, p.items.data(), p.items.size() * sizeof(hipfeat::RvItem));
  if (h_fft) std::memcpy(h_fft, p.fft.items.data(), p.fft.items.size() * sizeof(hipfeat::RfItem));
  if (h_rirs) std::memcpy(h_rirs, p.fft.rirs.data(), p.fft.rirs.size() * sizeof(hipfeat::RfRir));
  if (h_counts) h_counts[0] = (int64_t)p.items.size(), h_counts[1] = (int64_t)p.fft.items.size(), h_counts[2] = (int64_t)p.fft.rirs.size();
  return 0;
}

extern "C" int rf_block() { return hipfeat::kRfBlock; }
extern "C" int rf_spec_floats() { return hipfeat::kRfSpecFloats; }
extern "C" int rf_waves() { return hipfeat::kRfWaves; }
extern "C" int rf_grid_slots() { return hipfeat::kRfGridSlots; }

#ifdef REVERB_FFT_TABLES_MAIN
#define CHECK(c)                                                                                                        \
  do {                                                                                                                  \
    if (!(c)) {                                                                                                         \
      std::printf("FAILED %s (samples %lld taps %lld shift %lld)\n", #c, (long long)n, (long long)taps, (long long)s);  \
      return 1;                                                                                                         \
    }                                                                                                                   \
  } while (0)

int main() {
  constexpr int64_t B = hipfeat::kRfBlock;
  for (int64_t n : {1LL, 1023LL, 1024LL, 1025LL, 2047LL, 2048LL, 2049LL, 70001LL, (long long)(INT32_MAX / 2)})
    for (int64_t taps : {1LL, 2LL, 1023LL, 1024LL, 1025LL, 4097LL, (long long)(INT32_MAX / 2)})
      for (int64_t s : {(int64_t)0, (int64_t)1, (int64_t)1023, (int64_t)1024, taps / 2, taps - 1}) {
        if (s >= taps) continue;
        const int64_t far = 1LL << 33;
        // items 0 and 2 share an impulse response; item 1 has one of its own (of the same length, elsewhere)
        const int64_t src[3] = {0, far, far}, len[3] = {n, 5, 5}, rir[3] = {far + 5, far + 5 + taps, far + 5}, rl[3] = {taps, taps, taps}, shift[3] = {s, 0, s};
        const int32_t norm[3] = {1, 0, 0};
        const int64_t tail_start = far + 5 + 2 * taps + 1;
        const hipfeat::RvMethodPlan p = hipfeat::build_reverb_plan_method(3, src, len, rir, rl, shift, norm, tail_start, hipfeat::kRvFft, 0);
        CHECK(p.status == 0 && p.items.empty() && p.fft.items.size() == 3 && p.fft.rirs.size() == 2);
        const hipfeat::RfPlan& f = p.fft;
        const hipfeat::RfItem& it = f.items[0];
        const int64_t parts = (taps + B - 1) / B;
        CHECK(it.parts == parts && f.rirs[0].parts == parts && f.rir_work == 2 * parts && f.items[2].hspec_off == it.hspec_off && f.items[1].hspec_off != it.hspec_off);
        // every kept output lies in exactly one output block
        CHECK((int64_t)it.j0 * B <= s && s < ((int64_t)it.j0 + 1) * B);
        const int64_t j1 = (int64_t)it.j0 + it.ny - 1;
        CHECK(j1 * B <= s + n - 1 && s + n - 1 < (j1 + 1) * B && it.ny >= 1);
        // every sample of x lies in the new half of exactly one input block, and every input block an output block reads exists or is all zero
        CHECK((int64_t)it.nx * B >= n || (int64_t)it.nx - 1 == j1);
        for (int64_t j : {(int64_t)it.j0, j1}) {
          const int64_t p_lo = j - it.nx + 1 > 0 ? j - it.nx + 1 : 0, p_hi = parts - 1 < j ? parts - 1 : j;
          CHECK(p_lo <= p_hi && j - p_hi >= 0 && j - p_lo < it.nx);
          if (p_lo > 0) CHECK((j - p_lo + 1 - 1) * B >= n);  // the skipped blocks i = j - p > nx - 1 start at or behind the end of x
        }
        // the workspace: behind the outputs, 16-byte aligned, the formula, and inside the arena floats the plan reports
        const int64_t out_end = p.out_offsets[2] + 8;
        CHECK(f.rirs[0].spec_off == out_end && f.rirs[0].spec_off % 4 == 0 && f.rirs[1].spec_off == out_end + parts * hipfeat::kRfSpecFloats);
        CHECK(it.xspec_off == out_end + f.rir_work * hipfeat::kRfSpecFloats && f.items[2].xspec_off + (int64_t)f.items[2].nx * hipfeat::kRfSpecFloats == p.arena_need);
        CHECK(f.a_work == f.rir_work + f.x_total && f.x_total == (int64_t)it.nx + f.items[1].nx + f.items[2].nx && p.arena_need == out_end + f.a_work * hipfeat::kRfSpecFloats);
        CHECK(it.a_first == f.rir_work && f.items[1].a_first == it.a_first + it.nx && f.items[1].b_first == it.ny && f.items[1].g_first == (n + 2047) / 2048);
        CHECK(f.b_work == (int64_t)it.ny + f.items[1].ny + f.items[2].ny && p.fft_partials() == f.x_total + f.b_work);
        // auto at the threshold: >= takes the FFT route; a negative threshold and an unknown method are refused
        const hipfeat::RvMethodPlan a = hipfeat::build_reverb_plan_method(3, src, len, rir, rl, shift, norm, tail_start, hipfeat::kRvAuto, taps);
        const hipfeat::RvMethodPlan d = hipfeat::build_reverb_plan_method(3, src, len, rir, rl, shift, norm, tail_start, hipfeat::kRvAuto, taps + 1);
        CHECK(a.status == 0 && a.fft.items.size() == 3 && d.status == 0 && d.fft.items.empty() && d.items.size() == 3 && d.arena_need == out_end);
        CHECK(hipfeat::build_reverb_plan_method(3, src, len, rir, rl, shift, norm, tail_start, hipfeat::kRvAuto, -1).status == 1);
        CHECK(hipfeat::build_reverb_plan_method(3, src, len, rir, rl, shift, norm, tail_start, 3, 0).status == 1);
      }
  std::printf("ok\n");
  return 0;
}
#endif
