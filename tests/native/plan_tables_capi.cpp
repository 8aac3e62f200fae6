// Test shim (CPU only): C entry points around lhotse_amd/csrc/plan_tables.hpp so that tests/test_plan_tables.py can check the very
// tables and scalars a plan uploads and keeps.  pt_build runs one family's builder on `a` (the arguments the setup in hipfeat.hip passes:
// window rows and the kernel's geometry constants, listed per family below) and keeps the result: its tables in upload order and
// its scalars, read back with pt_table_* / pt_scalar.
#include <string>

#include "../../lhotse_amd/csrc/plan_tables.hpp"

using namespace hipfeat;

static std::vector<std::vector<unsigned char>> g_tables;
static std::vector<long long> g_scalars;

template <typename T>
static void put(const T* v, size_t n) {
  const unsigned char* b = reinterpret_cast<const unsigned char*>(v);
  g_tables.emplace_back(b, b + n * sizeof(T));
}

// scalars: lds, shared_floats, wtab_off, ltab_off, xs_floats, waves, mode, nrows, sch_nsets, sch_steps, w_nsets, w_steps[4], w_step0[4],
// tws_off, tw32_off, fixed, w12
static int put_wave_auto(const WaveAutoTables& t) {
  if (!t.fits) return 0;
  put(t.image.data(), t.image.size());
  if (!t.dct.empty()) put(t.dct.data(), t.dct.size());
  if (!t.twp.empty()) put(t.twp.data(), t.twp.size());
  g_scalars = {(long long)t.lds, t.shared_floats, t.wtab_off, t.ltab_off, t.xs_floats, t.waves, t.mode, t.nrows, t.sch_nsets, t.sch_steps, t.w_nsets};
  g_scalars.insert(g_scalars.end(), t.w_steps, t.w_steps + 4);
  g_scalars.insert(g_scalars.end(), t.w_step0, t.w_step0 + 4);
  g_scalars.insert(g_scalars.end(), {t.tws_off, t.tw32_off, t.fixed, t.w12});
  return 1;
}

// in5: N, shift, K, M, C.  Returns 1, or 0 when the configuration does not fit the family's schedule, -1 for an unknown family.
extern "C" int pt_build(const char* family, const int* in5, const float* window, const float* mel, const float* dct, const float* lifter, const int* a) {
  g_tables.clear();
  g_scalars.clear();
  PlanInputs in;
  in.N = in5[0], in.shift = in5[1], in.K = in5[2], in.M = in5[3], in.C = in5[4];
  in.window = window, in.mel = mel, in.dct = dct, in.lifter = lifter;
  const std::string f = family;
  const WaveAutoGeom g{a[1], a[2], a[3], a[4], a[5]};  // (wave-autonomous families) a: nrows, prow_stride, max_sets, max_steps, waves, region, ...
  if (f == "fft512c") return put_wave_auto(build_fft512c_tables(in, a[0], g, a[6], a[7]));  // ..., dct_chunks, dct_chunks_small
  if (f == "fft256c") return put_wave_auto(build_fft256c_tables(in, a[0], g));
  // ..., split_steps, waves_fixed, fixed instance?, its 3 steps (, w12_want, lds_budget)
  if (f == "fft1024c") return put_wave_auto(build_fft1024c_tables(in, a[0], g, a[6], a[7], a[8] ? a + 9 : nullptr));
  if (f == "fft2048c") return put_wave_auto(build_fft2048c_tables(in, a[0], g, a[6], a[7], a[8] ? a + 9 : nullptr, a[12] != 0, (size_t)a[13]));
  if (f == "whisper3") return put_wave_auto(build_whisper3_tables(in, g, a[6], a[7]));  // a[0] unused; ..., span, tail
  if (f == "tile") {  // a: nrows, lanes, prow_stride, max_groups0, max_groups1, tile_frames, wave_region, rotated_split
    const TileTables t = build_tile_tables(in, a[0], {a[1], a[2], a[3], a[4], a[5], a[6], a[7] != 0});
    if (!t.fits) return 0;
    put(t.consts.data(), t.consts.size());
    put(t.mel_a.data(), t.mel_a.size());
    put(t.work, 4);
    put(t.mel_a4.data(), t.mel_a4.size());
    put(t.dct.data(), t.dct.size());
    g_scalars = {(long long)t.lds, t.xs_floats, t.lm_stride, t.dct_groups, t.nrows};
    return 1;
  }
  if (f == "whisper2") {
    const Whisper2Tables t = build_whisper2_tables(in);
    put(t.cs.data(), t.cs.size());
    put(t.tw.data(), t.tw.size());
    put(t.mel.data(), t.mel.size());
    put(t.sched.data(), t.sched.size());
    g_scalars.assign(t.load, t.load + 4);
    return 1;
  }
  if (f == "wave") {  // a: H
    const WaveTables t = build_wave_tables(in, a[0]);
    put(t.blob.data(), t.blob.size());
    g_scalars = {(long long)t.lds, t.dct_in_lds};
    return 1;
  }
  if (f == "band") {  // a: j0, j1 -> scalars lo, hi
    const MelBand b = mel_band(mel, in.M, in.K, a[0], a[1]);
    g_scalars = {b.lo, b.hi};
    return 1;
  }
  return -1;
}

extern "C" int pt_num_tables() { return (int)g_tables.size(); }
extern "C" long long pt_table_bytes(int i) { return (long long)g_tables[(size_t)i].size(); }
extern "C" void pt_table_copy(int i, void* dst) { std::memcpy(dst, g_tables[(size_t)i].data(), g_tables[(size_t)i].size()); }
extern "C" int pt_num_scalars() { return (int)g_scalars.size(); }
extern "C" long long pt_scalar(int i) { return g_scalars[(size_t)i]; }
