// Test shim (CPU only): C entry points around lhotse_amd/csrc/sinc_tables.hpp -- the geometry of a rate pair, the window of a phase, the
// weight formula, the whole of what hipfeat_sinc_plan decides -- so that tests/test_sinc_tables.py and tests/test_sinc_abi.py can check
// them without a device.  With -DSINC_TABLES_MAIN it is a stand-alone program (also built with -fsanitize=address,undefined) that walks
// the same code over more ratios and row lengths and checks what the kernel relies on for its bounds.
#include "../../lhotse_amd/csrc/sinc_tables.hpp"

#include <cstdio>
#include <cstring>

using namespace hipfeat;

// dims[4] = {orig, new, width, W}; returns 0 served, 1 invalid, 3 unsupported
extern "C" int st_supported(long long src_rate, long long dst_rate, int32_t* dims) { return sinc_supported(src_rate, dst_rate, dims); }

extern "C" int st_constants(int which) { return which == 0 ? kSincPhases : which == 1 ? kSincHops : kSincMaxW; }

// first[new] and weights[new][W] of reduced rates orig : new, as the kernel evaluates them (this machine's libm)
extern "C" void st_filter(int orig, int nw, int32_t* first, float* weights) {
  const int width = (int)sinc_width(orig, nw), W = 2 * width + 2;
  const double base = sinc_base(orig, nw);
  for (int ph = 0; ph < nw; ++ph) {
    const int i0 = sinc_first_tap(ph, orig, nw, width, base);
    first[ph] = i0;
    if (weights)
      for (int d = 0; d < W; ++d) weights[(size_t)ph * W + d] = sinc_weight(ph, i0 + d, orig, nw, width, base);
  }
}

// returns the status; h_out_len[num_rows]; h_info[4] as hipfeat_sinc_plan (ticket 0); h_rows (may be NULL): up to num_rows descriptors of
// 64 bytes, *h_num_rows of them written; message: 256 bytes
extern "C" int st_plan(long long num_rows, const int64_t* h_in_offset, const int64_t* h_in_len, const int32_t* h_src_rate, const int32_t* h_dst_rate,
                       const int64_t* h_out_offset, long long arena_floats, int64_t* h_out_len, int64_t* h_info, void* h_rows, int64_t* h_num_rows, char* message) {
  const SincPlan p = build_sinc_plan(num_rows, h_in_offset, h_in_len, h_src_rate, h_dst_rate, h_out_offset, arena_floats);
  std::snprintf(message, 256, "%s", p.message.c_str());
  if (p.status != 0) return p.status;
  for (long long i = 0; i < num_rows; ++i) h_out_len[i] = p.out_len[(size_t)i];
  h_info[0] = 0;
  h_info[1] = p.arena_need;
  h_info[2] = p.workgroups;
  h_info[3] = p.max_w;
  if (h_num_rows) *h_num_rows = (int64_t)p.rows.size();
  if (h_rows && !p.rows.empty()) std::memcpy(h_rows, p.rows.data(), p.rows.size() * sizeof(SincRow));
  return 0;
}

// The (row, phase, hop) triples of workgroup `wg` of a planned table, exactly as sinc_kernel walks them: count[out_len] of the row that
// owns the workgroup is incremented per output sample it would store.  Returns the row's index in the table, -1: out of range.
extern "C" int st_walk(const void* h_rows, int num_rows, int wg, int32_t* count) {
  const SincRow* rows = static_cast<const SincRow*>(h_rows);
  int lo = 0, hi = num_rows - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].wg_first <= wg) lo = mid; else hi = mid - 1;
  }
  const SincRow& r = rows[lo];
  const int k = wg - r.wg_first;
  if (k < 0 || k >= sinc_row_workgroups(r)) return -1;
  const int chunk = k / r.tiles, tile = k - chunk * r.tiles;
  for (int tid = 0; tid < kSincPhases; ++tid) {
    const int ph = tile * kSincPhases + tid;
    if (ph >= r.nw || ph >= r.out_len) continue;
    const int j1 = std::min((chunk + 1) * kSincHops, r.hops);
    for (int j = chunk * kSincHops; j < j1; ++j) {
      const int64_t o = (int64_t)j * r.nw + ph;
      if (o >= r.out_len) break;
      ++count[o];
    }
  }
  return lo;
}

#ifdef SINC_TABLES_MAIN
#define CHECK(c)                                                                                         \
  do {                                                                                                   \
    if (!(c)) {                                                                                          \
      std::printf("FAILED %s (%d:%d, row of %lld)\n", #c, (int)orig, (int)nw, (long long)n);             \
      return 1;                                                                                          \
    }                                                                                                    \
  } while (0)

int main() {
  const int ratios[][2] = {{441, 160}, {160, 441}, {800, 467}, {467, 800}, {8000, 4673}, {4673, 8000}, {8000, 3501}, {3501, 8000}, {8000, 7999},
                           {7999, 8000}, {48, 7},  {7, 16},    {16, 7},    {2, 1},       {1, 2},       {11127, 16000}, {255, 256},  {257, 256}};
  for (const auto& ra : ratios) {
    const int orig = ra[0], nw = ra[1];
    int64_t n = 0;
    int32_t dims[4];
    CHECK(sinc_supported(orig, nw, dims) == 0 && dims[0] == orig && dims[1] == nw && dims[3] == 2 * dims[2] + 2 && dims[3] <= kSincMaxW);
    const int width = dims[2], W = dims[3], kw = 2 * width + orig;
    const double base = sinc_base(orig, nw);
    std::vector<int32_t> first((size_t)nw);
    st_filter(orig, nw, first.data(), nullptr);
    for (int ph = 0; ph < nw; ++ph) {
      const int i0 = first[(size_t)ph];
      // the window holds every live tap of the dense bank's row, and a clamped tap on either side
      CHECK(!sinc_live(ph, i0, orig, nw, width, base) && sinc_live(ph, i0 + 1, orig, nw, width, base) && !sinc_live(ph, i0 + W - 1, orig, nw, width, base));
      CHECK(i0 >= -1 && i0 + 1 < kw);
      for (int i : {0, i0 - 1, i0 + W, kw - 1})
        if (i >= 0 && i < kw && (i < i0 || i >= i0 + W)) CHECK(sinc_weight(ph, i, orig, nw, width, base) == 0.0f);
    }
    // every (row, phase, hop) once, nothing stored outside [0, out_len); what a lane reads is tested against [0, in_len) sample by sample
    for (int64_t len : {0LL, 1LL, 2LL, (long long)orig - 1, (long long)orig, (long long)orig + 1, 3LL * orig + 5, 70LL * orig + 3}) {
      n = len;
      const int64_t in_off[2] = {0, 1LL << 33}, in_len[2] = {n, n}, out_off[2] = {1LL << 32, 1LL << 34};
      const int32_t src[2] = {orig * 2, orig * 3}, dst[2] = {nw * 2, nw * 3};
      const SincPlan p = build_sinc_plan(2, in_off, in_len, src, dst, out_off, (1LL << 35));
      CHECK(p.status == 0 && p.out_len[0] == sinc_out_len(n, orig, nw) && p.out_len[1] == p.out_len[0]);
      CHECK(p.rows.size() == (p.out_len[0] > 0 ? 2u : 0u));
      if (p.rows.empty()) continue;
      std::vector<int32_t> count((size_t)p.out_len[0], 0);
      for (int wg = 0; wg < p.workgroups; ++wg) {
        const int row = st_walk(p.rows.data(), (int)p.rows.size(), wg, count.data());
        CHECK(row == (wg < p.rows[1].wg_first ? 0 : 1));
      }
      for (int32_t c : count) CHECK(c == 2);
      CHECK(p.rows[0].out_len <= (int64_t)p.rows[0].hops * nw && (int64_t)(p.rows[0].hops - 1) * nw < p.rows[0].out_len);
    }
  }
  std::printf("ok\n");
  return 0;
}
#endif
