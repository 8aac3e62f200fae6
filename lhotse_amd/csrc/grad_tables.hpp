// Host-side tables of the gradient kernels (kernel_grad.hpp): the mel filterbank as BANDS in both directions, the transposed DCT, and
// the piece arithmetic of the workspace.  Pure C++ (no HIP): also compiled by tests/native/grad_tables_capi.cpp and checked on the CPU
// (tests/test_grad_tables.py).
//
// The backward of a filterbank layer needs the mel matrix fb[K][M] twice per frame: forwards, mel_m = sum_k fb[k][m] P_k (the energies are
// recomputed, not saved), and transposed, Pbar_k = sum_m fb[k][m] g_m.  A Kaldi filter is a triangle over a few bins and a bin lies under
// at most two triangles, so both products run over bands:
//
//   blob, in 4-byte words
//     [off_fwd + 4 m ...]  int32 {lo, len, off, 0}   filter m has weights on bins [lo, lo + len): blob[off + t] = fb[lo + t][m]
//     [off_bwd + 4 k ...]  int32 {lo, len, off, 0}   bin k lies under the filters [lo, lo + len):  blob[off + t] = fb[k][lo + t]
//     [off_dct ...]        float [C][M]              dct_t[c][m] = dct[m][c]: lanes that own consecutive filters read consecutive floats
//     [off_lifter ...]     float [C]                 ones when no lifter is applied
//
// A band runs from the first to the last non-zero weight of its filter (bin) and holds the zeros in between, so ANY matrix is
// represented exactly -- a dense one just gets bands of full length, and a blob that no longer fits next to the kernel's buffers in
// LDS (grad_blob_fits_lds) is read from global memory instead.
//
// Workspace: one row of Nr = (N + 3) & ~3 floats per frame, T rows per waveform row, rows_per_piece waveform rows per piece.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace hipfeat {

struct GradTables {
  std::vector<float> blob;  // int32 descriptors are stored by bit pattern
  int32_t off_fwd = 0, off_bwd = 0, off_dct = 0, off_lifter = 0;
};

inline float grad_word(int32_t v) {
  float f;
  std::memcpy(&f, &v, sizeof(f));
  return f;
}

// mel: [K][M] (may be NULL when M == 0), dct: [M][C] (NULL when C == 0), lifter: [C] or NULL
inline GradTables build_grad_tables(int K, int M, int C, const float* mel, const float* dct, const float* lifter) {
  GradTables t;
  if (M <= 0) return t;
  std::vector<float>& b = t.blob;
  t.off_fwd = 0;
  t.off_bwd = 4 * M;
  b.assign((size_t)4 * M + (size_t)4 * K, 0.0f);
  for (int m = 0; m < M; ++m) {
    int lo = K, hi = -1;
    for (int k = 0; k < K; ++k)
      if (mel[(size_t)k * M + m] != 0.0f) lo = std::min(lo, k), hi = std::max(hi, k);
    const int len = hi < lo ? 0 : hi - lo + 1;
    const int32_t d[4] = {len ? lo : 0, len, (int32_t)b.size(), 0};
    for (int i = 0; i < 4; ++i) b[(size_t)t.off_fwd + 4 * m + i] = grad_word(d[i]);
    for (int i = 0; i < len; ++i) b.push_back(mel[(size_t)(lo + i) * M + m]);
  }
  for (int k = 0; k < K; ++k) {
    int lo = M, hi = -1;
    for (int m = 0; m < M; ++m)
      if (mel[(size_t)k * M + m] != 0.0f) lo = std::min(lo, m), hi = std::max(hi, m);
    const int len = hi < lo ? 0 : hi - lo + 1;
    const int32_t d[4] = {len ? lo : 0, len, (int32_t)b.size(), 0};
    for (int i = 0; i < 4; ++i) b[(size_t)t.off_bwd + 4 * k + i] = grad_word(d[i]);
    for (int i = 0; i < len; ++i) b.push_back(mel[(size_t)k * M + lo + i]);
  }
  t.off_dct = (int32_t)b.size();
  for (int c = 0; c < C; ++c)
    for (int m = 0; m < M; ++m) b.push_back(dct[(size_t)m * C + c]);
  t.off_lifter = (int32_t)b.size();
  for (int c = 0; c < C; ++c) b.push_back(lifter ? lifter[c] : 1.0f);
  while (b.size() % 4) b.push_back(0.0f);
  return t;
}

// LDS floats of grad_frames_kernel without the blob: four wave buffers (72 n1 + 4 float64 complex each), the window, W_2H^k and W_H^m in
// float32 and W_2H^k in float64 (kernel_grad.hpp)
inline size_t grad_lds_floats(int n1, int N) { return (size_t)4 * (288 * n1 + 16) + (size_t)((N + 3) & ~3) + (size_t)8 * 64 * n1; }
constexpr size_t kGradLdsBlobLimit = 96 * 1024;  // bytes of LDS a workgroup may take with the blob inside: two workgroups per CU stay resident
inline bool grad_blob_fits_lds(int n1, int N, size_t blob_floats) { return 4 * (grad_lds_floats(n1, N) + blob_floats) <= kGradLdsBlobLimit; }

// Piece arithmetic of the workspace: rows_per_piece = max(1, budget / (T Nr 4)), at most `batch`; a single row larger than the budget
// gets a workspace of its own size.  floats = rows_per_piece * T * Nr.  Returns false when the counts overflow int64.
struct GradPieces {
  int64_t Nr = 0, row_floats = 0, rows_per_piece = 0, floats = 0;
};
inline bool grad_pieces(int64_t batch, int64_t T, int32_t N, int64_t budget_bytes, GradPieces* out) {
  GradPieces p;
  p.Nr = ((int64_t)N + 3) & ~(int64_t)3;
  if (T < 0 || batch < 0 || T > INT64_MAX / 4 / p.Nr) return false;
  p.row_floats = T * p.Nr;
  if (batch == 0 || T == 0) {
    *out = p;
    return true;
  }
  p.rows_per_piece = std::max<int64_t>(1, (budget_bytes > 0 ? budget_bytes : 0) / (p.row_floats * 4));
  p.rows_per_piece = std::min(p.rows_per_piece, batch);
  if (p.rows_per_piece > INT64_MAX / 4 / p.row_floats) return false;
  p.floats = p.rows_per_piece * p.row_floats;
  *out = p;
  return true;
}

}  // namespace hipfeat
