// Test shim (CPU only): C entry points around lhotse_amd/csrc/grad_tables.hpp -- the banded filterbank blob and the piece arithmetic of the
// gradient workspace -- so that tests/test_grad_tables.py can check them without a device.
#include "../../lhotse_amd/csrc/grad_tables.hpp"

#include <cstring>

// -> the blob's length in 4-byte words; h_blob (may be NULL) receives at most `capacity` of them, h_offsets[4] = {fwd, bwd, dct, lifter}
extern "C" long long gt_build(int K, int M, int C, const float* mel, const float* dct, const float* lifter, float* h_blob, long long capacity,
                              int32_t* h_offsets) {
  const hipfeat::GradTables t = hipfeat::build_grad_tables(K, M, C, mel, dct, lifter);
  h_offsets[0] = t.off_fwd, h_offsets[1] = t.off_bwd, h_offsets[2] = t.off_dct, h_offsets[3] = t.off_lifter;
  if (h_blob) std::memcpy(h_blob, t.blob.data(), sizeof(float) * (size_t)std::min<long long>(capacity, (long long)t.blob.size()));
  return (long long)t.blob.size();
}

// -> 1 when the counts fit int64; h_out[4] = {Nr, floats of one row, rows per piece, floats of the workspace}
extern "C" int gt_pieces(long long batch, long long T, int N, long long budget_bytes, int64_t* h_out) {
  hipfeat::GradPieces p;
  if (!hipfeat::grad_pieces(batch, T, N, budget_bytes, &p)) return 0;
  h_out[0] = p.Nr, h_out[1] = p.row_floats, h_out[2] = p.rows_per_piece, h_out[3] = p.floats;
  return 1;
}

extern "C" long long gt_lds_floats(int n1, int N) { return (long long)hipfeat::grad_lds_floats(n1, N); }
extern "C" int gt_blob_fits(int n1, int N, long long blob_floats) { return hipfeat::grad_blob_fits_lds(n1, N, (size_t)blob_floats) ? 1 : 0; }
