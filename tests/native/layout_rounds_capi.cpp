// Test shim (CPU only): C entry points around lhotse_amd/csrc/layout_rounds.hpp so that tests/test_layout_rounds.py can compare the
// rounds build_descs chooses for a layout with the Python restatement the GPU tests use (tests/_layout_rounds.py).
#include "../../lhotse_amd/csrc/layout_rounds.hpp"
extern "C" int layout_rounds_per_cut(const int64_t* num_frames, int64_t batch, int fpb_unit, int rounds_max, int blocks_per_cu) {
  return hipfeat::layout_rounds_per_cut(num_frames, batch, fpb_unit, rounds_max, blocks_per_cu);
}
extern "C" int layout_rounds_quads(int64_t quads, int fpb_unit, int rounds_max, int blocks_per_cu) {
  return hipfeat::layout_rounds_quads(quads, fpb_unit, rounds_max, blocks_per_cu);
}
