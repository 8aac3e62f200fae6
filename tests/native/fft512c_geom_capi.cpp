// Test shim (CPU only): the LDS geometry constants of fft512c_kernel's exchange and the choice of its filterbank instance
// (lhotse_amd/csrc/fft512c_geom.hpp), so that tests/test_fft512c_exchange_layout.py models the addressing from the very constants the
// kernel is compiled with and asks the very function plan creation asks.
#include "../../lhotse_amd/csrc/fft512c_geom.hpp"
#include "../../lhotse_amd/csrc/mel4_schedule.hpp"

using namespace hipfeat;

// out: row stride, frame stride, power-row stride, region (dwords), max sets, max steps
extern "C" void f5g_constants(int* out) {
  const int v[6] = {kCExRowStride, kCExFrameStride, kCPRowStride, kCRegion, kCMaxSets, kCMaxSteps};
  for (int i = 0; i < 6; ++i) out[i] = v[i];
}

// The schedule of a filterbank ([K][M] row-major) as plan creation builds it for the two-set mode, and the steps of the instance chosen
// for it.  Returns the number of sets (0: the bank does not fit the two-set schedule).
extern "C" int f5g_instance(const float* h_mel, int M, int K, int* sched_steps, int* inst_steps) {
  Mel4Schedule s;
  if (!build_mel4_schedule(h_mel, M, K, kCPRowStride, kCMaxSets, kCMaxSteps, s)) return 0;
  for (int i = 0; i < 4; ++i) sched_steps[i] = s.steps[i];
  const Fft512cMelSteps t = fft512c_mel_steps(s.nsets, s.steps);
  inst_steps[0] = t.t0, inst_steps[1] = t.t1;
  return s.nsets;
}

// fft512c_mel_steps on its own (schedules no default bank has)
extern "C" void f5g_mel_steps(int nsets, const int* steps, int* inst_steps) {
  const Fft512cMelSteps t = fft512c_mel_steps(nsets, steps);
  inst_steps[0] = t.t0, inst_steps[1] = t.t1;
}
