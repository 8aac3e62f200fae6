// LDS geometry of a wave's exchange / power region in fft512c_kernel (kernel_fft512c.hpp) and the choice of the filterbank instance from
// the mel schedule.  Pure C++ (no HIP): also compiled by tests/ on the CPU (tests/native/fft512c_geom_capi.cpp).
#pragma once

namespace hipfeat {

// Exchange between the two FFT passes: per frame (16 lanes) a block of 8 rows x 16 complex columns.  A row is 16-byte aligned and 144 B
// long, so that a lane reads its row back with eight ds_read_b128 (two complex columns each) instead of sixteen ds_read_b64.  Banks
// (dwords mod 64): the rows of a frame start at 36 r = {0, 36, 8, 44, 16, 52, 24, 60}, those of the next frame 32 further on -- sixteen
// different multiples of 4, which is what a 16-lane group of a ds_read_b128 (8 lanes of each of two frames) needs to be conflict-free.
constexpr int kCExRowStride = 36;                       // dwords per exchange row (16 complex + 4 pad)
constexpr int kCExFrameStride = 8 * kCExRowStride;      // 288 (== 32 mod 64): 8 rows per half
constexpr int kCPRowStride = 272;                       // dwords per power row (== 16 mod 64: the 4 frames of a slot hit disjoint bank quads)
constexpr int kCRegion = 1168;                          // dwords per wave: the 4 exchange blocks (1152); the 4 power rows (1088) alias them
constexpr int kCMaxSets = 2;                            // accumulator sets (16 slots each)
constexpr int kCMaxSteps = 16;                          // MFMA steps per set
static_assert(kCExRowStride % 4 == 0 && kCExFrameStride % 4 == 0 && kCRegion % 4 == 0, "16-byte reads: rows, blocks and regions are 16-byte aligned");
static_assert(4 * kCExFrameStride <= kCRegion && 4 * kCPRowStride <= kCRegion, "four exchange blocks / four power rows per wave");
static_assert(kCExRowStride >= 32 && 7 * (kCExRowStride / 2) < 256, "a row holds 16 complex values; the ds_write2_b64 offsets have 8 bits");

// The step counts (T0 >= T1, multiples of 4) the two accumulator sets of a MODE 0 instance with the 16-byte store run: the schedule's own
// where an instance has them compiled in -- {16, 12}: the 80-filter default (and 72, 60, 56 filters); {16, 8}: 64 and 48 filters -- else
// the padded table's {kCMaxSteps, kCMaxSteps}.  The steps a short set drops multiply by zero weights.
struct Fft512cMelSteps {
  int t0, t1;
};
inline Fft512cMelSteps fft512c_mel_steps(int nsets, const int* steps) {
  if (nsets == 2 && steps[0] == 16 && (steps[1] == 12 || steps[1] == 8)) return {16, steps[1]};
  return {kCMaxSteps, kCMaxSteps};
}

}  // namespace hipfeat
