// Rounds per workgroup of the wave-autonomous kernels, chosen per LAYOUT (build_descs in hipfeat.hip).
// Pure C++ (no HIP): also compiled by tests/native/layout_rounds_capi.cpp and checked on the CPU (tests/test_layout_rounds.py) against
// the Python restatement tests/_layout_rounds.py, from which the GPU tests work out how many frames a workgroup of their layout holds.
//
// Frames per workgroup = fpb_unit (frames of one round of all waves) x rounds.  A workgroup pays a fixed start-up (the constant image,
// its first, un-overlapped span: ~0.64 of a round, from the 8-vs-16-rounds A/B of round 3), its last round-set is only partly filled (a
// cut's frames are not shared between workgroups), and the launch runs in ceil(workgroups / resident slots) waves of workgroups: the
// rounds that minimise  waves x (start-up + rounds).  10 000 x 1000 frames end up at the maximum (16: two workgroups per cut, start-up
// amortised); LibriSpeech-like lengths (mean 1230 frames) at 8 (16 would leave the third workgroup of a cut 60 % empty); a 600 s
// mini-batch (60 000 frames) at 4 rounds in ONE wave of ~470 workgroups instead of two waves of 2-round workgroups.
#pragma once
#include <algorithm>
#include <cstdint>

namespace hipfeat {

constexpr double kRoundsStartup = 0.64;   // start-up of a workgroup, in rounds
constexpr int64_t kRoundsSampledCuts = 512;  // the per-cut rule looks at (about) this many evenly spaced cuts of the batch

// resident workgroup slots of the device the rule is tuned for (256 CUs)
inline int64_t layout_slots(int blocks_per_cu) { return 256LL * std::max(blocks_per_cu, 1); }

// cost of a launch of nb workgroups of r rounds each
inline double layout_rounds_cost(int64_t nb, int64_t slots, int r) {
  const double waves = nb >= 8 * slots ? (double)nb / (double)slots : (double)((nb + slots - 1) / slots);  // (many waves: the last one hardly matters)
  return waves * (kRoundsStartup + r);
}

// the r in [min(2, rounds_max), rounds_max] of least cost; ties go to the larger workgroup
template <typename Workgroups>
inline int layout_rounds_argmin(int rounds_max, int64_t slots, Workgroups&& workgroups) {
  int rounds = rounds_max;
  double best = -1.0;
  for (int r = std::min(2, rounds_max); r <= rounds_max; ++r) {
    const double cost = layout_rounds_cost(workgroups(r), slots, r);
    if (best < 0.0 || cost <= best * (1.0 + 1e-9)) {
      best = cost;
      rounds = r;
    }
  }
  return rounds;
}

// workgroups of a layout by cuts at `rounds` rounds; step > 1: estimated from every step-th cut
inline int64_t layout_workgroups_per_cut(const int64_t* num_frames, int64_t batch, int fpb_unit, int rounds, int64_t step) {
  const int64_t per = (int64_t)fpb_unit * rounds;
  int64_t nb = 0, n = 0;
  for (int64_t b = 0; b < batch; b += step, ++n) nb += (num_frames[b] + per - 1) / per;
  return step == 1 ? nb : (nb * batch + n / 2) / std::max<int64_t>(n, 1);
}

// Layout by cuts (a cut's frames are not shared between workgroups).  Evaluated on at most ~512 evenly spaced cuts of the batch (a
// transient layout is built per call).
inline int layout_rounds_per_cut(const int64_t* num_frames, int64_t batch, int fpb_unit, int rounds_max, int blocks_per_cu) {
  const int64_t stride = std::max<int64_t>(1, batch / kRoundsSampledCuts);
  return layout_rounds_argmin(rounds_max, layout_slots(blocks_per_cu),
                              [&](int r) { return layout_workgroups_per_cut(num_frames, batch, fpb_unit, r, stride); });
}

// Layout by frame quads (kernel_fft512c.hpp, FLAT): a wave takes one quad per round, workgroups run across cut boundaries.
inline int layout_rounds_quads(int64_t quads, int fpb_unit, int rounds_max, int blocks_per_cu) {
  const int64_t waves_per_wg = fpb_unit / 4;
  return layout_rounds_argmin(rounds_max, layout_slots(blocks_per_cu),
                              [&](int r) { return (quads + waves_per_wg * r - 1) / (waves_per_wg * r); });
}

}  // namespace hipfeat
