// Sinc resampler without a filter bank: any rate pair, every row of a launch with its own (LowpassUsingResampling,
// lhotse/dataset/cut_transforms/lowpass.py, appends Resample(sr -> 2c) Resample(2c -> sr) with a random cutoff c per cut).
//
// Reference: ResampleTensor = _get_sinc_resample_kernel + _apply_sinc_resample_kernel (lhotse/augmentation/resample.py:184-315).  For
// 16000 -> 9346 (8000 : 4673) the reference builds a bank of 4673 x 8022 float64 weights of which 22 per phase are not zero, and
// resample_kernel (kernel_resample.hpp) would need that bank in HBM.  Here every phase's W = 2 * width + 2 window weights
// (sinc_tables.hpp: the formula, the window, why the rest is exactly zero in float32) are evaluated on the device, in float64 rounded
// once to float32 as the reference rounds them, and reused over the hops of the row.
//
// One workgroup = one row, a tile of 256 consecutive phases, a chunk of kSincHops hops (sinc_tables.hpp has the table).  A lane owns
// one phase: it evaluates its W weights into LDS as w[tap][lane] (a lane reads back only its own column: consecutive lanes, consecutive
// banks, no barrier), then walks the hops of the chunk:
//     y[j * new + ph] = sum_d w[d] * xpad[j * orig + i0(ph) + d],   xpad = the row with `width` zeros in front and zeros behind.
// The accumulator starts at 0, d ascends, one fmaf per tap: the chain of resample_kernel over the taps of the window.  The taps it leaves
// out have weight +-0 in the reference's bank, so for identical weights the outputs compare equal to resample_kernel's, value for value
// (the sign of an exact zero may differ; a non-finite sample under a zero-weight tap of the window is the other corner).
// Consecutive lanes store consecutive outputs; they read input addresses that differ by at most ceil(orig / new), so the loads of a
// wave fall into a few cache lines and the input is not staged.
//
// The arena holds inputs and outputs; hipfeat_sinc_plan has checked that no output range meets an input range or another output.
#pragma once
#include "common.hpp"
#include "sinc_tables.hpp"

namespace hipfeat {

struct SincArgs {
  float* arena;
  const SincRow* rows;
  int32_t num_rows, pad;
};

__device__ __forceinline__ int sinc_find_row(const SincRow* __restrict__ rows, int num_rows, int wg) {
  int lo = 0, hi = num_rows - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].wg_first <= wg) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void sinc_kernel(const SincArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sinc_w[];  // [W][256]
  const int tid = threadIdx.x;
  const SincRow* __restrict__ rp = a.rows + sinc_find_row(a.rows, a.num_rows, blockIdx.x);
  const int64_t in_off = rp->in_off, out_off = rp->out_off;
  const int in_len = rp->in_len, out_len = rp->out_len, orig = rp->orig, nw = rp->nw, width = rp->width, tiles = rp->tiles, hops = rp->hops;
  const double base = rp->base;
  const int k = blockIdx.x - rp->wg_first;
  const int chunk = k / tiles, tile = k - chunk * tiles;
  const int ph = tile * kSincPhases + tid;
  if (ph >= nw || ph >= out_len) return;  // (no barrier in this kernel)
  const int W = 2 * width + 2;
  const int i0 = sinc_first_tap(ph, orig, nw, width, base);
  float* w = sinc_w + tid;
  for (int d = 0; d < W; ++d) w[d * kSincPhases] = sinc_weight(ph, i0 + d, orig, nw, width, base);
  const float* __restrict__ x = a.arena + in_off;
  float* __restrict__ y = a.arena + out_off;
  const int j1 = min((chunk + 1) * kSincHops, hops);
  for (int j = chunk * kSincHops; j < j1; ++j) {
    const int64_t o = (int64_t)j * nw + ph;
    if (o >= out_len) break;
    const int64_t s0 = (int64_t)j * orig + (i0 - width);  // the input sample under tap i0
    float acc = 0.0f;
    for (int d = 0; d < W; ++d) {
      const int64_t s = s0 + d;
      const float xv = (s >= 0 && s < in_len) ? x[s] : 0.0f;
      acc = fmaf(xv, w[d * kSincPhases], acc);
    }
    y[o] = acc;
  }
}

// The filter a rate pair gets: weights[nw][W] and first[nw] (the window's first tap, counted in taps of the padded input).
__global__ __launch_bounds__(256) void sinc_weights_kernel(float* __restrict__ weights, int32_t* __restrict__ first, int orig, int nw, int width, double base) {
  const int ph = blockIdx.x * 256 + threadIdx.x;
  if (ph >= nw) return;
  const int W = 2 * width + 2;
  const int i0 = sinc_first_tap(ph, orig, nw, width, base);
  first[ph] = i0;
  for (int d = 0; d < W; ++d) weights[(int64_t)ph * W + d] = sinc_weight(ph, i0 + d, orig, nw, width, base);
}

}  // namespace hipfeat
