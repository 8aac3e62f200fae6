// Streaming instances of the two wave-per-frame kernels: online_inference of the six layers (layers.py:199-224, 326-333, 775-856).
//
// One call frames the VIRTUAL waveform V = [A | chunk] of L = R + S samples per row, where A is the caller's context (R samples) or, at
// the start of a stream without snip_edges, the flipped head of the chunk (R = min((N - shift) / 2, S) samples, A(j) = chunk[R - 1 - j]).
// Frame f is V[f shift : f shift + N] for f < T = 1 + (L - N) / shift (T = 0 when L < N): every index a frame touches lies inside V, so
// the source has no zero fill and no reflection test, and a stream has no right edge.  What the frames do not consume, V[T shift : L],
// is the remainder the caller hands back as the next context.
//
// The kernels are wave_body (kernel_wave.hpp: the four feature kinds) and stft_body (kernel_stft.hpp: frames, spectrum) with the
// StreamSource below as their source policy: the same per-frame arithmetic, in the same order, as the instances `forward` launches,
// by one wave from the frame's own samples alone -- which is what makes the output independent of how the stream was cut into chunks.
// A frame that lies wholly inside the context or wholly inside the chunk takes the 8-byte loads at 4-byte alignment; a frame that
// straddles the seam, or touches a flipped head, goes sample by sample.  The choice is per frame, hence wave-uniform.
//
// After its frames the first workgroup of each row copies the remainder (fewer than N <= 2048 floats when T >= 1; all of V, fewer than
// N as well, when T = 0) to row b of the remainder output with plain 4-byte loads and stores.  The grid is B x max(blocks_per_row, 1), so
// a call without frames still writes its remainder.  No scratch, no atomics, no memset; all element indexing is 64-bit.
#pragma once
#include "common.hpp"
#include "kernel_stft.hpp"
#include "kernel_wave.hpp"

namespace hipfeat {

struct StreamArgs {
  const float* ctx;    // row b at ctx + b * ctx_stride, R samples (not read when flipped)
  const float* chunk;  // row b at chunk + b * chunk_stride, S samples
  float* remainder;    // [B][L - T shift], contiguous
  int64_t ctx_stride, chunk_stride, R, S, T, blocks_per_row;
  int32_t flipped;     // A(j) = chunk[R - 1 - j]
  int32_t shift;
};

struct StreamSource {
  using Args = StreamArgs;
  static constexpr bool kPads = false;
  const float* __restrict__ ctx;
  const float* __restrict__ chunk;
  int64_t R, S, row, fb, T, out_row;
  bool flipped;
  template <class Params>
  __device__ __forceinline__ StreamSource(const Params&, const StreamArgs& a, int64_t blk) {
    row = blk / a.blocks_per_row;
    fb = blk - row * a.blocks_per_row;
    T = a.T;
    out_row = row * a.T;
    R = a.R, S = a.S;
    flipped = a.flipped != 0;
    chunk = a.chunk + row * a.chunk_stride;
    ctx = flipped ? chunk : a.ctx + row * a.ctx_stride;
  }
  // V(j), 0 <= j < R + S
  __device__ __forceinline__ float at(int64_t j) const { return j < R ? (flipped ? chunk[R - 1 - j] : ctx[j]) : chunk[j - R]; }
  // [j0, j0 + span) lies inside one span that is stored forwards (span = N rounded up to even: the 8-byte load of an odd frame's last pair)
  __device__ __forceinline__ bool inside(int64_t j0, int span) const { return j0 >= R ? j0 - R + span <= S : (!flipped && j0 + span <= R); }
  __device__ __forceinline__ const float* base(int64_t j0) const { return j0 >= R ? chunk + (j0 - R) : ctx + j0; }
  __device__ __forceinline__ v2 slow_pair(int64_t j, bool second) const {
    v2 v = {at(j), 0.f};
    if (second) v.y = at(j + 1);
    return v;
  }
};

// V[T shift : L] -> remainder row, by the first workgroup of the row
__device__ __forceinline__ void stream_copy_remainder(const StreamArgs& a) {
  const StreamSource src(a, a, (int64_t)blockIdx.x);
  if (src.fb != 0) return;
  const int64_t from = a.T * a.shift, len = a.R + a.S - from;
  float* __restrict__ dst = a.remainder + src.row * len;
  for (int64_t i = threadIdx.x; i < len; i += 256) dst[i] = src.at(from + i);
}

template <int N1>
__global__ __launch_bounds__(256, (N1 == 16 ? 2 : HIPFEAT_WAVE_OCC)) void wave_stream_kernel(const WaveParams p, const StreamArgs a) {
  wave_body<N1, StreamSource>(p, a);
  stream_copy_remainder(a);
}

template <int N1, int OUT>
__global__ __launch_bounds__(256, (N1 == 16 ? 2 : HIPFEAT_WAVE_OCC)) void stft_stream_kernel(const StftParams p, const StreamArgs a) {
  stft_body<N1, OUT, StreamSource>(p, a);
  stream_copy_remainder(a);
}

}  // namespace hipfeat
