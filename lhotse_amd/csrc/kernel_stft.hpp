// Kaldi-preprocessed frames (Wav2Win, lhotse/features/kaldi/layers.py:151-197) and their complex STFT (Wav2FFT, layers.py:309-324)
// of a uniform (B, S) float32 batch, handed out instead of being consumed by a feature epilogue.
//
// The front end and the FFT are those of kernel_wave.hpp: one WAVE owns one frame at a time and never synchronises with the rest of
// its workgroup (the only __syncthreads is behind the table load).  Samples come straight from global memory (frame_indices of
// layers.py:727-772 as an index map: snip_edges, or the flip-reflection at both ends), lane l holds the pairs (x[2n], x[2n+1]) for
// n = l + 64 q, the DC mean and the two log-energies (layers.py:859-870) are wave reductions, pre-emphasis takes the previous
// sample from the neighbouring lane, the window comes from LDS.
//
//   OUT == 0, frames.  The windowed frame goes to the wave's LDS buffer in natural order and from there to the (B, T, pad) row:
//     taps N .. pad - 1 are zeros.  A row starts at (b T + f) pad floats, so it is 16-byte aligned only when pad % 4 == 0: positions
//     are counted from the 16-byte boundary at or below the row's first element, a lane owns whole 16-byte groups, a group inside
//     the row is one 16-byte store and the groups the row's first and last element cut are stored element by element (the head and
//     tail of kernel_collate.hpp).  Nothing is stored outside [row, row + pad).
//   OUT == 1, spectrum.  pad = fft = 2 H: the frame is the H complex numbers z[n] = x[2n] + i x[2n+1], fft3_frame transforms them
//     (three register passes, H = N1 x 8 x 8) and the split step X[k] = E[k] + W_2H^k O[k] yields bins k and H - k from Z[k] and
//     Z[H - k].  Each bin leaves the lane's registers as one 8-byte (re, im) store into a row of fft + 2 floats (the base of the output
//     is 8-byte aligned: the host checks it); consecutive lanes store consecutive bins.  With want_energy bin 0 is (log_energy, 0).
//
// All arguments are scalars (the batch is uniform: no device table).  All element indexing is 64-bit.  No scratch, no atomics.
//
// The kernel's text is stft_body, parametrised by the source policy of kernel_wave.hpp: stft_kernel is the body on RowSource (the row
// with its reflections, as described above), kernel_stream.hpp runs it on the two-span source of the streaming layers, and
// stft_ragged_kernel is the body on RaggedRowSource: rows with a length of their own (the one device table of this file), whose padding
// rows in the (B, Tmax, width) output the same launch writes.
#pragma once
#include "common.hpp"
#include "fft_common.hpp"
#include "kernel_wave.hpp"

namespace hipfeat {

struct StftParams {
  const float* wave;    // row b at wave + b * row_stride, 4-byte aligned
  float* out;           // OUT 0: [B][T][pad]; OUT 1: [B][T][fft + 2]
  float* log_energy;    // [B][T] or NULL
  const float* window;  // [N]
  const float2* tw;     // OUT 1: W_2H^k, k < H
  int64_t row_stride, num_samples, frames_per_row, blocks_per_row;
  int32_t N, shift, pad, npad_left, frames_per_wave, flags;
  float preemph, log_energy_floor;
};

// frame_indices (layers.py:756-764) on a row of S samples: j < 0 -> -j - 1, j >= S -> 2 S - 1 - j; what the host's length check lets
// through lies inside the row, anything else reads as zero
__device__ __forceinline__ float stft_sample(const float* __restrict__ w, int64_t j, int64_t S) {
  if (j < 0) j = -j - 1;
  if (j >= S) j = 2 * S - 1 - j;
  return (j >= 0 && j < S) ? w[j] : 0.0f;
}

// The frame mean is summed in float64 and rounded once: the frames ARE the output here, and after DC removal alone (rectangular window,
// no pre-emphasis) the mean's error is all the error there is -- a float32 sum of 1200 samples is off by an ulp or two of the mean, which
// measured at up to 2.07 x the error of the reference's own frames (torch.mean sums pairwise).  wave_sum with 64-bit DPP moves.
template <int CTRL>
__device__ __forceinline__ double dpp_mov_f64(double v) {
  const int2 b = __builtin_bit_cast(int2, v);
  return __builtin_bit_cast(double, int2{__builtin_amdgcn_update_dpp(0, b.x, CTRL, 0xF, 0xF, true), __builtin_amdgcn_update_dpp(0, b.y, CTRL, 0xF, 0xF, true)});
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const int2 b = __builtin_bit_cast(int2, v);
  return __builtin_bit_cast(double, int2{__builtin_amdgcn_readlane(b.x, l), __builtin_amdgcn_readlane(b.y, l)});
}
__device__ __forceinline__ double wave_sum_f64(double v) {  // every lane gets the total, in a fixed order
  v += dpp_mov_f64<DPP_QUAD(1, 0, 3, 2)>(v);
  v += dpp_mov_f64<DPP_QUAD(2, 3, 0, 1)>(v);
  v += dpp_mov_f64<DPP_ROW_HALF_MIRROR>(v);
  v += dpp_mov_f64<DPP_ROW_MIRROR>(v);
  return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}

constexpr int stft_buf_floats(int N1, int OUT) { return OUT == 1 ? 144 * N1 + 8 : 128 * N1; }  // per wave
inline size_t stft_lds_bytes(int N1, int OUT, int N) {
  return sizeof(float) * (size_t)(4 * stft_buf_floats(N1, OUT) + ((N + 3) & ~3) + (OUT == 1 ? 4 * 64 * N1 : 0));
}

// Source policy of stft_body (kernel_wave.hpp says what a policy offers): RowSource is what stft_kernel has always done, one row of
// num_samples samples with the flip-reflection at both ends.
struct RowSource {
  using Args = NoSourceArgs;
  static constexpr bool kPads = false;
  const float* __restrict__ w;
  int64_t row, fb, T, S;
  __device__ __forceinline__ RowSource(const StftParams& p, const NoSourceArgs&, int64_t blk) {
    row = blk / p.blocks_per_row, fb = blk - row * p.blocks_per_row;
    T = p.frames_per_row, S = p.num_samples;
    w = p.wave + row * p.row_stride;
  }
  __device__ __forceinline__ bool inside(int64_t j0, int span) const { return j0 >= 0 && j0 + span <= S; }
  __device__ __forceinline__ const float* base(int64_t j0) const { return w + j0; }
  __device__ __forceinline__ v2 slow_pair(int64_t j, bool second) const {
    v2 v = {stft_sample(w, j, S), 0.f};
    if (second) v.y = stft_sample(w, j + 1, S);
    return v;
  }
};

// RaggedRowSource: the rows of a zero-padded (B, Smax) batch, each with a length of its own.  The grid is that of RowSource with
// frames_per_row = Tmax = max_b T_b; a workgroup takes S_b and T_b of its row from the length table (rows x {S_b, T_b}, which the host
// has checked against Smax before it staged it) and reflects at S_b, so row b is framed exactly as x[b, :S_b] alone and nothing from
// S_b on is read.  kPads: the frames T_b <= f < Tmax of the (B, Tmax, width) output are the padding rows, which the same launch writes.
struct RaggedArgs {
  const int64_t* table;  // [rows][2]: S_b, T_b
  float padding;         // what the padding rows hold
};

struct RaggedRowSource {
  using Args = RaggedArgs;
  static constexpr bool kPads = true;
  const float* __restrict__ w;
  int64_t row, fb, T, S;
  float padding;
  template <class Params>
  __device__ __forceinline__ RaggedRowSource(const Params& p, const RaggedArgs& a, int64_t blk) {
    row = blk / p.blocks_per_row, fb = blk - row * p.blocks_per_row;
    S = a.table[2 * row], T = a.table[2 * row + 1];
    padding = a.padding;
    w = p.wave + row * p.row_stride;
  }
  __device__ __forceinline__ bool inside(int64_t j0, int span) const { return j0 >= 0 && j0 + span <= S; }
  __device__ __forceinline__ const float* base(int64_t j0) const { return w + j0; }
  __device__ __forceinline__ v2 slow_pair(int64_t j, bool second) const {
    v2 v = {stft_sample(w, j, S), 0.f};
    if (second) v.y = stft_sample(w, j + 1, S);
    return v;
  }
};

// One padding row of the output, by one wave, with the stores of a computed row: OUT 0 the 16-byte groups counted from the boundary at or
// below the row's start with the scalar head and tail, OUT 1 one 8-byte (padding, 0) store per bin; and the row's padded log-energy.
template <int OUT>
__device__ __forceinline__ void stft_pad_row(const StftParams& p, float padding, int64_t orow_index, int lane) {
  if (p.log_energy != nullptr && lane == 0) p.log_energy[orow_index] = padding;
  if constexpr (OUT == 0) {
    float* __restrict__ orow = p.out + orow_index * (int64_t)p.pad;
    const int head = (int)((reinterpret_cast<uintptr_t>(orow) / sizeof(float)) & 3);
    const int64_t row_end = (int64_t)head + p.pad;
    for (int64_t pp = 4 * lane; pp < row_end; pp += 256) {
      if (pp >= head && pp + 4 <= row_end) {
        *reinterpret_cast<f32x4*>(orow + (pp - head)) = f32x4{padding, padding, padding, padding};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (pp + j >= head && pp + j < row_end) orow[pp + j - head] = padding;
      }
    }
  } else {
    float* __restrict__ orow = p.out + orow_index * (int64_t)(p.pad + 2);
    for (int k = lane; k <= p.pad / 2; k += 64) *reinterpret_cast<v2*>(orow + 2 * k) = v2{padding, 0.f};
  }
}

template <int N1, int OUT, class Src>
__device__ __forceinline__ void stft_body(const StftParams& p, const typename Src::Args& sa) {
  constexpr int H = 64 * N1, BUF = stft_buf_floats(N1, OUT);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  HF_POISON_LDS(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* buf = smem + wv * BUF;                                          // wave-private: the frame (OUT 0) or the padded FFT buffer
  float* winl = smem + 4 * BUF;                                          // [N] window, shared by the four waves
  float2* tw = reinterpret_cast<float2*>(winl + ((p.N + 3) & ~3));       // [H] W_2H^k for the split step
  v2* twh = reinterpret_cast<v2*>(tw + H);                               // [H] W_H^m for the FFT passes
  const int N = p.N;
  for (int i = tid; i < N; i += 256) winl[i] = p.window[i];
  if constexpr (OUT == 1) {
    for (int i = tid; i < H; i += 256) {
      tw[i] = p.tw[i];
      twh[i] = twiddle_h(p.tw, i, H);
    }
  }
  __syncthreads();

  const Src src(p, sa, (int64_t)blockIdx.x);
  const int64_t row = src.row, fb = src.fb, T = src.T;
  int64_t Tout = T;  // frames of an output row: the padding rows of a ragged batch included
  if constexpr (Src::kPads) Tout = p.frames_per_row;
  const bool want_e = (p.flags & F_USE_ENERGY) != 0;
  const int64_t fbase = fb * 4 * p.frames_per_wave;
#pragma unroll 1
  for (int i = 0; i < p.frames_per_wave; ++i) {
    const int64_t f = fbase + 4 * i + wv;
    if (f >= Tout) break;
    if constexpr (Src::kPads) {
      if (f >= T) {  // wave-uniform: a wave owns the whole frame
        stft_pad_row<OUT>(p, sa.padding, row * Tout + f, lane);
        continue;
      }
    }
    const int64_t j0 = f * p.shift - p.npad_left;

    // ---- samples, DC mean, raw log-energy (layers.py:155-162): lane l holds (x[2n], x[2n+1]) for n = l + 64 q ----------------------
    // Frames that lie inside the row (almost all) use one 8-byte load per pair; edge frames go sample by sample.
    v2 xp[N1];
    double s = 0.0;
    const bool inside = src.inside(j0, (N + 1) & ~1);
    const float* __restrict__ w = src.base(j0);
#pragma unroll
    for (int q = 0; q < N1; ++q) {
      const int m0 = 2 * (lane + 64 * q);
      v2 v = {0.f, 0.f};
      if (m0 < N) {
        if (inside) {
          __builtin_memcpy(&v, w + m0, sizeof(v2));  // 4-byte aligned 8-byte load
          if (m0 + 1 >= N) v.y = 0.f;
        } else {
          v = src.slow_pair(j0 + m0, m0 + 1 < N);
        }
      }
      xp[q] = v;
      s += (double)v.x + (double)v.y;
    }
    float mean = 0.f;
    if (p.flags & F_REMOVE_DC) mean = (float)(wave_sum_f64(s) / (double)N);
    float log_e = 0.f;
    if (want_e && (p.flags & F_RAW_ENERGY)) {
      float e = 0.f;
#pragma unroll
      for (int q = 0; q < N1; ++q) {
        const int m0 = 2 * (lane + 64 * q);
        const float d0 = m0 < N ? xp[q].x - mean : 0.f, d1 = m0 + 1 < N ? xp[q].y - mean : 0.f;
        e = fmaf(d0, d0, fmaf(d1, d1, e));
      }
      log_e = fmaxf(logf(wave_sum(e) + 1e-15f), p.log_energy_floor);
    }
    // y[m] = (d[m] - c d[max(m-1, 0)]) w[m] with d = x - mean, zeros from tap N on (layers.py:165-181); d[2n-1] is the previous
    // lane's second sample: lane 63 offers the one of its previous register, so a single wrap-around ds_bpermute serves both
    v2 y[N1];
    {
      float e = 0.f;
#pragma unroll
      for (int q = 0; q < N1; ++q) {
        const int m0 = 2 * (lane + 64 * q);
        const float d0 = xp[q].x - mean, d1 = xp[q].y - mean;
        const float offer = (q > 0 && lane == 63) ? xp[q > 0 ? q - 1 : 0].y - mean : d1;
        float dm = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(4 * ((lane - 1) & 63), __builtin_bit_cast(int, offer)));
        if (q == 0 && lane == 0) dm = d0;  // d[max(m - 1, 0)] at the start of the frame
        v2 v = {0.f, 0.f};
        if (m0 < N) {
          const v2 wn = *reinterpret_cast<const v2*>(winl + m0);
          v.x = (d0 - p.preemph * dm) * wn.x;
          if (m0 + 1 < N) v.y = (d1 - p.preemph * d0) * wn.y;
        }
        y[q] = v;
        e = fmaf(v.x, v.x, fmaf(v.y, v.y, e));
      }
      if (want_e && !(p.flags & F_RAW_ENERGY)) log_e = fmaxf(logf(wave_sum(e) + 1e-15f), p.log_energy_floor);  // layers.py:183-185
    }
    const int64_t orow_index = row * Tout + f;
    if (p.log_energy != nullptr && lane == 0) p.log_energy[orow_index] = log_e;
    wave_lds_sync();  // the previous frame's readers of this wave's buffer are done

    if constexpr (OUT == 0) {
      // ---- frames: through LDS into natural order, then 16-byte groups counted from the boundary at or below the row's start ------
#pragma unroll
      for (int q = 0; q < N1; ++q) *reinterpret_cast<v2*>(buf + 2 * (lane + 64 * q)) = y[q];
      wave_lds_sync();
      float* __restrict__ orow = p.out + orow_index * (int64_t)p.pad;
      const int head = (int)((reinterpret_cast<uintptr_t>(orow) / sizeof(float)) & 3);
      const int64_t row_end = (int64_t)head + p.pad;  // the row is [head, row_end)
      for (int64_t pp = 4 * lane; pp < row_end; pp += 256) {
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t m = pp + j - head;
          e[j] = (m >= 0 && m < N) ? buf[m] : 0.f;
        }
        if (pp >= head && pp + 4 <= row_end) {
          *reinterpret_cast<f32x4*>(orow + (pp - head)) = f32x4{e[0], e[1], e[2], e[3]};
        } else {  // the row's first or last element cuts the group
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (pp + j >= head && pp + j < row_end) orow[pp + j - head] = e[j];
        }
      }
    } else {
      // ---- complex FFT of size H, split step (kernel_wave.hpp): with a = Z[k], b = Z[H-k], E = (a + conj b)/2, O = -i (a - conj b)/2,
      // T = W_2H^k O:  X[k] = E + T and X[H-k] = conj(E - T).  Lane l takes k = l + 64 q <= H/2; k = 0 yields X[0] and X[H]. -----------
      v2* zf = reinterpret_cast<v2*>(buf);
      fft3_frame<N1>(zf, twh, lane, y);
      float* __restrict__ orow = p.out + orow_index * (int64_t)(2 * H + 2);
#pragma unroll
      for (int q = 0; q <= N1 / 2; ++q) {
        const int k = lane + 64 * q;
        if (k <= H / 2) {
          const v2 a = zf[k], b = zf[(H - k) & (H - 1)];
          const float ex = 0.5f * (a.x + b.x), ey = 0.5f * (a.y - b.y);
          const float ox = 0.5f * (a.y + b.y), oy = -0.5f * (a.x - b.x);
          const float2 wk = tw[k];
          const float tx = wk.x * ox - wk.y * oy, ty = wk.x * oy + wk.y * ox;
          v2 lo = {ex + tx, ey + ty};
          const v2 hi = {ex - tx, ty - ey};
          if (want_e && k == 0) lo = v2{log_e, 0.f};  // X[:, :, 0] = log_e (layers.py:317-318)
          *reinterpret_cast<v2*>(orow + 2 * k) = lo;
          if (k < H / 2) *reinterpret_cast<v2*>(orow + 2 * (H - k)) = hi;
        }
      }
    }
    wave_lds_sync();  // the buffer is reused by the next frame
  }
}

template <int N1, int OUT>
__global__ __launch_bounds__(256, (N1 == 16 ? 2 : HIPFEAT_WAVE_OCC)) void stft_kernel(const StftParams p) {
  stft_body<N1, OUT, RowSource>(p, NoSourceArgs{});
}

template <int N1, int OUT>
__global__ __launch_bounds__(256, (N1 == 16 ? 2 : HIPFEAT_WAVE_OCC)) void stft_ragged_kernel(const StftParams p, const RaggedArgs a) {
  stft_body<N1, OUT, RaggedRowSource>(p, a);
}

}  // namespace hipfeat
