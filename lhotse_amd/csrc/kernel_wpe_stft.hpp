// The two transforms around the WPE kernel for batches with per-row lengths ("Ragged WPE"): a centred STFT that reflects at
// each row's own two ends, and the inverse STFT with overlap-add and window-envelope division.  gfx950 only.
//
// Both run a real transform of N points as a complex one of M = N / 2 points on packed data, z[m] = x[2 m] + i x[2 m + 1], in float64:
//   forward:  Z = FFT_M(z);  E[k] = (Z[k] + conj(Z[M - k])) / 2,  O[k] = (Z[k] - conj(Z[M - k])) / 2i,  X[k] = E[k] + W^k O[k],  k = 0 ... M
//   inverse:  E[k] = (X[k] + conj(X[M - k])) / 2,  O[k] = (X[k] - conj(X[M - k])) / 2 * conj(W^k),  Z = E + i O,  z = conj(FFT_M(conj(Z))) / M
// with W = exp(-2 pi i / N) and Z[M] = Z[0]; the inverse drops the imaginary parts of X[0] and X[M], as irfft does.  FFT_M is one
// radix-2 decimation-in-time transform in place in LDS: the packing pass stores to bit-reversed places, and log2(M) butterfly passes
// follow.  A wave owns a frame from its first load to its last store, so the passes are ordered by the wave's own LDS queue and no
// workgroup barrier stands inside a transform.  The twiddles W^k, k < M, are made once per workgroup by sincospi in float64.
//
// Arithmetic: sample times window is exact in float64 (24 + 24 bits), every later step is float64, and the result is rounded once to
// float32.  The window is read from memory as float32: the device sees the bits torch.blackman_window gave the reference.
//
// Order of summation (ISTFT): a thread owns its output samples and adds the frames that cover one in ascending frame order, starting from
// zero; the envelope likewise.  No atomics, no workspace, no memset: a row's bits depend on nothing but its own frames.
#pragma once
#include "common.hpp"

namespace hipfeat {

constexpr int kWpeStftThreads = 256;
constexpr int kWpeStftWaves = kWpeStftThreads / 64;
constexpr int kWpeStftTileFrames = 32;  // frames per workgroup of the forward transform: eight per wave behind one table set-up
constexpr int kWpeIstftTileHops = 8;    // R: output hops per workgroup of the inverse; it transforms R + N / hop - 1 frames for them

struct WpeStftParams {
  const float* audio;      // (batch, D, num_samples) through a_row / a_chan, unit sample stride
  const int32_t* lengths;  // per example
  const float* window;     // N float32
  float2* out;             // (batch * D, M + 1, frames_max) through the three element strides
  int32_t* frames_out;     // per example: 1 + length / hop (may be null)
  int64_t a_row, a_chan, o_row, o_bin, o_frame, num_samples;
  int32_t D, N, log2n, hop, frames_max, tiles;
  int32_t off_win, off_work, lds_bytes;  // LDS map (bytes); the twiddles at 0
};

struct WpeIstftParams {
  const float2* in;       // (batch * D, M + 1, frames_max) through the three element strides
  const int32_t* frames;  // per example
  const float* window;
  float* out;  // (batch, D, out_samples) through o_row / o_chan
  int64_t i_row, i_bin, i_frame, o_row, o_chan, out_samples;
  int32_t D, N, log2n, hop, frames_max, tiles;
  int32_t off_win, off_work, off_acc, lds_bytes;
};

// twiddles, window, one transform buffer per wave (, the accumulator of `acc_doubles` float64)
inline void wpe_stft_lds_map(int32_t N, int64_t acc_doubles, int32_t& off_win, int32_t& off_work, int32_t& off_acc, int32_t& lds_bytes) {
  const int64_t M = N / 2;
  off_win = (int32_t)(M * 16);
  off_work = off_win + N * 4;
  off_acc = (int32_t)(off_work + kWpeStftWaves * M * 16);
  lds_bytes = (int32_t)(off_acc + acc_doubles * 8);
}

__device__ __forceinline__ void wpe_stft_tables(double2* __restrict__ tw, float* __restrict__ win, const float* __restrict__ gwin, int N, int tid) {
  for (int k = tid; k < (N >> 1); k += kWpeStftThreads) {
    double s, c;
    sincospi(-2.0 * (double)k / (double)N, &s, &c);
    tw[k] = make_double2(c, s);
  }
  for (int j = tid; j < N; j += kWpeStftThreads) win[j] = gwin[j];
}

__device__ __forceinline__ int wpe_bitrev(int k, int bits) { return (int)(__brev((unsigned)k) >> (32 - bits)); }

// FFT_M in place on one wave's buffer, input in bit-reversed places, output in natural order.  Pass s joins blocks of 2^(s-1): butterfly
// j pairs i0 = (j >> (s-1)) 2^s + pos with i0 + 2^(s-1), pos = j mod 2^(s-1), twiddle exp(-2 pi i pos / 2^s) = W^(pos 2^(log2n - s)).
__device__ __forceinline__ void wpe_fft_wave(double2* __restrict__ buf, const double2* __restrict__ tw, int log2n, int lane) {
  const int log2m = log2n - 1, pairs = 1 << (log2m - 1);
  for (int s = 1; s <= log2m; ++s) {
    wave_lds_sync();
    const int half = 1 << (s - 1);
    for (int j = lane; j < pairs; j += 64) {
      const int pos = j & (half - 1), i0 = ((j >> (s - 1)) << s) + pos, i1 = i0 + half;
      const double2 w = tw[pos << (log2n - s)], a = buf[i0], c = buf[i1];
      const double2 b = make_double2(c.x * w.x - c.y * w.y, c.x * w.y + c.y * w.x);
      buf[i0] = make_double2(a.x + b.x, a.y + b.y);
      buf[i1] = make_double2(a.x - b.x, a.y - b.y);
    }
  }
  wave_lds_sync();
}

// ---- centred STFT: workgroup = (row, tile of 32 frames), wave = one frame at a time ----
__global__ __launch_bounds__(kWpeStftThreads) void wpe_stft_kernel(const WpeStftParams p) {
  extern __shared__ double2 wpe_stft_lds[];
  char* base = reinterpret_cast<char*>(wpe_stft_lds);
  double2* tw = wpe_stft_lds;
  float* win = reinterpret_cast<float*>(base + p.off_win);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = p.N, M = N >> 1, hop = p.hop, log2m = p.log2n - 1;
  double2* buf = reinterpret_cast<double2*>(base + p.off_work) + (size_t)wave * M;

  const int64_t row = blockIdx.x / p.tiles, b = row / p.D, d = row - b * p.D;
  const int t_begin = (int)(blockIdx.x - row * p.tiles) * kWpeStftTileFrames;
  const int64_t L = min(max((int64_t)p.lengths[b], (int64_t)0), p.num_samples);  // nothing behind it is read, whatever the table says
  const int Tb = L > M ? (int)min(1 + L / hop, (int64_t)p.frames_max) : 0;       // a row too short to reflect has no frame (the host refuses it)
  if (t_begin == 0 && d == 0 && tid == 0 && p.frames_out) p.frames_out[b] = Tb;
  if (t_begin < Tb) {  // workgroup-uniform
    wpe_stft_tables(tw, win, p.window, N, tid);
    __syncthreads();
  }
  const float* __restrict__ x = p.audio + b * p.a_row + d * p.a_chan;
  const bool pairs_ok = (reinterpret_cast<uintptr_t>(x) & 7) == 0;  // frame starts are even: 8-byte loads wherever the row starts on one
  float2* __restrict__ out = p.out + row * p.o_row;
  const int t_end = min(t_begin + kWpeStftTileFrames, p.frames_max);

  for (int t = t_begin + wave; t < t_end; t += kWpeStftWaves) {  // everything below is wave-uniform in t
    float2* __restrict__ o = out + (int64_t)t * p.o_frame;
    if (t >= Tb) {
      for (int k = lane; k <= M; k += 64) o[(int64_t)k * p.o_bin] = make_float2(0.0f, 0.0f);
      continue;
    }
    const int64_t s0 = (int64_t)t * hop - M;
    wave_lds_release();  // the last frame's reads are done with the buffer
    if (pairs_ok && s0 >= 0 && s0 + N <= L) {
      const float2* __restrict__ x2 = reinterpret_cast<const float2*>(x + s0);
      for (int k = lane; k < M; k += 64) {
        const float2 v = x2[k];
        buf[wpe_bitrev(k, log2m)] = make_double2((double)v.x * (double)win[2 * k], (double)v.y * (double)win[2 * k + 1]);
      }
    } else {  // torch's `reflect` at the row's own ends (L > M: one reflection always lands inside); also rows on odd 4-byte addresses
      for (int k = lane; k < M; k += 64) {
        double v[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          int64_t s = s0 + 2 * k + c;
          if (s < 0) s = -s;
          if (s >= L) s = 2 * (L - 1) - s;
          v[c] = (double)x[s] * (double)win[2 * k + c];
        }
        buf[wpe_bitrev(k, log2m)] = make_double2(v[0], v[1]);
      }
    }
    wpe_fft_wave(buf, tw, p.log2n, lane);
    for (int k = lane; k <= M; k += 64) {
      const double2 a = buf[k & (M - 1)], c = buf[(M - k) & (M - 1)];
      const double ex = 0.5 * (a.x + c.x), ey = 0.5 * (a.y - c.y);  // E = (a + conj(c)) / 2
      const double ox = 0.5 * (a.y + c.y), oy = -0.5 * (a.x - c.x);  // O = (a - conj(c)) / 2i
      const double2 w = k < M ? tw[k] : make_double2(-1.0, 0.0);
      o[(int64_t)k * p.o_bin] = make_float2((float)(ex + (w.x * ox - w.y * oy)), (float)(ey + (w.x * oy + w.y * ox)));
    }
  }
}

// ---- inverse STFT with overlap-add: workgroup = (row, R output hops).  Rounds of four frames, one per wave, transformed into the
//      waves' buffers; between two barriers every thread then adds the round's frames, in frame order, to the samples it owns. ----
__global__ __launch_bounds__(kWpeStftThreads) void wpe_istft_kernel(const WpeIstftParams p) {
  extern __shared__ double2 wpe_stft_lds[];
  char* base = reinterpret_cast<char*>(wpe_stft_lds);
  double2* tw = wpe_stft_lds;
  float* win = reinterpret_cast<float*>(base + p.off_win);
  double2* work = reinterpret_cast<double2*>(base + p.off_work);
  double* acc = reinterpret_cast<double*>(base + p.off_acc);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = p.N, M = N >> 1, hop = p.hop, log2m = p.log2n - 1, ov = N / hop, span = kWpeIstftTileHops * hop;

  const int64_t row = blockIdx.x / p.tiles, b = row / p.D, d = row - b * p.D;
  const int g = (int)(blockIdx.x - row * p.tiles);
  const int Tb = min(max(p.frames[b], 0), p.frames_max);
  const int64_t zlen = Tb > 0 ? (int64_t)hop * (Tb - 1) : 0, n0 = (int64_t)g * span;
  const int cnt = (int)min((int64_t)span, p.out_samples - n0);
  float* __restrict__ o = p.out + b * p.o_row + d * p.o_chan + n0;
  const bool live = n0 < zlen;  // workgroup-uniform; a workgroup wholly behind the row's end writes its zeros and nothing else

  if (live) {
    wpe_stft_tables(tw, win, p.window, N, tid);
    for (int i = tid; i < span; i += kWpeStftThreads) acc[i] = 0.0;
    __syncthreads();
    // sample n sits at n + M of the overlap-add; frame t covers [t hop, t hop + N) of it
    const int t_lo = max(0, g * kWpeIstftTileHops - ov / 2 + 1), t_hi = min(Tb, (g + 1) * kWpeIstftTileHops + ov / 2);
    const float2* __restrict__ zin = p.in + row * p.i_row;
    double2* buf = work + (size_t)wave * M;
    for (int tr = t_lo; tr < t_hi; tr += kWpeStftWaves) {
      const int t = tr + wave;
      if (t < t_hi) {
        const float2* __restrict__ f = zin + (int64_t)t * p.i_frame;
        for (int k = lane; k < M; k += 64) {
          const float2 a32 = f[(int64_t)k * p.i_bin], c32 = f[(int64_t)(M - k) * p.i_bin];
          double2 a = make_double2((double)a32.x, (double)a32.y), c = make_double2((double)c32.x, -(double)c32.y);  // c = conj(X[M - k])
          if (k == 0) a.y = c.y = 0.0;
          const double ex = 0.5 * (a.x + c.x), ey = 0.5 * (a.y + c.y), hx = 0.5 * (a.x - c.x), hy = 0.5 * (a.y - c.y);
          const double2 w = tw[k];
          const double ox = hx * w.x + hy * w.y, oy = hy * w.x - hx * w.y;  // O = h conj(W^k)
          buf[wpe_bitrev(k, log2m)] = make_double2(ex - oy, -(ey + ox));    // conj(E + i O)
        }
        wpe_fft_wave(buf, tw, p.log2n, lane);  // x[2 m] = buf[m].x / M, x[2 m + 1] = -buf[m].y / M
      }
      __syncthreads();
      const int last = min(tr + kWpeStftWaves, t_hi) - 1;
      const int lo = (int)max((int64_t)0, (int64_t)tr * hop - M - n0), hi = (int)min((int64_t)span, (int64_t)last * hop + M - n0);
      for (int pos = (lo & ~(kWpeStftThreads - 1)) + tid; pos < hi; pos += kWpeStftThreads) {  // pos = tid (mod 256): the thread owns it
        double a = acc[pos];
        for (int q = 0; tr + q <= last; ++q) {
          const int64_t j = n0 + pos + M - (int64_t)(tr + q) * hop;
          if (j >= 0 && j < N) {
            const double2 r = work[(size_t)q * M + (j >> 1)];
            a += ((j & 1) ? -r.y : r.x) * (double)win[j];
          }
        }
        acc[pos] = a;
      }
      __syncthreads();
    }
  }

  const double inv_m = 1.0 / (double)M;  // a power of two: exact
  auto value = [&](int pos) -> float {
    const int64_t n = n0 + pos;
    if (!live || n >= zlen) return 0.0f;
    const int64_t at = n + M, ta = at >= N ? (at - N) / hop + 1 : 0, tb = min((int64_t)Tb - 1, at / hop);
    double env = 0.0;
    for (int64_t t = ta; t <= tb; ++t) {
      const double w = (double)win[at - t * hop];
      env += w * w;
    }
    return (float)(acc[pos] * inv_m / env);
  };
  // 16-byte stores between a scalar head and tail
  const int head = min(cnt, (int)(((16 - (reinterpret_cast<uintptr_t>(o) & 15)) & 15) >> 2));
  const int body = (cnt - head) >> 2;
  for (int i = tid; i < head; i += kWpeStftThreads) o[i] = value(i);
  for (int v = tid; v < body; v += kWpeStftThreads) {
    const int pos = head + 4 * v;
    *reinterpret_cast<float4*>(o + pos) = make_float4(value(pos), value(pos + 1), value(pos + 2), value(pos + 3));
  }
  for (int i = head + 4 * body + tid; i < cnt; i += kWpeStftThreads) o[i] = value(i);
}

}  // namespace hipfeat
