// Waveform gradient of the six Kaldi layers (the autograd of lhotse/features/kaldi/layers.py, restated as two launches).
//
// grad_frames_kernel.  One WAVE owns one frame at a time, as in kernel_wave.hpp / kernel_stft.hpp, and never synchronises with the rest
// of its workgroup after the table load.  It recomputes the frame's forward from the saved waveform (RowSource, the front end with the
// float64 frame mean, the three passes of fft3_frame and the split step -- in float64 for the four feature kinds, see fft3_frame_f64
// below) and runs the backward of include/hipfeat.h's gradient block:
//   seed      Gbar_k, k = 0 .. H (H = fft / 2), from the output cotangent: power 2 Pbar X, magnitude Mbar X / |X| (0 where X = 0), log
//             Pbar = ybar / (P + 1e-15), mel Pbar_k = sum_m fb[k][m] ybar_m [mel_m > floor] / mel_m with mel_m recomputed, MFCC
//             ybar_mel = dct (lifter * cbar) first; the element that carries the log-energy gives ebar and seeds no bin.  The
//             filterbank is applied BANDED in both directions (grad_tables.hpp), from LDS where the blob fits, else from global memory.
//   adjoint   real FFT: wbar_n = sum_k Re(Gbar_k e^{+2 pi i k n / fft}).  With Y_0 = Re Gbar_0, Y_H = Re Gbar_H, Y_k = Gbar_k / 2 the
//             adjoint split step is Q_k = (Y_k + conj Y_{H-k}) + i e^{+i pi k / H} (Y_k - conj Y_{H-k}), k < H, and
//             wbar[2n] + i wbar[2n+1] = sum_k Q_k e^{+2 pi i k n / H} = conj(FFT_H(conj Q))[n]: the same three register passes as the
//             forward, on conjugated data.  Lane l holds Q_k for k = l + 64 q, which is how fft3_frame takes its input.
//   front end the adjoint of window, pre-emphasis (replicate pad), the two log-energies and the DC removal, in the forward's register
//             layout: lane l holds the pairs (2n, 2n + 1), n = l + 64 q; the next sample's pbar comes from the neighbouring lane.
//   store     the frame's sbar as a row of Nr = (N + 3) & ~3 floats of the workspace (rows, T, Nr), through the wave's LDS buffer into
//             natural order, 16-byte stores; the floats N .. Nr - 1 are zeros.
//
// grad_overlap_add_kernel.  One lane per 4 consecutive samples of a waveform row (16-byte stores counted from the 16-byte boundary at or
// below the row's first element, scalar head and tail).  Sample j gathers sbar[t][i] from every (t, i) whose index (layers.py:747-772:
// j' = t shift - npad_left + i, j' < 0 -> -j' - 1, j' >= S -> 2 S - 1 - j') lands on j, in a FIXED order: ascending t, and within a frame
// the direct tap before the left-reflected before the right-reflected one.  Every element of the row is written (a sample no frame reads
// gets +0.0), so the output needs no memset.  The loop has no bound on the contributors: ceil(N / shift) direct ones and as many
// reflected ones.
//
// No atomics anywhere: the gradient of a row has the same bits alone or in any batch, from run to run and under any piece size.  All
// element indexing is 64-bit.
//
// Both kernels have a ragged instance (rows with a length of their own, kernel_stft.hpp's RaggedRowSource and length table): the frames
// kernel leaves at a row's own frame count, the gather runs over the row's own index map and writes +0.0 from its length on; the
// cotangent, the workspace and the gradient keep the launch's dense (rows, Tmax, .) / (rows, Smax) shapes.
#pragma once
#include "common.hpp"
#include "fft_common.hpp"
#include "kernel_stft.hpp"
#include "kernel_wave.hpp"

namespace hipfeat {

enum : int32_t { GRAD_SPEC = 0, GRAD_LOG_SPEC = 1, GRAD_FBANK = 2, GRAD_MFCC = 3, GRAD_FRAMES = 4, GRAD_SPECTRUM = 5 };

struct GradParams {
  const float* wave;    // first row of the piece; row b at wave + b * row_stride
  const float* gout;    // cotangent of the output, first row of the piece: [rows][T][width], may be NULL (GRAD_FRAMES)
  const float* glog_e;  // GRAD_FRAMES: cotangent of the log-energies [rows][T], may be NULL
  float* ws;            // [rows][T][Nr]
  const float* window;  // [N]
  const float2* tw;     // W_2H^k, k < H
  const double2* tw64;  // the same in float64 (the four feature kinds)
  const float* blob;    // grad_tables.hpp (M > 0)
  int64_t row_stride, num_samples, frames_per_row, blocks_per_row, width;
  int32_t N, Nr, shift, npad_left, frames_per_wave, flags, mode;
  int32_t M, C, blob_floats, blob_in_lds, off_fwd, off_bwd, off_dct, off_lifter;
  float preemph, log_energy_floor, mel_floor, log_offset;
};

constexpr int grad_buf_floats(int N1) { return 288 * N1 + 16; }  // per wave: the padded FFT buffer of the float64 forward (72 N1 + 4 complex)

// ---- the forward spectrum in float64 ----------------------------------------------------------------------------------------------------
// The four feature kinds divide by what they recompute (1 / mel_m, 1 / (P + 1e-15), X / |X|), so the error of a SMALL bin of X comes back
// multiplied by rms(X) / |X_k| -- 65 x for the bins under the first mel filters of a pre-emphasised noise frame.  In float32 the packed
// half-size transform loses to the reference's real FFT there: bin k is the difference E_k + W^k O_k of two terms as large as the bins
// around fft / 2 - k, and measured 3.4 x the reference's own float32 error on such a row.  The recomputed spectrum therefore
// runs the same three passes and the same split step in float64 (W_2H^k from a float64 table), on a windowed frame that is float64 from
// the samples on (the float64 frame mean, the pre-emphasis and the window, rounded once): a frame rounded to float32 first puts
// eps rms(X) onto every bin, which is as much as a float32 FFT does.  Everything after the spectrum is float32.
struct cd {
  double x, y;
};
__device__ __forceinline__ cd operator+(cd a, cd b) { return cd{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cd operator-(cd a, cd b) { return cd{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cd cdmul(cd a, cd w) { return cd{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }

// W_16^j = (cos, -sin)(2 pi j / 16), j < 8
__device__ __forceinline__ cd w16(int j) {
  constexpr double C1 = 0.92387953251128673848, S1 = 0.38268343236508977173, R2 = 0.70710678118654752440;
  constexpr double c[8] = {1.0, C1, R2, S1, 0.0, -S1, -R2, -C1}, sn[8] = {0.0, S1, R2, C1, 1.0, C1, R2, S1};
  return cd{c[j], -sn[j]};
}

// R-point FFT in registers, natural order in and out: decimation in time, fully unrolled (R = 2, 4, 8, 16; x is read with `stride`)
template <int R>
__device__ __forceinline__ void fft_f64(const cd* x, int stride, cd* X) {
  if constexpr (R == 1) {
    X[0] = x[0];
  } else {
    cd e[R / 2], o[R / 2];
    fft_f64<R / 2>(x, 2 * stride, e);
    fft_f64<R / 2>(x + stride, 2 * stride, o);
#pragma unroll
    for (int k = 0; k < R / 2; ++k) {
      cd t = o[k];
      if (k != 0) t = (4 * k == R) ? cd{t.y, -t.x} : cdmul(t, w16(k * (16 / R)));
      X[k] = e[k] + t;
      X[k + R / 2] = e[k] - t;
    }
  }
}

__device__ __forceinline__ cd twiddle_h_f64(const double2* __restrict__ tw, int m, int H) {  // W_H^m from W_2H^k (k < H)
  int t = 2 * m;
  const bool neg = t >= H;
  t -= neg ? H : 0;
  const double2 w = tw[t];
  return neg ? cd{-w.x, -w.y} : cd{w.x, w.y};
}

// fft3_frame (kernel_wave.hpp) in float64: the same index maps and the same padded layout e + (e >> 3), tw = W_2H^k in LDS
template <int N1>
__device__ __forceinline__ void fft3_frame_f64(cd* zf, const double2* __restrict__ tw, int lane, const cd* x) {
  constexpr int H = 64 * N1;
  const int lp = lane + (lane >> 3);
  {
    cd A[N1];
    fft_f64<N1>(x, 1, A);
    const int n2 = lane >> 3;
#pragma unroll
    for (int k1 = 1; k1 < N1; ++k1) A[k1] = cdmul(A[k1], twiddle_h_f64(tw, 8 * n2 * k1, H));
#pragma unroll
    for (int k1 = 0; k1 < N1; ++k1) zf[72 * k1 + lp] = A[k1];
  }
  wave_lds_sync();
  constexpr int ITEMS = 8 * N1, ROUNDS = (ITEMS + 63) / 64;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int it = lane + 64 * r;
    if (it < ITEMS) {
      const int k1 = it >> 3, n3 = it & 7;
      cd v[8], B[8];
#pragma unroll
      for (int n2 = 0; n2 < 8; ++n2) v[n2] = zf[72 * k1 + 9 * n2 + n3];
      fft_f64<8>(v, 1, B);
#pragma unroll
      for (int k2 = 0; k2 < 8; ++k2) zf[72 * k1 + 9 * k2 + n3] = cdmul(B[k2], twiddle_h_f64(tw, n3 * (k1 + N1 * k2), H));
    }
  }
  wave_lds_sync();
  {
    cd X[ROUNDS][8];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const int it = lane + 64 * r;
      if (it < ITEMS) {
        const int k1 = it >> 3, k2 = it & 7;
        cd v[8];
#pragma unroll
        for (int n3 = 0; n3 < 8; ++n3) v[n3] = zf[72 * k1 + 9 * k2 + n3];
        fft_f64<8>(v, 1, X[r]);
      }
    }
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const int it = lane + 64 * r;
      if (it < ITEMS) {
        const int k1 = it >> 3, k2 = it & 7;
#pragma unroll
        for (int k3 = 0; k3 < 8; ++k3) zf[k1 + N1 * k2 + 8 * N1 * k3] = X[r][k3];
      }
    }
  }
  wave_lds_sync();
}

template <int N1, class Src>
__device__ __forceinline__ void grad_frames_body(const GradParams& p, const typename Src::Args& sa) {
  constexpr int H = 64 * N1, BUF = grad_buf_floats(N1);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  HF_POISON_LDS(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* buf = smem + wv * BUF;                                    // wave-private
  float* winl = smem + 4 * BUF;                                    // [N] window, shared by the four waves
  float2* tw = reinterpret_cast<float2*>(winl + ((p.N + 3) & ~3));  // [H] W_2H^k
  v2* twh = reinterpret_cast<v2*>(tw + H);                         // [H] W_H^m
  double2* tw64 = reinterpret_cast<double2*>(twh + H);             // [H] W_2H^k in float64
  float* blobl = reinterpret_cast<float*>(tw64 + H);               // the filterbank blob when it fits
  const int N = p.N, mode = p.mode;
  const bool spectral = mode != GRAD_FRAMES;
  for (int i = tid; i < N; i += 256) winl[i] = p.window[i];
  if (spectral) {
    for (int i = tid; i < H; i += 256) {
      tw[i] = p.tw[i];
      twh[i] = twiddle_h(p.tw, i, H);
      if (mode <= GRAD_MFCC) tw64[i] = p.tw64[i];
    }
  }
  if (p.blob_in_lds)
    for (int i = tid; i < p.blob_floats; i += 256) blobl[i] = p.blob[i];
  __syncthreads();
  const float* __restrict__ blob = p.blob_in_lds ? blobl : p.blob;
  const int4* fwd = reinterpret_cast<const int4*>(blob + p.off_fwd);
  const int4* bwd = reinterpret_cast<const int4*>(blob + p.off_bwd);

  StftParams sp{};
  sp.wave = p.wave, sp.row_stride = p.row_stride, sp.num_samples = p.num_samples;
  sp.frames_per_row = p.frames_per_row, sp.blocks_per_row = p.blocks_per_row;
  const Src src(sp, sa, (int64_t)blockIdx.x);
  const int64_t row = src.row;
  const int64_t T = Src::kPads ? p.frames_per_row : src.T;  // frames of a cotangent / workspace row: dense at Tmax for a ragged batch
  const bool want_e = (p.flags & F_USE_ENERGY) != 0, raw_e = (p.flags & F_RAW_ENERGY) != 0, mag = (p.flags & F_FFT_MAG) != 0;
  const int M = p.M;
  const int64_t fbase = src.fb * 4 * p.frames_per_wave;
#pragma unroll 1
  for (int it = 0; it < p.frames_per_wave; ++it) {
    const int64_t f = fbase + 4 * it + wv;
    if (f >= src.T) break;  // (a ragged row: its cotangent rows from T_b on are never read, their workspace rows never written)
    const int64_t j0 = f * p.shift - p.npad_left;
    const int64_t frame = row * T + f;
    const float* __restrict__ grow = p.gout ? p.gout + frame * p.width : nullptr;

    // ---- the forward's front end (kernel_stft.hpp): samples, float64 mean, d = x - mean -------------------------------------------
    v2 d[N1];
    float mean = 0.f;
    double mean64 = 0.0;
    {
      double s = 0.0;
      const bool inside = src.inside(j0, (N + 1) & ~1);
      const float* __restrict__ w = src.base(j0);
#pragma unroll
      for (int q = 0; q < N1; ++q) {
        const int m0 = 2 * (lane + 64 * q);
        v2 v = {0.f, 0.f};
        if (m0 < N) {
          if (inside) {
            __builtin_memcpy(&v, w + m0, sizeof(v2));
            if (m0 + 1 >= N) v.y = 0.f;
          } else {
            v = src.slow_pair(j0 + m0, m0 + 1 < N);
          }
        }
        d[q] = v;
        s += (double)v.x + (double)v.y;
      }
      if (p.flags & F_REMOVE_DC) {
        mean64 = wave_sum_f64(s) / (double)N;
        mean = (float)mean64;
      }
    }
    // y[m] = (d[m] - c d[max(m-1, 0)]) w[m], d = x - mean.  The float32 y is the forward's and feeds the two log-energies; the feature
    // kinds also take it in float64 from the samples themselves (yd: the float64 mean, one rounding at the end), for the float64 spectrum
    // below: the rounding of a float32 y alone moves a bin at 6e-5 of the frame's rms by 1e-3 of itself (sweep case 87).
    v2 y[N1];
    cd yd[N1];
    float sum_d = 0.f, sum_w = 0.f;
    const bool feature = mode <= GRAD_MFCC;
    const double c64 = (double)p.preemph;
    float last_y = 0.f;  // the sample in front of this register's first one, in lane 63
#pragma unroll
    for (int q = 0; q < N1; ++q) {
      const int m0 = 2 * (lane + 64 * q);
      const v2 x = d[q];  // the samples; d[q] becomes x - mean below
      const float offer = (q > 0 && lane == 63) ? last_y : x.y;
      float xm = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(4 * ((lane - 1) & 63), __builtin_bit_cast(int, offer)));
      if (q == 0 && lane == 0) xm = x.x;  // the replicate pad
      last_y = x.y;
      const float dm = xm - mean;
      d[q].x = m0 < N ? x.x - mean : 0.f;
      d[q].y = m0 + 1 < N ? x.y - mean : 0.f;
      v2 v = {0.f, 0.f};
      cd vd = {0.0, 0.0};
      if (m0 < N) {
        const v2 wn = *reinterpret_cast<const v2*>(winl + m0);
        v.x = (d[q].x - p.preemph * dm) * wn.x;
        if (m0 + 1 < N) v.y = (d[q].y - p.preemph * d[q].x) * wn.y;
        if (feature) {
          const double dx = (double)x.x - mean64;
          vd.x = (dx - c64 * ((double)xm - mean64)) * (double)wn.x;
          if (m0 + 1 < N) vd.y = (((double)x.y - mean64) - c64 * dx) * (double)wn.y;
        }
      }
      y[q] = v;
      yd[q] = vd;
      sum_d = fmaf(d[q].x, d[q].x, fmaf(d[q].y, d[q].y, sum_d));
      sum_w = fmaf(v.x, v.x, fmaf(v.y, v.y, sum_w));
    }

    // ---- ebar: the cotangent of the log-energy, times 2 / (sum + 1e-15) where the floor did not take over (layers.py:859-870) ------
    float ecoef = 0.f;
    if (want_e) {
      float ebar = 0.f;
      if (mode == GRAD_FRAMES) ebar = p.glog_e ? p.glog_e[frame] : 0.f;
      else ebar = grow[0];
      const float sum = wave_sum(raw_e ? sum_d : sum_w) + 1e-15f;
      ecoef = logf(sum) > p.log_energy_floor ? 2.0f * ebar / sum : 0.f;
    }

    v2 wb[N1];  // wbar in the forward's layout
    wave_lds_sync();  // the previous frame's readers of this wave's buffer are done
    if (mode == GRAD_FRAMES) {
#pragma unroll
      for (int q = 0; q < N1; ++q) {
        const int m0 = 2 * (lane + 64 * q);
        v2 v = {0.f, 0.f};
        if (grow != nullptr && m0 < N) {
          if (m0 + 1 < N) __builtin_memcpy(&v, grow + m0, sizeof(v2));
          else v.x = grow[m0];
        }
        wb[q] = v;
      }
    } else {
      v2* zf = reinterpret_cast<v2*>(buf);
      v2 glo[N1 / 2 + 1], ghi[N1 / 2 + 1];  // Gbar at k = lane + 64 q <= H / 2 and at H - k
      if (mode == GRAD_SPECTRUM) {
#pragma unroll
        for (int q = 0; q <= N1 / 2; ++q) {
          const int k = lane + 64 * q;
          glo[q] = ghi[q] = v2{0.f, 0.f};
          if (k <= H / 2) {
            __builtin_memcpy(&glo[q], grow + 2 * k, sizeof(v2));
            if (k < H / 2) __builtin_memcpy(&ghi[q], grow + 2 * (H - k), sizeof(v2));
            if (want_e && k == 0) glo[q] = v2{0.f, 0.f};  // bin 0 carries the log-energy (layers.py:317-318)
          }
        }
      } else {
        // ---- the forward spectrum: X[k] and X[H - k] per lane, P = |X|^2 or |X| ------------------------------------------------
        cd* zd = reinterpret_cast<cd*>(buf);
        fft3_frame_f64<N1>(zd, tw64, lane, yd);
        v2 xlo[N1 / 2 + 1], xhi[N1 / 2 + 1];
        float plo[N1 / 2 + 1], phi[N1 / 2 + 1];
#pragma unroll
        for (int q = 0; q <= N1 / 2; ++q) {
          const int k = lane + 64 * q;
          xlo[q] = xhi[q] = v2{0.f, 0.f};
          plo[q] = phi[q] = 0.f;
          if (k <= H / 2) {
            const cd a = zd[k], b = zd[(H - k) & (H - 1)];
            const double ex = 0.5 * (a.x + b.x), ey = 0.5 * (a.y - b.y);
            const double ox = 0.5 * (a.y + b.y), oy = -0.5 * (a.x - b.x);
            const double2 wk = tw64[k];
            const double tx = wk.x * ox - wk.y * oy, ty = wk.x * oy + wk.y * ox;
            const double lx = ex + tx, ly = ey + ty, hx = ex - tx, hy = ty - ey;
            xlo[q] = v2{(float)lx, (float)ly};
            xhi[q] = v2{(float)hx, (float)hy};
            double v = lx * lx + ly * ly, u = hx * hx + hy * hy;
            if (mag) { v = sqrt(v); u = sqrt(u); }
            plo[q] = (float)v;
            phi[q] = (float)u;
          }
        }
        wave_lds_sync();
        // ---- Pbar at the lane's bins ---------------------------------------------------------------------------------------
        float blo[N1 / 2 + 1], bhi[N1 / 2 + 1];
        if (mode == GRAD_SPEC || mode == GRAD_LOG_SPEC) {
#pragma unroll
          for (int q = 0; q <= N1 / 2; ++q) {
            const int k = lane + 64 * q;
            blo[q] = bhi[q] = 0.f;
            if (k <= H / 2) {
              blo[q] = (want_e && k == 0) ? 0.f : grow[k];  // bin 0 carries the log-energy (layers.py:399, 470)
              if (k < H / 2) bhi[q] = grow[H - k];
              if (mode == GRAD_LOG_SPEC) {
                blo[q] = blo[q] / (plo[q] + p.log_offset);
                bhi[q] = bhi[q] / (phi[q] + p.log_offset);
              }
            }
          }
        } else {
          // the power row into LDS, mel energies by one lane per filter, g_m = ybar_m [mel_m > floor] / mel_m behind the row
#pragma unroll
          for (int q = 0; q <= N1 / 2; ++q) {
            const int k = lane + 64 * q;
            if (k <= H / 2) {
              buf[k] = plo[q];
              if (k < H / 2) buf[H - k] = phi[q];
            }
          }
          wave_lds_sync();
          float* gm = buf + 2 * H - 120;  // [M <= 128]; H + 1 <= 2 H - 120
          const int ecol = (mode == GRAD_FBANK && want_e) ? 1 : 0;  // the energy column is prepended (layers.py:575)
          float gv[2] = {0.f, 0.f};
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const int m = lane + 64 * r;
            if (m < M) {
              const int4 dsc = fwd[m];
              float mel = 0.f;
              for (int t = 0; t < dsc.y; ++t) mel = fmaf(buf[dsc.x + t], blob[dsc.z + t], mel);
              float yb = 0.f;
              if (mode == GRAD_FBANK) {
                yb = grow[ecol + m];
              } else {  // ybar_mel = dct (lifter * cbar) (layers.py:708-722); with use_energy C0 is replaced and seeds nothing
                const float* __restrict__ dct_t = blob + p.off_dct;
                const float* __restrict__ lift = blob + p.off_lifter;
                for (int c = want_e ? 1 : 0; c < p.C; ++c) yb = fmaf(dct_t[(int64_t)c * M + m], lift[c] * grow[c], yb);
              }
              gv[r] = mel > p.mel_floor ? yb / mel : 0.f;
            }
          }
          wave_lds_sync();  // every lane has read the power row
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const int m = lane + 64 * r;
            if (m < M) gm[m] = gv[r];
          }
          wave_lds_sync();
#pragma unroll
          for (int q = 0; q <= N1 / 2; ++q) {
            const int k = lane + 64 * q;
            blo[q] = bhi[q] = 0.f;
            if (k <= H / 2) {
              const int4 da = bwd[k];
              float acc = 0.f;
              for (int t = 0; t < da.y; ++t) acc = fmaf(blob[da.z + t], gm[da.x + t], acc);
              blo[q] = acc;
              if (k < H / 2) {
                const int4 db = bwd[H - k];
                acc = 0.f;
                for (int t = 0; t < db.y; ++t) acc = fmaf(blob[db.z + t], gm[db.x + t], acc);
                bhi[q] = acc;
              }
            }
          }
          wave_lds_sync();  // gm is read; the buffer is written again below
        }
        // ---- Gbar = 2 Pbar X, or Mbar X / |X| with 0 where X = 0 -------------------------------------------------------------------
#pragma unroll
        for (int q = 0; q <= N1 / 2; ++q) {
          float sl, sh;
          if (mag) {
            sl = plo[q] > 0.f ? blo[q] / plo[q] : 0.f;
            sh = phi[q] > 0.f ? bhi[q] / phi[q] : 0.f;
          } else {
            sl = 2.0f * blo[q], sh = 2.0f * bhi[q];
          }
          glo[q] = xlo[q] * sl;
          ghi[q] = xhi[q] * sh;
        }
      }
      // ---- adjoint real FFT: Y into LDS, Q_k from Y_k and Y_{H-k}, the forward's three passes on conj Q --------------------------
#pragma unroll
      for (int q = 0; q <= N1 / 2; ++q) {
        const int k = lane + 64 * q;
        if (k <= H / 2) {
          zf[k] = k == 0 ? v2{glo[q].x, 0.f} : glo[q] * 0.5f;
          if (k < H / 2) zf[H - k] = k == 0 ? v2{ghi[q].x, 0.f} : ghi[q] * 0.5f;
        }
      }
      wave_lds_sync();
      v2 qc[N1];
#pragma unroll
      for (int q = 0; q < N1; ++q) {
        const int k = lane + 64 * q;
        const v2 a = zf[k], b0 = zf[H - k];
        const v2 b = {b0.x, -b0.y};
        const float2 wk = tw[k];  // e^{+i pi k / H} = (wk.x, -wk.y)
        const float c = wk.x, s = -wk.y;
        const float dx = a.x - b.x, dy = a.y - b.y;
        const float qx = a.x + b.x - (c * dy + s * dx), qy = a.y + b.y + (c * dx - s * dy);
        qc[q] = v2{qx, -qy};
      }
      wave_lds_sync();  // every lane has read Y
      fft3_frame<N1>(zf, twh, lane, qc);
#pragma unroll
      for (int q = 0; q < N1; ++q) {
        const int m0 = 2 * (lane + 64 * q);
        const v2 z = zf[lane + 64 * q];
        wb[q] = v2{m0 < N ? z.x : 0.f, m0 + 1 < N ? -z.y : 0.f};  // the adjoint of zero padding is truncation
      }
      wave_lds_sync();
    }

    // ---- front end: windowed energy, window, pre-emphasis, raw energy, DC removal ------------------------------------------------------
    v2 pb[N1];
#pragma unroll
    for (int q = 0; q < N1; ++q) {
      const int m0 = 2 * (lane + 64 * q);
      v2 v = wb[q];
      if (want_e && !raw_e) v = v + y[q] * ecoef;
      v2 wn = {0.f, 0.f};
      if (m0 < N) {
        wn = *reinterpret_cast<const v2*>(winl + m0);
        if (m0 + 1 >= N) wn.y = 0.f;
      }
      pb[q] = v * wn;
    }
    double sd = 0.0;
#pragma unroll
    for (int q = 0; q < N1; ++q) {
      // pbar[2n + 2]: lane l < 63 wants lane l + 1's first element of this register, lane 63 wants lane 0's of the next register: lane 0
      // offers that one (nobody reads its current one here)
      const float offer = lane == 0 ? (q + 1 < N1 ? pb[q + 1 < N1 ? q + 1 : q].x : 0.f) : pb[q].x;
      const float nx = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(4 * ((lane + 1) & 63), __builtin_bit_cast(int, offer)));
      v2 v = {pb[q].x - p.preemph * pb[q].y, pb[q].y - p.preemph * nx};
      if (q == 0 && lane == 0) v.x -= p.preemph * pb[q].x;  // the replicate pad: d[0] is also its own predecessor
      if (want_e && raw_e) v = v + d[q] * ecoef;
      wb[q] = v;  // dbar; zero from tap N on, because pbar is
      sd += (double)v.x + (double)v.y;
    }
    if (p.flags & F_REMOVE_DC) {
      const float mean = (float)(wave_sum_f64(sd) / (double)N);
#pragma unroll
      for (int q = 0; q < N1; ++q) {
        const int m0 = 2 * (lane + 64 * q);
        if (m0 < N) wb[q].x -= mean;
        if (m0 + 1 < N) wb[q].y -= mean;
      }
    }
    // ---- the workspace row: natural order through LDS, 16-byte stores --------------------------------------------------------------
#pragma unroll
    for (int q = 0; q < N1; ++q) *reinterpret_cast<v2*>(buf + 2 * (lane + 64 * q)) = wb[q];
    wave_lds_sync();
    float* __restrict__ wrow = p.ws + frame * (int64_t)p.Nr;
    for (int pp = 4 * lane; pp < p.Nr; pp += 256) *reinterpret_cast<f32x4*>(wrow + pp) = *reinterpret_cast<const f32x4*>(buf + pp);
    wave_lds_sync();  // the buffer is reused by the next frame
  }
}

template <int N1>
__global__ __launch_bounds__(256, (N1 == 16 ? 1 : 2)) void grad_frames_kernel(const GradParams p) {
  grad_frames_body<N1, RowSource>(p, NoSourceArgs{});
}

// ... on RaggedRowSource (kernel_stft.hpp): row b has S_b samples and T_b frames of its own
template <int N1>
__global__ __launch_bounds__(256, (N1 == 16 ? 1 : 2)) void grad_frames_ragged_kernel(const GradParams p, const RaggedArgs a) {
  grad_frames_body<N1, RaggedRowSource>(p, a);
}

struct GradOlaParams {
  const float* ws;  // [rows][T][Nr]
  float* gwave;     // row b at gwave + b * stride
  int64_t stride, S, T, groups_per_row, rows;
  int32_t N, Nr, shift, npad_left;
};

// the frames that hold position u (u + npad_left = a >= 0): t in [lo, hi], empty when lo > hi
__device__ __forceinline__ void grad_cover(int64_t a, int64_t T, int N, int shift, int64_t& lo, int64_t& hi) {
  if (a < 0) {
    lo = 1, hi = 0;
    return;
  }
  hi = a / shift;
  if (hi > T - 1) hi = T - 1;
  const int64_t first = a - N + 1;
  lo = first <= 0 ? 0 : (first + shift - 1) / shift;
}

__device__ __forceinline__ float grad_sample(const GradOlaParams& p, const float* __restrict__ ws_row, int64_t j) {
  const int64_t a0 = j + p.npad_left, a1 = -j - 1 + p.npad_left, a2 = 2 * p.S - 1 - j + p.npad_left;
  int64_t lo0, hi0, lo1, hi1, lo2, hi2;
  grad_cover(a0, p.T, p.N, p.shift, lo0, hi0);
  grad_cover(a1, p.T, p.N, p.shift, lo1, hi1);
  grad_cover(a2, p.T, p.N, p.shift, lo2, hi2);
  int64_t lo = INT64_MAX, hi = -1;
  if (lo0 <= hi0) lo = lo0, hi = hi0;
  if (lo1 <= hi1) lo = lo1 < lo ? lo1 : lo, hi = hi1 > hi ? hi1 : hi;
  if (lo2 <= hi2) lo = lo2 < lo ? lo2 : lo, hi = hi2 > hi ? hi2 : hi;
  float acc = 0.f;
  for (int64_t t = lo; t <= hi; ++t) {
    const float* __restrict__ fr = ws_row + t * (int64_t)p.Nr;
    const int64_t t0 = t * p.shift;
    if (t >= lo0 && t <= hi0) acc += fr[a0 - t0];
    if (t >= lo1 && t <= hi1) acc += fr[a1 - t0];
    if (t >= lo2 && t <= hi2) acc += fr[a2 - t0];
  }
  return acc;
}

// `table` (a ragged batch, else NULL): rows x {S_b, T_b}.  The output row and the workspace row keep the launch's p.S = Smax samples and
// p.T = Tmax frames; row b gathers its own T_b frames over the index map of S_b samples, and every sample from S_b on gets +0.0.
__device__ __forceinline__ void grad_overlap_add_body(const GradOlaParams& p, const int64_t* __restrict__ table) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = gid / p.groups_per_row, g = gid - row * p.groups_per_row;
  if (row >= p.rows) return;
  float* __restrict__ orow = p.gwave + row * p.stride;
  const float* __restrict__ ws_row = p.ws + row * p.T * (int64_t)p.Nr;
  const int head = (int)((reinterpret_cast<uintptr_t>(orow) / sizeof(float)) & 3);
  const int64_t row_end = (int64_t)head + p.S, pp = 4 * g;  // the row is [head, row_end), counted from the 16-byte boundary below it
  if (pp >= row_end) return;
  GradOlaParams q = p;  // the row's own index map
  if (table != nullptr) q.S = table[2 * row], q.T = table[2 * row + 1];
  float e[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t j = pp + i - head;
    e[i] = (j >= 0 && j < q.S) ? grad_sample(q, ws_row, j) : 0.f;
  }
  if (pp >= head && pp + 4 <= row_end) {
    *reinterpret_cast<f32x4*>(orow + (pp - head)) = f32x4{e[0], e[1], e[2], e[3]};
  } else {  // the row's first or last element cuts the group
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (pp + i >= head && pp + i < row_end) orow[pp + i - head] = e[i];
  }
}

__global__ __launch_bounds__(256) void grad_overlap_add_kernel(const GradOlaParams p) { grad_overlap_add_body(p, nullptr); }

__global__ __launch_bounds__(256) void grad_overlap_add_ragged_kernel(const GradOlaParams p, const int64_t* table) { grad_overlap_add_body(p, table); }

}  // namespace hipfeat
