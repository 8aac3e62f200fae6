// Weighted prediction error (WPE) dereverberation of a batch of STFTs: one workgroup per (cut, frequency bin), everything but the
// spectrogram itself on chip ("WPE").  gfx950 only.
//
// The algorithm (nara_wpe's wpe_v6 with psd_context = 0, as lhotse/augmentation/wpe.py:87-130 calls it), for one cut and one bin,
// Y[d, t] complex64, D channels, K = taps * D:
//   Yt[tau * D + d, t] = Y[d, t - delay - tau], tau = 0 ... taps - 1, zero where the frame index is negative
//   X = Y;  `iterations` times:
//     p_t = mean_d |X[d, t]|^2,  eps = 1e-10 * max_t p_t,  lambda_t = 1 / max(p_t, eps)
//     R = sum_{t in S} lambda_t Yt_t Yt_t^H (K x K),  P = sum_{t in S} lambda_t Yt_t Y_t^H (K x D),  G = R^-1 P,  X = Y - G^H Yt
//   S: every frame ("full") or t >= delay + taps - 1 ("valid"); p_t and its maximum are always taken over every frame.
// Deliberate difference: where R has no Cholesky factor (a pivot that is not a positive finite number) the bin returns X = Y, bit for
// bit -- a silent bin, or "valid" with no frame in S.  nara_wpe falls back to lstsq there, or gives NaN.
//
// Arithmetic: Y converts to float64 exactly; X, p_t, R, P, the Cholesky factor and G are float64; the weights are kept as
// w_t = max_t p_t / max(p_t, eps) in float32 (1 ... 1e10: G does not change when every lambda_t is scaled by one factor).  p_t
// itself passes through the float32 array on its way, so |Y| of a bin must lie within about 1e-19 ... 1e19; the output is rounded once to complex64.  X is never stored between iterations:
// a pass that needs X_t recomputes it from the Y tile and the current G.
//
// Ragged batches: with a frame table (WpeParams::frames) the T of a workgroup is its cut's own count; the frames behind it are not read and
// are written as zeros.  Everything below runs on that T, so a cut's bits are those of the cut alone (given the same time tile).
//
// Order of summation: a thread owns a BS x BS block of R or P and one of `slices` residues of the frame index; it adds its frames in
// ascending order, and the slices are folded by a butterfly over the lanes (K <= 16).  Above, a wave owns 16 x 16 blocks on the float64
// matrix instruction, four frames per step in ascending order (mono blocks split over two waves by alternate steps, folded in order).  No atomics, no workspace: same bits from run to run and
// for any batch composition.
#pragma once
#include "common.hpp"

namespace hipfeat {

constexpr int kWpeThreads = 256;
constexpr int kWpeMaxK = 64;
constexpr int kWpeMaxTile = 256;           // frames per time tile while the tile fits (one frame per thread in the X passes)
constexpr int kWpeMinTile = 32;
constexpr int kWpeFmaMaxK = 16;            // K up to here: pass 2 on float64 FMAs; above: on the float64 matrix instruction
constexpr int kWpeLdsBytes = 160 * 1024;   // LDS of a gfx950 compute unit

struct WpeParams {
  const float2* in;
  float2* out;
  const int32_t* frames;                // per cut: only its first frames[cut] frames exist (clamped to 0 ... T); null: all T of every cut
  int64_t in_row, in_bin, in_frame;     // element (complex64) strides of the (B * D, F, T) input ...
  int64_t out_row, out_bin, out_frame;  // ... and output
  int32_t D, F, T, taps, delay, iterations, valid;
  int32_t K, halo, tile, width;         // halo = delay + taps - 1 frames in front of a tile; width = tile + halo
  int32_t bs, nb, ndb, n_rblk, n_blk;   // blocks of bs x bs: nb block rows, n_rblk = nb (nb + 1) / 2 of R, then nb * ndb of P
  int32_t log2_slices;                  // frame residues per block (a power of two <= 64, so a block's slices share a wave)
  int32_t off_p, off_inv, off_misc, off_lam, off_tile, lds_bytes;  // LDS map (bytes); R (packed lower triangle) at 0
};

// Fills the derived fields.  false: the working set does not fit the LDS of one compute unit (`p.lds_bytes` says what it needs).
inline bool wpe_plan(WpeParams& p) {
  p.K = p.taps * p.D;
  p.halo = p.delay + p.taps - 1;
  p.bs = p.K <= 16 ? 2 : 4;
  p.nb = (p.K + p.bs - 1) / p.bs;
  p.ndb = (p.D + p.bs - 1) / p.bs;
  p.n_rblk = p.nb * (p.nb + 1) / 2;
  p.n_blk = p.n_rblk + p.nb * p.ndb;
  p.log2_slices = 6;
  while (p.log2_slices > 0 && ((int64_t)p.n_blk << p.log2_slices) > kWpeThreads) --p.log2_slices;
  int64_t off = (int64_t)p.K * (p.K + 1) / 2 * 16;
  p.off_p = (int32_t)off;
  off += (int64_t)p.K * p.D * 16;
  p.off_inv = (int32_t)off;
  off += (int64_t)p.K * 8;
  p.off_misc = (int32_t)off;
  off += 8 * 8;
  p.off_lam = (int32_t)off;
  off += (((int64_t)p.T + 1) & ~(int64_t)1) * 4;
  p.off_tile = (int32_t)off;
  for (p.tile = kWpeMaxTile;; p.tile >>= 1) {
    p.width = p.tile + p.halo;
    const int64_t total = off + (int64_t)p.D * p.width * 8;
    p.lds_bytes = (int32_t)std::min<int64_t>(total, INT32_MAX);
    if (total <= kWpeLdsBytes) return true;
    if (p.tile == kWpeMinTile) return false;
  }
}

__device__ __forceinline__ double2 wpe_cvt(float2 v) { return make_double2((double)v.x, (double)v.y); }
__device__ __forceinline__ int wpe_tri(int i, int j) { return i * (i + 1) / 2 + j; }  // packed lower triangle, i >= j

// X[d, t] = Y[d, t] - sum_i conj(G[i, d]) Yt[i, t] for the four channels d = dc ... dc + 3 (zero past D); x = t - tile start.
__device__ __forceinline__ void wpe_predict4(const WpeParams& p, const float2* __restrict__ tile, const double2* __restrict__ G, int x, int dc,
                                             bool have_g, double2 (&X)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) X[r] = dc + r < p.D ? wpe_cvt(tile[(dc + r) * p.width + x + p.halo]) : make_double2(0.0, 0.0);
  if (!have_g) return;
  for (int tau = 0; tau < p.taps; ++tau) {
    const float2* src = tile + x + p.taps - 1 - tau;
    const double2* g = G + (size_t)tau * p.D * p.D + dc;
    for (int d2 = 0; d2 < p.D; ++d2, g += p.D) {
      const double2 y = wpe_cvt(src[d2 * p.width]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (dc + r < p.D) {
          const double2 c = g[r];
          X[r].x -= c.x * y.x + c.y * y.y;
          X[r].y -= c.x * y.y - c.y * y.x;
        }
      }
    }
  }
}

typedef double wpe_d4 __attribute__((ext_vector_type(4)));

// MFMA = false: pass 2 on float64 FMAs, BS x BS register blocks.  MFMA = true: pass 2 on v_mfma_f64_16x16x4_f64 -- a wave owns up to four
// 16 x 16 blocks of R's lower block triangle or of P (K and D padded to 16), four frames per instruction, a conj(b) as four real products.
template <int BS, bool MFMA>
__global__ __launch_bounds__(kWpeThreads) void wpe_kernel(const WpeParams p) {
  extern __shared__ double2 wpe_lds[];
  char* base = reinterpret_cast<char*>(wpe_lds);
  double2* R = wpe_lds;
  double2* P = reinterpret_cast<double2*>(base + p.off_p);
  double* inv = reinterpret_cast<double*>(base + p.off_inv);
  double* misc = reinterpret_cast<double*>(base + p.off_misc);  // [0..3] per-wave maxima, [4] "no Cholesky factor"
  float* lam = reinterpret_cast<float*>(base + p.off_lam);
  float2* tile = reinterpret_cast<float2*>(base + p.off_tile);

  const int tid = threadIdx.x;
  const int64_t cut = blockIdx.x / p.F, bin = blockIdx.x - cut * p.F;
  const float2* __restrict__ yin = p.in + cut * p.D * p.in_row + bin * p.in_bin;
  float2* __restrict__ zout = p.out + cut * p.D * p.out_row + bin * p.out_bin;
  const int K = p.K, D = p.D, T = p.frames ? min(max(p.frames[cut], 0), p.T) : p.T;  // workgroup-uniform

  auto load_tile = [&](int t0) {  // frames t0 - halo ... t0 + tile - 1 of every channel, zero outside 0 ... T - 1
    __syncthreads();
    for (int e = tid; e < D * p.width; e += kWpeThreads) {
      const int d = e / p.width, t = t0 - p.halo + (e - d * p.width);
      float2 v = make_float2(0.0f, 0.0f);
      if (t >= 0 && t < T) v = yin[(int64_t)d * p.in_row + (int64_t)t * p.in_frame];
      tile[e] = v;
    }
    __syncthreads();
  };

  const int slices = 1 << p.log2_slices, group = tid >> p.log2_slices, slice = tid & (slices - 1);
  const int groups = kWpeThreads >> p.log2_slices;
  const int tmin = p.valid ? p.halo : 0;
  bool have_g = false, failed = false;

  for (int it = 0; it < p.iterations; ++it) {
    // ---- pass 1: the power of the recomputed X, and its maximum ----
    double mx = 0.0;
    for (int t0 = 0; t0 < T; t0 += p.tile) {
      load_tile(t0);
      const int t = t0 + tid;
      if (tid < p.tile && t < T) {
        double pw = 0.0;
        for (int dc = 0; dc < D; dc += 4) {
          double2 X[4];
          wpe_predict4(p, tile, P, tid, dc, have_g, X);
#pragma unroll
          for (int r = 0; r < 4; ++r) pw += X[r].x * X[r].x + X[r].y * X[r].y;
        }
        pw /= (double)D;
        lam[t] = (float)pw;
        mx = fmax(mx, pw);
      }
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
    if ((tid & 63) == 0) misc[tid >> 6] = mx;
    __syncthreads();
    mx = fmax(fmax(misc[0], misc[1]), fmax(misc[2], misc[3]));
    const double eps = 1e-10 * mx;
    for (int t = tid; t < T; t += kWpeThreads) lam[t] = (float)(mx / fmax((double)lam[t], eps));  // a silent bin: 0 / 0, no factor below

    // ---- pass 2: R and P ----
    if constexpr (MFMA) {
      const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
      const int nb16 = (K + 15) >> 4, ndb16 = (D + 15) >> 4, nr16 = nb16 * (nb16 + 1) / 2, nblk16 = nr16 + nb16 * ndb16;
      const int wpb = nblk16 <= 2 ? 2 : 1;  // the mono case has one block of R and one of P: two waves each, alternate chunks of 4 frames
      const int units = nblk16 * wpb;       // unit u = block * wpb + slice -> wave u % 4, slot (u / 4) % 4, round u / 16
      for (int u0 = 0; u0 < units; u0 += 16) {
        int bi[4], bj[4], sl[4], ao[4], bo[4];
        bool on[4], isp[4];
        wpe_d4 cre[4], cim[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int u = u0 + q * 4 + wave, blk = u / wpb;
          on[q] = u < units;
          sl[q] = u - blk * wpb;
          isp[q] = blk >= nr16;
          bi[q] = 0;
          if (isp[q]) {
            bi[q] = (blk - nr16) / ndb16;
            bj[q] = (blk - nr16) - bi[q] * ndb16;
          } else {
            while ((bi[q] + 1) * (bi[q] + 2) / 2 <= blk) ++bi[q];
            bj[q] = blk - bi[q] * (bi[q] + 1) / 2;
          }
          const int ig = bi[q] * 16 + li, jg = bj[q] * 16 + li;
          ao[q] = on[q] && ig < K ? (ig % D) * p.width + p.taps - 1 - ig / D : -1;
          if (isp[q]) bo[q] = on[q] && jg < D ? jg * p.width + p.halo : -1;
          else bo[q] = on[q] && jg < K ? (jg % D) * p.width + p.taps - 1 - jg / D : -1;
          cre[q] = cim[q] = wpe_d4{0.0, 0.0, 0.0, 0.0};
        }
        for (int t0 = 0; t0 < T; t0 += p.tile) {
          load_tile(t0);
          for (int c = 0; 4 * c < p.tile && t0 + 4 * c < T; ++c) {
            const int x = 4 * c + lk, t = t0 + x;
            const double w = t < T && t >= tmin ? (double)lam[t] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              if (!on[q] || (c & (wpb - 1)) != sl[q]) continue;  // wave-uniform
              const float2 ya = ao[q] >= 0 ? tile[ao[q] + x] : make_float2(0.0f, 0.0f);
              const float2 yb = bo[q] >= 0 ? tile[bo[q] + x] : make_float2(0.0f, 0.0f);
              const double ar = w * (double)ya.x, ai = w * (double)ya.y, br = (double)yb.x, bim = (double)yb.y;
              cre[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, cre[q], 0, 0, 0);
              cre[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bim, cre[q], 0, 0, 0);
              cim[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, cim[q], 0, 0, 0);
              cim[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ar, bim, cim[q], 0, 0, 0);
            }
          }
        }
        for (int s = 0; s < wpb; ++s) {  // the slices of a block fold in slice order; register v of a lane is row 4 v + lane / 16
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (!on[q] || sl[q] != s) continue;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int ig = bi[q] * 16 + 4 * v + lk, jg = bj[q] * 16 + li;
              double2* dst = nullptr;
              if (isp[q] && ig < K && jg < D) dst = P + ig * D + jg;
              if (!isp[q] && ig < K && jg <= ig) dst = R + wpe_tri(ig, jg);
              if (dst) {
                double2 val = make_double2(cre[q][v], cim[q][v]);
                if (s > 0) val.x += dst->x, val.y += dst->y;
                *dst = val;
              }
            }
          }
          __syncthreads();
        }
      }
    } else {
      for (int blk0 = 0; blk0 < p.n_blk; blk0 += groups) {
        const int blk = blk0 + group;
        const bool active = blk < p.n_blk;
        int bi = 0, bj = 0;
        const bool is_p = blk >= p.n_rblk;
        if (active && !is_p) {
          while ((bi + 1) * (bi + 2) / 2 <= blk) ++bi;
          bj = blk - bi * (bi + 1) / 2;
        } else if (active) {
          bi = (blk - p.n_rblk) / p.ndb;
          bj = (blk - p.n_rblk) - bi * p.ndb;
        }
        int roff[BS], coff[BS];  // where row i / column j of the block lies in the tile at x = 0; -1: past K (or D)
  #pragma unroll
        for (int r = 0; r < BS; ++r) {
          const int i = bi * BS + r, j = bj * BS + r;
          roff[r] = active && i < K ? (i % D) * p.width + p.taps - 1 - i / D : -1;
          if (is_p) coff[r] = active && j < D ? j * p.width + p.halo : -1;
          else coff[r] = active && j < K ? (j % D) * p.width + p.taps - 1 - j / D : -1;
        }
        double2 acc[BS][BS];
  #pragma unroll
        for (int r = 0; r < BS; ++r)
  #pragma unroll
          for (int c = 0; c < BS; ++c) acc[r][c] = make_double2(0.0, 0.0);

        for (int t0 = 0; t0 < T; t0 += p.tile) {
          load_tile(t0);
          if (!active) continue;
          for (int x = slice; x < p.tile && t0 + x < T; x += slices) {
            if (t0 + x < tmin) continue;
            const double w = (double)lam[t0 + x];
            double2 a[BS], b[BS];
  #pragma unroll
            for (int r = 0; r < BS; ++r) {
              a[r] = roff[r] >= 0 ? wpe_cvt(tile[roff[r] + x]) : make_double2(0.0, 0.0);
              b[r] = coff[r] >= 0 ? wpe_cvt(tile[coff[r] + x]) : make_double2(0.0, 0.0);
              a[r].x *= w;
              a[r].y *= w;
            }
  #pragma unroll
            for (int r = 0; r < BS; ++r)
  #pragma unroll
              for (int c = 0; c < BS; ++c) {  // a conj(b)
                acc[r][c].x += a[r].x * b[c].x + a[r].y * b[c].y;
                acc[r][c].y += a[r].y * b[c].x - a[r].x * b[c].y;
              }
          }
        }
        for (int off = slices >> 1; off > 0; off >>= 1)
  #pragma unroll
          for (int r = 0; r < BS; ++r)
  #pragma unroll
            for (int c = 0; c < BS; ++c) {
              acc[r][c].x += __shfl_xor(acc[r][c].x, off);
              acc[r][c].y += __shfl_xor(acc[r][c].y, off);
            }
        if (active && slice == 0) {
  #pragma unroll
          for (int r = 0; r < BS; ++r)
  #pragma unroll
            for (int c = 0; c < BS; ++c) {
              const int i = bi * BS + r, j = bj * BS + c;
              if (is_p) {
                if (i < K && j < D) P[i * D + j] = acc[r][c];
              } else if (i < K && j <= i) {
                R[wpe_tri(i, j)] = acc[r][c];
              }
            }
        }
      }
    }
    __syncthreads();

    // ---- R = L L^H in place, column by column, row i on lane i of the first wave; inv[j] = 1 / L[j, j] ----
    if (tid < 64) {
      const int i = tid;
      bool bad = false;
      for (int j = 0; j < K; ++j) {
        double2 s = make_double2(0.0, 0.0);
        if (i >= j && i < K) {
          s = R[wpe_tri(i, j)];
          const double2 *li = R + wpe_tri(i, 0), *lj = R + wpe_tri(j, 0);
          for (int k = 0; k < j; ++k) {
            const double2 a = li[k], b = lj[k];
            s.x -= a.x * b.x + a.y * b.y;
            s.y -= a.y * b.x - a.x * b.y;
          }
        }
        const double pivot = __shfl(s.x, j);
        if (!(pivot > 0.0 && pivot < __builtin_inf())) {
          bad = true;
          break;
        }
        const double diag = sqrt(pivot), rdiag = 1.0 / diag;
        if (i == j) {
          R[wpe_tri(j, j)] = make_double2(diag, 0.0);
          inv[j] = rdiag;
        } else if (i > j && i < K) {
          R[wpe_tri(i, j)] = make_double2(s.x * rdiag, s.y * rdiag);
        }
        wave_lds_sync();
      }
      if (i == 0) misc[4] = bad ? 1.0 : 0.0;
    }
    __syncthreads();
    if (misc[4] != 0.0) {
      failed = true;
      break;
    }

    // ---- G = L^-H L^-1 P in place.  Step k reads row k (final up to its 1 / L[k, k], which every reader applies) and updates the
    //      rows behind it; the rows are scaled once all steps are done. ----
    const int KD = K * D;
    for (int k = 0; k < K; ++k) {
      for (int e = tid; e < KD; e += kWpeThreads) {
        const int i = e / D, d = e - i * D;
        if (i > k) {
          const double2 z = P[k * D + d], l = R[wpe_tri(i, k)];
          const double zx = z.x * inv[k], zy = z.y * inv[k];
          double2 v = P[e];
          v.x -= l.x * zx - l.y * zy;
          v.y -= l.x * zy + l.y * zx;
          P[e] = v;
        }
      }
      __syncthreads();
    }
    for (int e = tid; e < KD; e += kWpeThreads) {
      const double s = inv[e / D];
      P[e].x *= s;
      P[e].y *= s;
    }
    __syncthreads();
    for (int k = K - 1; k >= 0; --k) {
      for (int e = tid; e < KD; e += kWpeThreads) {
        const int i = e / D, d = e - i * D;
        if (i < k) {
          const double2 g = P[k * D + d], l = R[wpe_tri(k, i)];  // conj(L[k, i]) g
          const double gx = g.x * inv[k], gy = g.y * inv[k];
          double2 v = P[e];
          v.x -= l.x * gx + l.y * gy;
          v.y -= l.x * gy - l.y * gx;
          P[e] = v;
        }
      }
      __syncthreads();
    }
    for (int e = tid; e < KD; e += kWpeThreads) {
      const double s = inv[e / D];
      P[e].x *= s;
      P[e].y *= s;
    }
    have_g = true;  // load_tile's barrier stands between these writes and the first reader
  }

  // ---- the last pass writes X (or Y itself where a factorisation failed) ----
  for (int t0 = 0; t0 < T; t0 += p.tile) {
    load_tile(t0);
    const int t = t0 + tid;
    if (tid < p.tile && t < T) {
      for (int dc = 0; dc < D; dc += 4) {
        double2 X[4];
        wpe_predict4(p, tile, P, tid, dc, have_g && !failed, X);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (dc + r < D) zout[(int64_t)(dc + r) * p.out_row + (int64_t)t * p.out_frame] = make_float2((float)X[r].x, (float)X[r].y);
      }
    }
  }
  const int rest = p.T - T;  // frames behind a shorter cut's own: zero
  for (int e = tid; e < D * rest; e += kWpeThreads) {
    const int d = e / rest, t = T + (e - d * rest);
    zout[(int64_t)d * p.out_row + (int64_t)t * p.out_frame] = make_float2(0.0f, 0.0f);
  }
}

}  // namespace hipfeat
