// Polyphase sinc resampler (speed perturbation), SURVEY.md section 8f row 1.
//
// Reference: ResampleTensor = _get_sinc_resample_kernel + _apply_sinc_resample_kernel
// (lhotse/augmentation/resample.py:184-315), reached from Speed.__call__ (lhotse/augmentation/torchaudio.py:37-42).
// The reference zero-pads the waveform by (width, width + orig) and runs conv1d(stride = orig) with `new` filters
// of 2*width + orig taps:  y[j*new + ph] = sum_i xpad[j*orig + i] * K[ph][i].
//
// Here: one workgroup = `outs_per_block` consecutive output samples of one cut.  The input span those outputs
// touch is staged in LDS once (coalesced, zero outside the cut), the filter bank too when it is small (speed
// factors 0.9 / 1.1 give 10 x 23 / 10 x 25 taps); each lane then accumulates one output at a time as an
// ascending-tap fmaf chain and stores it coalesced.
#pragma once
#include "common.hpp"

namespace hipfeat {

struct ResCut {
  int64_t in_off, out_off;
  int32_t in_len, out_len;
  int32_t first_block, pad;
};

struct ResampleParams {
  const float* in;
  float* out;
  const ResCut* cuts;
  const float* kernel;  // [nw][kw]
  int32_t num_cuts, orig, nw, kw, width, outs_per_block, span_floats, kernel_in_lds;
};

__device__ __forceinline__ int find_res_cut(const ResCut* __restrict__ cuts, int num_cuts, int blk) {
  int lo = 0, hi = num_cuts - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (cuts[mid].first_block <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void resample_kernel(const ResampleParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* xs = smem;                  // [span_floats]
  float* kl = smem + p.span_floats;  // [nw * kw] when kernel_in_lds
  const int tid = threadIdx.x;
  const int cut = find_res_cut(p.cuts, p.num_cuts, blockIdx.x);
  const ResCut cd = p.cuts[cut];
  const int o0 = (blockIdx.x - cd.first_block) * p.outs_per_block;
  const int o1 = min(o0 + p.outs_per_block, cd.out_len);
  const int j0 = o0 / p.nw, j1 = (o1 - 1) / p.nw;
  const int span = (j1 - j0) * p.orig + p.kw;
  const int64_t x0 = (int64_t)j0 * p.orig - p.width;  // input index of xs[0]
  const float* __restrict__ x = p.in + cd.in_off;
  for (int i = tid; i < span; i += 256) {
    const int64_t s = x0 + i;
    xs[i] = (s >= 0 && s < cd.in_len) ? x[s] : 0.0f;
  }
  if (p.kernel_in_lds)
    for (int i = tid; i < p.nw * p.kw; i += 256) kl[i] = p.kernel[i];
  __syncthreads();
  const float* __restrict__ kt = p.kernel_in_lds ? kl : p.kernel;
  float* __restrict__ y = p.out + cd.out_off;
  for (int o = o0 + tid; o < o1; o += 256) {
    const int j = o / p.nw, ph = o - j * p.nw;
    const float* xr = xs + (j - j0) * p.orig;
    const float* kr = kt + ph * p.kw;
    float acc = 0.f;
    for (int i = 0; i < p.kw; ++i) acc = fmaf(xr[i], kr[i], acc);
    y[o] = acc;
  }
}

// --------------------------------------------------------------------------------------
// Fast path for the ratios speed perturbation actually uses (compile-time ORIG / NEW / WIDTH).
//
// One lane = one input hop j (ORIG input samples -> NEW output samples): it reads its KW = 2*WIDTH + ORIG taps of
// x from LDS once and feeds NEW independent accumulators, so one LDS read serves NEW FMAs.  The filter bank is
// wave-uniform: it is read through the scalar cache (`kt` = transposed bank [KW][NEWP], one row per tap) and the
// FMAs take it as an SGPR operand -- no LDS or VGPR traffic for coefficients.  Per accumulator the order is the
// same ascending-tap fmaf chain as the generic kernel (results are bit-identical between the two).
// The NEW results per lane are transposed through LDS (re-using the input span) so the stores are coalesced.
// --------------------------------------------------------------------------------------
template <int ORIG, int NEW, int WIDTH>
struct ResampleFast {
  static constexpr int KW = 2 * WIDTH + ORIG;
  static constexpr int NEWP = (NEW + 3) & ~3;       // row pitch of the transposed bank
  static constexpr int HOPS = 256;                  // hops per block (one per lane)
  static constexpr int SPAN = HOPS * ORIG + KW - ORIG;  // input samples the block touches
  static constexpr int OUTS = HOPS * NEW;
  static constexpr int LDS_FLOATS = SPAN > OUTS ? SPAN : OUTS;
};

// The work of one workgroup: hops [j0, j0 + 256) of cut `cd`.  `xs` = G::LDS_FLOATS floats of LDS.
template <int ORIG, int NEW, int WIDTH>
__device__ __forceinline__ void resample_fast_block(const float* __restrict__ in, float* __restrict__ out, const ResCut& cd, int block_in_cut,
                                                    const float* __restrict__ kt, float* xs) {
  using G = ResampleFast<ORIG, NEW, WIDTH>;
  const int tid = threadIdx.x;
  const int j0 = block_in_cut * G::HOPS;
  const int x0 = j0 * ORIG - WIDTH;  // j0 * ORIG <= in_len + ORIG < 2^31
  const float* __restrict__ x = in + cd.in_off;
  {
    constexpr int N = (G::SPAN + 255) / 256;
    float v[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {  // all loads in flight before the first LDS write
      const int s = x0 + tid + 256 * k;
      v[k] = ((unsigned)s < (unsigned)cd.in_len) ? x[s] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (tid + 256 * k < G::SPAN) xs[tid + 256 * k] = v[k];
  }
  __syncthreads();
  float acc[NEW];
#pragma unroll
  for (int ph = 0; ph < NEW; ++ph) acc[ph] = 0.f;
  const float* xr = xs + tid * ORIG;
  // the bank through the constant address space: wave-uniform, read-only for the whole launch -> scalar loads, SGPR operands.  (As a plain
  // pointer that came out of a struct the compiler has to assume that the kernel's own stores may alias it, fetches the 250 coefficients
  // with vector loads into 250 registers per lane -- and the mixed launch ran at half the rate of the per-factor ones.)
  const __attribute__((address_space(4))) float* ktc = (const __attribute__((address_space(4))) float*)kt;
#pragma unroll
  for (int i = 0; i < G::KW; ++i) {
    const float xv = xr[i];
#pragma unroll
    for (int ph = 0; ph < NEW; ++ph) acc[ph] = fmaf(xv, ktc[i * G::NEWP + ph], acc[ph]);
  }
  __syncthreads();
#pragma unroll
  for (int ph = 0; ph < NEW; ++ph) xs[tid * NEW + ph] = acc[ph];
  __syncthreads();
  const int o0 = j0 * NEW;
  const int n = min(G::OUTS, cd.out_len - o0);
  float* __restrict__ y = out + cd.out_off + o0;
#pragma unroll
  for (int k = 0; k < NEW; ++k)
    if (tid + 256 * k < n) y[tid + 256 * k] = xs[tid + 256 * k];
}

template <int ORIG, int NEW, int WIDTH>
__global__ __launch_bounds__(256) void resample_fast_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            const ResCut* __restrict__ cuts, const float* __restrict__ kt,
                                                            int num_cuts) {
  using G = ResampleFast<ORIG, NEW, WIDTH>;
  __shared__ float xs[G::LDS_FLOATS];
  const int cut = find_res_cut(cuts, num_cuts, blockIdx.x);
  const ResCut cd = cuts[cut];
  resample_fast_block<ORIG, NEW, WIDTH>(in, out, cd, blockIdx.x - cd.first_block, kt, xs);
}

// --------------------------------------------------------------------------------------
// Matrix-core path for ratios with many phases (44.1 -> 16 kHz = 441:160, 441:320, 441:640, 147:80): runtime orig / nw / kw.
//
// For one cut the resampler is the GEMM  Y[j][ph] = sum_i X[j][i] * K[ph][i],  X[j][i] = xpad[j * orig + i]  (j = hop, ph < nw,
// i < kw).  A workgroup owns 16 * HT consecutive hops of one cut (resample_tables.hpp has the geometry); their input span is staged in
// LDS once, coalesced, zero outside [0, in_len), exactly as resample_kernel stages it.  A wave owns phase tiles (16 phases each,
// tile = wave, wave + 4, ...) and, per phase tile, HT accumulators of 16 hops x 16 phases on v_mfma_f32_16x16x4_f32:
//   A[r][k] = xs[(16 t + r) * orig + i0 + k]      lane l holds A[l & 15][l >> 4]        (LDS; stride orig over the rows)
//   B[k][c] = kt[(i0 + k) * nwp + ph0 + c]        lane l holds B[l >> 4][l & 15]        (L2; four 64-byte rows per wave load)
//   D[row][c], row = 4 (l >> 4) + reg, c = l & 15                                       (64-byte runs of consecutive outputs)
// One B fragment serves the HT hop tiles, whose accumulators are independent: with HT = 2 and two workgroups per CU, or HT = 4, a SIMD
// has four MFMA chains in flight.  The tap loop takes 16 taps per trip and has the next trip's B fragments in flight meanwhile.
//
// Summation order (contract): the accumulator starts at 0, i0 ascends in steps of 4, and the k index of an MFMA is the ascending tap
// i0 + k; an f32 MFMA is bit for bit the k-ordered fmaf chain D = fma(a3, b3, fma(a2, b2, fma(a1, b1, fma(a0, b0, C)))).  That is the
// chain of resample_kernel, tap by tap.  The taps kw .. kwp - 1 of kt (kwp = kw rounded up to 16) are zeros: for finite samples fma(x, 0, acc) == acc, so the
// outputs compare equal to resample_kernel's, value for value.  (Two corners where the padding shows: an accumulator that is exactly
// -0 behind tap kw - 1 comes out as +0, and a non-finite sample reaches the hops whose up to 15 padded taps touch it.)
//
// d_in == d_out with the outputs behind every input of the launch is fine: a workgroup reads inputs and writes outputs only.
// --------------------------------------------------------------------------------------
struct ResMfmaParams {
  const float* in;
  float* out;
  const ResCut* cuts;
  const float* kt;  // [kwp][nwp]
  int32_t num_cuts, orig, nw, width, kwp, nwp, span_floats, pad;
};

typedef float res_f32x4 __attribute__((ext_vector_type(4)));

template <int HT>
__global__ __launch_bounds__(256) void resample_mfma_kernel(const ResMfmaParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* xs = smem;  // [span_floats]
  const int tid = threadIdx.x;
  const int cut = find_res_cut(p.cuts, p.num_cuts, blockIdx.x);
  const ResCut cd = p.cuts[cut];
  const int j0 = (blockIdx.x - cd.first_block) * (16 * HT);
  const int64_t x0 = (int64_t)j0 * p.orig - p.width;  // input index of xs[0]
  const float* __restrict__ x = p.in + cd.in_off;
  for (int base = 0; base < p.span_floats; base += 8 * 256) {  // eight loads per lane in flight before the first LDS write
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t s = x0 + base + tid + 256 * k;
      v[k] = (base + tid + 256 * k < p.span_floats && s >= 0 && s < cd.in_len) ? x[s] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (base + tid + 256 * k < p.span_floats) xs[base + tid + 256 * k] = v[k];
  }
  __syncthreads();
  const int lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles = p.nwp >> 4;
  float* __restrict__ y = p.out + cd.out_off;
  const float* ap = xs + r * p.orig + q;
  for (int pt = wave; pt < tiles; pt += 4) {
    res_f32x4 acc[HT];
#pragma unroll
    for (int t = 0; t < HT; ++t) acc[t] = res_f32x4{0.f, 0.f, 0.f, 0.f};
    const float* __restrict__ bp = p.kt + (size_t)q * p.nwp + pt * 16 + r;
    // kwp is a multiple of 16: a trip takes 16 taps = four B fragments and their 4 * HT MFMAs in tap order.  Two register sets take turns:
    // while a trip computes from one, the next trip's fragments are on their way from L2 into the other (behind the last trip its rows
    // are fetched again and not used: no branch around a load, no register move that would wait for one).
    float ba[4], bb[4];
    auto fetch = [&](float (&b)[4], int i0) {
      const int ip = min(i0, p.kwp - 16);
#pragma unroll
      for (int u = 0; u < 4; ++u) b[u] = bp[(size_t)(ip + 4 * u) * p.nwp];
      __builtin_amdgcn_sched_barrier(0);  // issued here, in front of the LDS reads and MFMAs of the trip that runs meanwhile
    };
    auto trip = [&](const float (&b)[4], int i0) {
      float a[4][HT];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int t = 0; t < HT; ++t) a[u][t] = ap[t * 16 * p.orig + i0 + 4 * u];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int t = 0; t < HT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][t], b[u], acc[t], 0, 0, 0);
    };
    fetch(ba, 0);
    for (int i0 = 0; i0 < p.kwp; i0 += 32) {
      fetch(bb, i0 + 16);
      trip(ba, i0);
      fetch(ba, i0 + 32);
      if (i0 + 16 < p.kwp) trip(bb, i0 + 16);
    }
    const int ph = pt * 16 + r;
    if (ph < p.nw) {
#pragma unroll
      for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int64_t o = (int64_t)(j0 + t * 16 + q * 4 + g) * p.nw + ph;
          if (o < cd.out_len) y[o] = acc[t][g];
        }
    }
  }
}

}  // namespace hipfeat
