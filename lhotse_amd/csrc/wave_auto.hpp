// The skeleton that the wave-autonomous kernels (kernel_fft512c.hpp, kernel_fft256c.hpp, kernel_fft1024c.hpp, kernel_fft2048c.hpp,
// kernel_whisper3.hpp) and the tile kernels (kernel_fft512b.hpp, kernel_fft256.hpp) have in common: span staging, the small
// instruction-selection helpers and the phase timers of experiment builds.  Everything is forced inline and stateless, and a piece is
// shared only where every instance compiles to the device code it had with its own copy (tools/isa_diff.py; DESIGN.md section
// 4.3 lists what stays in a kernel and why).  block_owner, wave_lds_sync and wave_lds_release are in common.hpp,
// the row sums in fft_common.hpp.
#pragma once
#include "common.hpp"
#include "fft_common.hpp"

namespace hipfeat {

#define HFC_SEP() asm volatile("")  // keeps hipcc from merging two ds_read_b64 into one half-rate ds_read2_b64 (tools/ubench/lds_rate.hip)
// lane-index multiplies: v_mul_u32_u24 issues at the full VALU rate, v_mul_lo_u32 at a quarter of it
__device__ __forceinline__ int mul24(int a, int b) { return (int)__umul24((unsigned)a, (unsigned)b); }

// r = m ? a : b per lane with the mask in an SGPR pair (VOP3 encoding: the VOP2 / VCC form of v_cndmask issues ~5x slower on gfx950)
__device__ __forceinline__ float sel64(unsigned long long m, float a, float b) {
  float r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
  return r;
}
__device__ __forceinline__ v2 sel64(unsigned long long m, v2 a, v2 b) { return v2{sel64(m, a.x, b.x), sel64(m, a.y, b.y)}; }

// Phase timers (experiment builds, -DHIPFEAT_PHASE_TIMERS): per-wave shader-clock totals of up to seven phases and, in slot 7, the rounds.
// HFC_TIMERS() declares the accumulators in front of the round loop, HFC_T(i) closes phase i, HFC_ROUND() ends a round and
// HFC_DUMP(lane, slot) writes the wave's row of g_phase_buf (slot = workgroup * waves per workgroup + wave).
#ifdef HIPFEAT_PHASE_TIMERS
__device__ unsigned long long* g_phase_buf;  // [grid * waves][8], written once per wave (no atomics)
#define HFC_TIMERS() unsigned long long hfc_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, hfc_last = __builtin_readcyclecounter()
#define HFC_T(i) { const unsigned long long tt_ = __builtin_readcyclecounter(); hfc_acc[i] += tt_ - hfc_last; hfc_last = tt_; }
#define HFC_ROUND() hfc_acc[7] += 1
#define HFC_DUMP(lane_, slot_)                                             \
  if ((lane_) == 0 && g_phase_buf) {                                       \
    unsigned long long* o_ = g_phase_buf + (size_t)(slot_) * 8;            \
    for (int i_ = 0; i_ < 8; ++i_) o_[i_] = hfc_acc[i_];                   \
  }
#else
#define HFC_TIMERS()
#define HFC_T(i)
#define HFC_ROUND()
#define HFC_DUMP(lane_, slot_)
#endif

// ---- span staging ----------------------------------------------------------------------------------------------------------------------
// LDS-DMA: lane i supplies the global address of its 16 bytes, the hardware writes them to piece base + 16 i; a piece is 1 KiB.

// One wave requests its span of xs_floats floats (a multiple of 4): up to MAXFULL whole pieces under a wave-uniform test each, then the
// lanes of the partial piece that start inside the span.  src: wave-uniform address of the first sample; lane4 = 4 * lane.
// What keeps the device code as it was when every kernel had this loop in its own body (tools/isa_diff.py): a piece's LDS address is taken
// before its global one; a span length that the instance knows at compile time comes as XS (an argument turns constant only after
// inlining, past the first round of address folding), and the partial piece's offset is then signed (4 lane4 <= 1008), which lets hipcc
// split the constant part off as a 64-bit step as it did there.
template <int MAXFULL, int XS = 0>
__device__ __forceinline__ void span_request(const char* src, float* xs, int xs_floats, unsigned lane4) {
  typedef __attribute__((address_space(3))) void lds_void;
  const int n = XS > 0 ? XS : xs_floats, nfull = n >> 8;
#pragma unroll
  for (int ch = 0; ch < MAXFULL; ++ch) {
    if (ch < nfull) {
      lds_void* dst = (lds_void*)(xs + ch * 256);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + ((unsigned)ch * 1024u + 4u * lane4)), dst, 16, 0, 0);
    }
  }
  if ((unsigned)nfull * 256u + lane4 < (unsigned)n) {
    lds_void* dst = (lds_void*)(xs + nfull * 256);
    const char* from = XS > 0 ? src + ((XS >> 8) * 1024 + (int)(4u * lane4)) : src + ((unsigned)nfull * 1024u + 4u * lane4);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)from, dst, 16, 0, 0);
  }
}
// The span that starts at sample j0 of the cut w[0 .. num_samples): by LDS-DMA where it lies inside the cut, else through the kernel's
// edge rule (reflection, zero padding of a batch row), which fills the whole buffer with per-lane loads: edge(j0).
template <int MAXFULL, int XS = 0, class Edge>
__device__ __forceinline__ void stage_span_wave(const float* w, int64_t j0, float* xs, int xs_floats, int num_samples, unsigned lane4,
                                                Edge edge) {
  if (j0 >= 0 && j0 + (XS > 0 ? XS : xs_floats) <= num_samples)
    span_request<MAXFULL, XS>(reinterpret_cast<const char*>(w + j0), xs, xs_floats, lane4);
  else edge(j0);
}
// The edge rule's loop for one wave: xs[i] = sample(j0 + i)
template <class Sample>
__device__ __forceinline__ void span_fill(float* xs, int xs_floats, unsigned lane4, int64_t j0, Sample sample) {
  for (int i = (int)(lane4 >> 2); i < xs_floats; i += 64) xs[i] = sample(j0 + i);
}

// Tile kernels (4 waves share one span buffer): the waves take the pieces round-robin, whole pieces only (the buffer is a multiple of
// 1 KiB past the span); edge tiles go through load_sample on all 256 threads.  lane16 = 16 * lane.
__device__ __forceinline__ void stage_span_tile(const float* w, int64_t j0, float* xs, int xs_floats, int nchunks, const CutDesc& cd,
                                                int wv, int tid, unsigned lane16) {
  if (j0 >= 0 && j0 + (int64_t)nchunks * 256 <= cd.num_samples) {
    const char* src = reinterpret_cast<const char*>(w + j0);  // uniform
    for (int ch = wv; ch < nchunks; ch += 4)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + ((unsigned)ch * 1024u + lane16)),
                                       (__attribute__((address_space(3))) void*)(xs + ch * 256), 16, 0, 0);
  } else {
    for (int i = tid; i < xs_floats; i += 256) xs[i] = load_sample(w, j0 + i, cd.num_samples, cd.padded_len);  // the whole buffer: rows past N are read (and masked or met by a zero window) too
  }
}

}  // namespace hipfeat
