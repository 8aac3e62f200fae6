// Collation of the cuts of a mini-batch on the device: ragged float32 runs of the arena -> one dense, zero-padded (rows, row_len) tensor.
//
// Reference: collate_audio (lhotse/dataset/collation.py:148-260: cuts.pad to the longest, then collate_vectors(..., padding_value=0.0))
// behind AudioSamples (lhotse/dataset/input_strategies.py:208-299) and behind return_audio=True of the feature input strategy.
//
// One launch for the whole mini-batch.  Row r of `out` receives the row's `len` samples at arena + src_off, starting at element dst_off
// of the row; every other element of the row is written as +0.  Every element of out[0 : rows * row_len] is written exactly once (no
// memset in front), nothing else is written, the arena is only read.  float32 output is a bit copy (the samples travel as 32-bit
// patterns); binary16 / bfloat16 output is one round-to-nearest-even conversion per sample (binary16: the hardware conversion, with
// subnormals; bfloat16: the integer rounding torch uses, NaN -> 0x7fc0).
//
// A work item = one tile of kCoTile output elements of one row; work item w belongs to row w / tiles_per_row (every row has as many
// tiles), a flat 1-D grid walks them with a 64-bit grid stride.  Tiles are counted from the 16-byte boundary at or below the ROW's first
// byte -- rows start at r * row_len elements, so every row has its own alignment -- and a lane owns whole 16-byte groups of the
// destination (4 float32 or 8 two-byte elements): a group that lies wholly inside the row is stored with one 16-byte store, the groups
// that the row's first and last element cut are stored element by element (the scalar head and tail, as kernel_level.hpp).  A group
// wholly in padding stores zeros and loads nothing, so a tile in padding only stores.
//
// The source is in general not aligned like the destination (packed items lie back to back, dst_off is arbitrary).  A group wholly
// inside the samples reads its 4 (8) consecutive floats with 16-byte loads at DWORD alignment: on gfx950 under HSA the compiler treats
// a wide global load at 4-byte alignment as legal and fast and emits one global_load_dwordx4 for it -- it does the same to four
// separate dword loads of a lane, so "dword loads" is not a form that survives to the code object.  When (src - dst) % 4 == 0 in
// elements those addresses are 16-byte aligned; otherwise the same instruction straddles.  Which of the two a row gets is a property
// of the row, so no wave diverges on it.  The groups that the first and last sample cut load sample by sample.
// All element indexing is 64-bit.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "collate_tables.hpp"
#include "common.hpp"

namespace hipfeat {

struct CoArgs {
  const uint32_t* arena;  // float32 samples, as bit patterns
  void* out;
  const CoRow* rows;  // device
  int64_t row_len, tiles_per_row, work_items;
};

typedef uint32_t co_u4 __attribute__((ext_vector_type(4)));
typedef co_u4 co_u4_dword_aligned __attribute__((aligned(4)));

template <typename OutT>
struct CoOut;
template <>
struct CoOut<float> {
  typedef uint32_t Bits;
  static __device__ __forceinline__ Bits cvt(uint32_t x) { return x; }
};
template <>
struct CoOut<__half> {
  typedef uint16_t Bits;
  static __device__ __forceinline__ Bits cvt(uint32_t x) { return __builtin_bit_cast(uint16_t, (_Float16)__builtin_bit_cast(float, x)); }
};
template <>
struct CoOut<__hip_bfloat16> {
  typedef uint16_t Bits;
  static __device__ __forceinline__ Bits cvt(uint32_t x) {
    if ((x & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    return (uint16_t)((x + 0x7fffu + ((x >> 16) & 1u)) >> 16);
  }
};

__device__ __forceinline__ CoRow co_uniform(const CoRow* p) {  // every dword through v_readfirstlane (the index was workgroup-uniform)
  const int* w = reinterpret_cast<const int*>(p);
  union {
    int w[8];
    CoRow t;
  } u;
#pragma unroll
  for (int i = 0; i < 8; ++i) u.w[i] = __builtin_amdgcn_readfirstlane(w[i]);
  return u.t;
}

// V converted elements -> the dwords of one 16-byte store
template <typename O, int V>
__device__ __forceinline__ co_u4 co_pack(const typename O::Bits (&e)[V]) {
  co_u4 q;
  if constexpr (V == 4) {
    q = co_u4{(uint32_t)e[0], (uint32_t)e[1], (uint32_t)e[2], (uint32_t)e[3]};
  } else {
    q = co_u4{(uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16), (uint32_t)e[4] | ((uint32_t)e[5] << 16),
              (uint32_t)e[6] | ((uint32_t)e[7] << 16)};
  }
  return q;
}

template <typename OutT>
__global__ __launch_bounds__(256) void collate_wave_kernel(const CoArgs a) {
  typedef CoOut<OutT> O;
  typedef typename O::Bits Bits;
  constexpr int V = 16 / (int)sizeof(Bits);   // elements per 16-byte group
  constexpr int kRounds = kCoTile / (V * 256);
  static_assert(kRounds * V * 256 == kCoTile, "tile size");
  const int tid = threadIdx.x;
  for (int64_t w = blockIdx.x; w < a.work_items; w += gridDim.x) {
    const int64_t r = w / a.tiles_per_row, t = w - r * a.tiles_per_row;  // (workgroup-uniform: scalar arithmetic)
    const CoRow row = co_uniform(a.rows + r);
    Bits* rowp = static_cast<Bits*>(a.out) + r * a.row_len;
    // positions p are counted from the 16-byte boundary at or below the row's first element: element e of the row is p = head + e
    const int64_t head = (int64_t)((reinterpret_cast<uintptr_t>(rowp) / sizeof(Bits)) & (uintptr_t)(V - 1));
    const int64_t row_end = head + a.row_len;                       // the row is [head, row_end)
    const int64_t s_lo = head + row.dst_off, s_hi = s_lo + row.len;  // its samples are [s_lo, s_hi): sample p is arena[src_off + p - s_lo]
    const int64_t p0 = t * kCoTile;
    if (p0 >= row_end) continue;
#pragma unroll
    for (int k = 0; k < kRounds; ++k) {
      const int64_t p = p0 + V * (tid + 256 * k);
      Bits e[V];
      if (p >= s_lo && p + V <= s_hi) {  // wholly samples
        const uint32_t* s = a.arena + (row.src_off + (p - s_lo));
#pragma unroll
        for (int j = 0; j < V; j += 4) {
          const co_u4 q = *reinterpret_cast<const co_u4_dword_aligned*>(s + j);
          e[j] = O::cvt(q.x), e[j + 1] = O::cvt(q.y), e[j + 2] = O::cvt(q.z), e[j + 3] = O::cvt(q.w);
        }
      } else if (p + V <= s_lo || p >= s_hi) {  // wholly padding
#pragma unroll
        for (int j = 0; j < V; ++j) e[j] = 0;
      } else {  // the first or the last sample cuts the group
#pragma unroll
        for (int j = 0; j < V; ++j) e[j] = (p + j >= s_lo && p + j < s_hi) ? O::cvt(a.arena[row.src_off + (p + j - s_lo)]) : (Bits)0;
      }
      if (p >= head && p + V <= row_end) {
        *reinterpret_cast<co_u4*>(rowp + (p - head)) = co_pack<O, V>(e);
      } else {  // the row's first or last element cuts the group (or the group lies outside the row)
#pragma unroll
        for (int j = 0; j < V; ++j)
          if (p + j >= head && p + j < row_end) rowp[p + j - head] = e[j];
      }
    }
  }
}

// ---- the sources form (collate_tables.hpp, build_collate_sources_plan): a row is the mean of its k sources ------------------------------
// Reference: the channel handling of collate_audio (lhotse/dataset/collation.py:215-241): audio.mean(dim=0) of a (C, T) cut, or the
// (B, C, T) tensor whose missing channels are zero rows.  The same tiles, the same four alignment cases and the same 16-byte loads as
// collate_wave_kernel; a group reads its V elements of EVERY source of the row (the channels of a row may sit at different residues
// mod 4: uniform per workgroup, the same instruction) into V float64 accumulators, sum from +0.0 in ascending source order,
// divides once in float64 and rounds once to float32; rows of k <= 1 take the bit path of collate_wave_kernel.  The source offsets
// are read through v_readfirstlane in a scalar loop over k.  No LDS, no atomics; every element of out is written exactly once.
struct CoMeanArgs {
  const uint32_t* arena;  // float32 samples, as bit patterns
  void* out;
  const CoRow* rows;    // device
  const int64_t* srcs;  // device: the source offsets of all rows, row r at [first, first + k) of CoRow.pad
  int64_t row_len, tiles_per_row, work_items;
};

__device__ __forceinline__ int64_t co_uniform_i64(const int64_t* p) {
  const int* w = reinterpret_cast<const int*>(p);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane(w[0]), hi = (uint32_t)__builtin_amdgcn_readfirstlane(w[1]);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <typename OutT>
__global__ __launch_bounds__(256) void collate_mean_kernel(const CoMeanArgs a) {
  typedef CoOut<OutT> O;
  typedef typename O::Bits Bits;
  constexpr int V = 16 / (int)sizeof(Bits);   // elements per 16-byte group
  constexpr int kRounds = kCoTile / (V * 256);
  static_assert(kRounds * V * 256 == kCoTile, "tile size");
  const int tid = threadIdx.x;
  for (int64_t w = blockIdx.x; w < a.work_items; w += gridDim.x) {
    const int64_t r = w / a.tiles_per_row, t = w - r * a.tiles_per_row;  // (workgroup-uniform: scalar arithmetic)
    const CoRow row = co_uniform(a.rows + r);
    const int nsrc = co_num_sources(row.pad);
    const int64_t* srcs = a.srcs + co_first_source(row.pad);
    const double count = (double)nsrc;
    Bits* rowp = static_cast<Bits*>(a.out) + r * a.row_len;
    const int64_t head = (int64_t)((reinterpret_cast<uintptr_t>(rowp) / sizeof(Bits)) & (uintptr_t)(V - 1));
    const int64_t row_end = head + a.row_len;                       // the row is [head, row_end)
    const int64_t s_lo = head + row.dst_off, s_hi = s_lo + row.len;  // its samples are [s_lo, s_hi): sample p is source[p - s_lo]
    const int64_t p0 = t * kCoTile;
    if (p0 >= row_end) continue;
    for (int k = 0; k < kRounds; ++k) {
      const int64_t p = p0 + V * (tid + 256 * k);
      const bool whole = p >= s_lo && p + V <= s_hi;
      Bits e[V];
      if (p + V <= s_lo || p >= s_hi) {  // wholly padding (every group of a row without sources)
#pragma unroll
        for (int j = 0; j < V; ++j) e[j] = 0;
      } else if (nsrc <= 1) {  // one source: the samples travel as bit patterns
        const uint32_t* s = a.arena + (row.src_off + (p - s_lo));
        if (whole) {
#pragma unroll
          for (int j = 0; j < V; j += 4) {
            const co_u4 q = *reinterpret_cast<const co_u4_dword_aligned*>(s + j);
            e[j] = O::cvt(q.x), e[j + 1] = O::cvt(q.y), e[j + 2] = O::cvt(q.z), e[j + 3] = O::cvt(q.w);
          }
        } else {  // the first or the last sample cuts the group
#pragma unroll
          for (int j = 0; j < V; ++j) e[j] = (p + j >= s_lo && p + j < s_hi) ? O::cvt(s[j]) : (Bits)0;
        }
      } else {
        double acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.0;
        for (int c = 0; c < nsrc; ++c) {  // (scalar loop: nsrc and the offsets are workgroup-uniform)
          const uint32_t* s = a.arena + (co_uniform_i64(srcs + c) + (p - s_lo));
          uint32_t x[V];
          if (whole) {
#pragma unroll
            for (int j = 0; j < V; j += 4) {
              const co_u4 q = *reinterpret_cast<const co_u4_dword_aligned*>(s + j);
              x[j] = q.x, x[j + 1] = q.y, x[j + 2] = q.z, x[j + 3] = q.w;
            }
          } else {
#pragma unroll
            for (int j = 0; j < V; ++j) x[j] = (p + j >= s_lo && p + j < s_hi) ? s[j] : 0u;
          }
#pragma unroll
          for (int j = 0; j < V; ++j) acc[j] += (double)__builtin_bit_cast(float, x[j]);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
          float m = (float)(acc[j] / count);
          // the float32 mean is a value of its own: without this the compiler fuses double -> float -> binary16 into ONE rounding, which
          // is not .to(float16) of the float32 mean (no instruction is emitted for it)
          asm("" : "+v"(m));
          e[j] = (p + j >= s_lo && p + j < s_hi) ? O::cvt(__builtin_bit_cast(uint32_t, m)) : (Bits)0;
        }
      }
      if (p >= head && p + V <= row_end) {
        *reinterpret_cast<co_u4*>(rowp + (p - head)) = co_pack<O, V>(e);
      } else {  // the row's first or last element cuts the group (or the group lies outside the row)
#pragma unroll
        for (int j = 0; j < V; ++j)
          if (p + j >= head && p + j < row_end) rowp[p + j - head] = e[j];
      }
    }
  }
}

}  // namespace hipfeat
