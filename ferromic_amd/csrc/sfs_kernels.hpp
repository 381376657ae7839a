// sfs_kernels.hpp — site frequency spectra from the packed bit planes: the 1-D spectrum of one group per row window and the joint
// spectrum of two groups (sfs.hip; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.12).
//
// Read side: LPR lanes (4 or 16) own one row and walk the 16-byte vectors [vec_begin, vec_end) the groups have members in; per group the
// lanes count  alt = |p0 & called & mask|  and note whether  (p1 | p2) & called & mask  or  ~called & mask  has a bit, then fold the LPR
// partial results with shuffles.  row_gap / row_hi (one byte per row, may be null) spare the called / upper planes of the rows that have
// nothing there, as the PCA site scan does.
// Histogram side: a persistent grid walks a table of work items (row ranges that never straddle a window).  Per item the workgroup counts
// its rows into an LDS tile of u32 bins with LDS atomics and then adds the non-zero bins to the window's slice of the u64 table with 64-bit
// global atomics - integer adds, exact in any order.  The tile holds the keys whose every coordinate is near an end of its axis
// (min(k, n - k) < T); any other key goes to the table directly with one global atomic.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sweep_kernels.hpp"  // and128, popc128

namespace fmh {

struct SfsItem {
  unsigned long long row_begin;
  uint32_t rows;    // at most 2^30: an LDS bin cannot wrap
  uint32_t window;
};

// one axis of the table: sample size n, near-edge threshold T, LDS slots L = n + 1 (the whole axis) or 2 T (both ends)
struct SfsAxis {
  uint32_t n, T, L;
};

struct SfsArgs {
  const uint8_t *p0, *p1, *p2, *pc;  // planes (p1 / p2 / pc may be null)
  const uint8_t *row_gap, *row_hi;   // one byte per row or null (null = read the plane of every row)
  const uint8_t *mask0, *mask1;      // the groups' membership as one bit per column (mask1 unused by the 1-D kernel)
  size_t plane_pitch;
  uint32_t vec_begin, vec_end;       // the 16-byte vectors of a row that can hold a member
  SfsAxis ax0, ax1;                  // ax1 = {0, 1, 1} for the 1-D spectrum
  const SfsItem* items;
  uint32_t n_items;
  size_t bins;                       // (n0 + 1) * (n1 + 1): one window's slice
  unsigned long long* sfs;           // [n_windows][bins]
  unsigned long long* skipped;       // [n_windows][2] (multiallelic, incomplete) or null
};

constexpr uint32_t kSfsLdsHead = 4;  // dwords before the tile: the item's two skipped tallies, padded to 16 bytes

__device__ __forceinline__ int sfs_slot(const SfsAxis& ax, uint32_t k) {
  if (ax.L == ax.n + 1 || k < ax.T) return (int)k;
  const uint32_t back = ax.n - k;
  return back < ax.T ? (int)(ax.L - 1 - back) : -1;
}
__device__ __forceinline__ uint32_t sfs_key(const SfsAxis& ax, uint32_t slot) {
  if (ax.L == ax.n + 1 || slot < ax.T) return slot;
  return ax.n - (ax.L - 1 - slot);
}

__device__ __forceinline__ uint4 sfs_load16(const uint8_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ uint4 sfs_or128(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }
__device__ __forceinline__ uint4 sfs_andn128(uint4 a, uint4 b) { return make_uint4(a.x & ~b.x, a.y & ~b.y, a.z & ~b.z, a.w & ~b.w); }  // a & ~b
__device__ __forceinline__ uint32_t sfs_any128(uint4 a) { return (a.x | a.y | a.z | a.w) != 0 ? 1u : 0u; }

// Launched with 256 or 512 threads (sfs.hip picks the size that keeps eight waves per CU resident for the tile) and
// (kSfsLdsHead + L0 * L1) * 4 bytes of dynamic LDS.
template <int LPR, bool JOINT>
__global__ __launch_bounds__(512) void sfs_kernel(const SfsArgs A) {
  extern __shared__ uint32_t sfs_lds[];
  uint32_t* s_skip = sfs_lds;
  uint32_t* tile = sfs_lds + kSfsLdsHead;
  const uint32_t threads = blockDim.x, tid = threadIdx.x;
  const uint32_t sub = tid % LPR, slot_row = tid / LPR, rows_per_pass = threads / LPR;
  const uint32_t tile_bins = A.ax0.L * A.ax1.L;
  const uint32_t width1 = A.ax1.n + 1;

  for (uint32_t s = tid; s < tile_bins + kSfsLdsHead; s += threads) sfs_lds[s] = 0;
  __syncthreads();

  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const SfsItem item = A.items[it];
    unsigned long long* out = A.sfs + (size_t)item.window * A.bins;
    // every thread runs every pass (the shuffles below need whole waves); rows past the item count nothing
    for (uint32_t base = 0; base < item.rows; base += rows_per_pass) {
      const uint32_t r = base + slot_row;
      const bool live = r < item.rows;
      uint32_t alt0 = 0, alt1 = 0, flags0 = 0, flags1 = 0;  // flags: 1 = a called member above allele 1, 2 = an uncalled member
      if (live) {
        const size_t row = (size_t)item.row_begin + r;
        const bool read_called = A.pc && (!A.row_gap || A.row_gap[row] != 0);
        const bool read_high = (A.p1 || A.p2) && (!A.row_hi || A.row_hi[row] != 0);
        const size_t row_off = row * A.plane_pitch;
        for (uint32_t v = A.vec_begin + sub; v < A.vec_end; v += LPR) {
          const size_t at = row_off + (size_t)v * 16;
          const uint4 m0 = sfs_load16(A.mask0 + (size_t)v * 16);
          uint4 a = sfs_load16(A.p0 + at);
          uint4 called = make_uint4(~0u, ~0u, ~0u, ~0u);
          if (read_called) called = sfs_load16(A.pc + at);
          uint4 high = make_uint4(0, 0, 0, 0);
          if (read_high) {
            if (A.p1) high = sfs_load16(A.p1 + at);
            if (A.p2) high = sfs_or128(high, sfs_load16(A.p2 + at));
            high = and128(high, called);
          }
          a = and128(a, called);
          alt0 = popc128(and128(a, m0), alt0);
          flags0 |= sfs_any128(and128(high, m0)) | (sfs_any128(sfs_andn128(m0, called)) << 1);
          if constexpr (JOINT) {
            const uint4 m1 = sfs_load16(A.mask1 + (size_t)v * 16);
            alt1 = popc128(and128(a, m1), alt1);
            flags1 |= sfs_any128(and128(high, m1)) | (sfs_any128(sfs_andn128(m1, called)) << 1);
          }
        }
      }
      if constexpr (JOINT) flags0 |= flags1;  // a row is multiallelic / incomplete for the pair when it is so for either group
      // the LPR lanes of a row are consecutive lanes of one wave
#pragma unroll
      for (int o = LPR / 2; o > 0; o >>= 1) {
        alt0 += __shfl_xor(alt0, o);
        flags0 |= __shfl_xor(flags0, o);
        if constexpr (JOINT) alt1 += __shfl_xor(alt1, o);
      }
      if (live && sub == 0) {
        if (flags0 & 1u) atomicAdd(&s_skip[0], 1u);
        else if (flags0 & 2u) atomicAdd(&s_skip[1], 1u);
        else {
          const int s0 = sfs_slot(A.ax0, alt0);
          const int s1 = JOINT ? sfs_slot(A.ax1, alt1) : 0;
          if (s0 >= 0 && s1 >= 0) atomicAdd(&tile[(uint32_t)s0 * A.ax1.L + (uint32_t)s1], 1u);
          else atomicAdd(&out[(size_t)alt0 * width1 + alt1], 1ull);
        }
      }
    }
    __syncthreads();
    // flush and clear: the non-zero bins of the tile into the window's slice
    for (uint32_t s = tid; s < tile_bins; s += threads) {
      const uint32_t c = tile[s];
      if (c == 0) continue;
      tile[s] = 0;
      uint32_t k0, k1 = 0;
      if constexpr (JOINT) { k0 = sfs_key(A.ax0, s / A.ax1.L); k1 = sfs_key(A.ax1, s % A.ax1.L); }
      else k0 = sfs_key(A.ax0, s);
      atomicAdd(&out[(size_t)k0 * width1 + k1], (unsigned long long)c);
    }
    if (tid < 2) {
      const uint32_t c = s_skip[tid];
      if (c != 0) {
        s_skip[tid] = 0;
        if (A.skipped) atomicAdd(&A.skipped[(size_t)item.window * 2 + tid], (unsigned long long)c);
      }
    }
    __syncthreads();
  }
}

}  // namespace fmh
