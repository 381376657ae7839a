// fstat_kernels.hpp — the moment blocks behind Patterson's f2 / f3 / f4 from the packed bit planes (fstat.hip; definition in
// include/ferromic_hip.h, scheme in DESIGN.md section 3.15): per block of rows the usable rows, the sums of up to 32 groups' allele counts
// and the sums of their pairwise products, all u64.
//
// Read side, as the spectra's (sfs_kernels.hpp): LPR lanes (4 or 16) own one row and walk the 16-byte vectors [vec_begin, vec_end) of the
// union of the groups; row_gap / row_hi spare the called / upper planes of the rows that have nothing there.  Every plane vector is loaded
// ONCE for all groups: the host lists, per vector, the (group, 16-byte mask) entries whose mask is non-zero there (CSR, sorted by vector), so
// disjoint populations cost about `vectors + groups` masked popcounts per row; a vector no group holds is not loaded at all.  The entries sit
// in LDS (LDS_MASKS) or are read from global memory - the same table either way.
// Per-row counts go to LDS with ds_add_u32, [rows of a pass][G + 1] (a register array indexed by group would spill); column G holds the
// constant 1, so that the usable-row count (1 x 1), the linear sums (a_g x 1) and the products (a_i x a_j) are one kind of slot.
// Product phase, per pass: a thread owns fixed slots of the block's slice - slot tid % M of the rows tid / M, tid / M + W, .. when M <= 256
// (W = 256 / M thread groups share the rows), slots tid, tid + 256, tid + 512 of every row otherwise - reads the two counts from LDS and
// accumulates (u64)a_i * a_j in registers across the whole work item; at the end of the item each non-zero accumulator goes to the block's
// slice with one 64-bit global atomic.  Integer adds, exact in any order.  No MFMA: counts need 17 bits and the sums 64.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plane_rows.hpp"
#include "sfs_kernels.hpp"  // sfs_load16, sfs_or128, sfs_andn128, sfs_any128; and128, popc128

namespace fmh {

constexpr int kFstatMaxGroups = 32;
constexpr uint32_t kFstatThreads = 256;
constexpr uint32_t kFstatMaxSlots = 1 + kFstatMaxGroups + kFstatMaxGroups * (kFstatMaxGroups + 1) / 2;                // 561
constexpr int kFstatSlotsPerThread = (int)((kFstatMaxSlots + kFstatThreads - 1) / kFstatThreads);                    // 3
constexpr uint32_t kFstatLdsHead = 4;  // dwords before the per-row state: the item's two skipped tallies, padded to 16 bytes

struct FstatItem {
  unsigned long long row_begin;
  uint32_t rows;
  uint32_t block;
};

struct FstatArgs : PlaneRows {  // the packed image first (plane_rows.hpp)
  uint32_t vec_begin, vec_end;       // the 16-byte vectors of a row that can hold a member of any group
  uint32_t n_groups;
  uint32_t n_entries;
  const uint32_t* ent_off;           // [vec_end - vec_begin + 1]: the entries of vector v are [ent_off[v - vec_begin], ent_off[v - vec_begin + 1])
  const uint32_t* ent_group;         // [n_entries]
  const uint4* ent_mask;             // [n_entries]: the group's membership bits in that vector
  const FstatItem* items;
  uint32_t n_items;
  uint32_t slots;                    // M = 1 + G + G (G + 1) / 2: one block's slice
  unsigned long long* moments;       // [n_blocks][M]
  unsigned long long* skipped;       // [n_blocks][2] (multiallelic, incomplete) or null
};

// dwords of LDS before the mask entries: head, flags [RPP], counts [RPP][G + 1], rounded up to 16 bytes
__host__ __device__ inline uint32_t fstat_lds_state_dwords(uint32_t rows_per_pass, uint32_t n_groups) {
  return (kFstatLdsHead + rows_per_pass + rows_per_pass * (n_groups + 1) + 3u) & ~3u;
}
// ... and with the entries behind them: masks (16 bytes each), groups, offsets
__host__ __device__ inline uint32_t fstat_lds_entry_dwords(uint32_t n_entries, uint32_t n_vectors) { return 5u * n_entries + n_vectors + 1u; }

// the two count columns of slot s (column G = the constant 1); s >= M maps to (G, G) and is never flushed
__device__ __forceinline__ void fstat_slot_columns(uint32_t s, uint32_t G, uint32_t M, uint32_t* ci, uint32_t* cj) {
  if (s == 0 || s >= M) { *ci = G; *cj = G; return; }
  if (s <= G) { *ci = s - 1; *cj = G; return; }
  uint32_t t = s - 1 - G, i = 0;
  while (t >= G - i) { t -= G - i; ++i; }
  *ci = i;
  *cj = i + t;
}

// Launched with kFstatThreads threads and (fstat_lds_state_dwords + [LDS_MASKS] fstat_lds_entry_dwords) * 4 bytes of dynamic LDS.
template <int LPR, bool LDS_MASKS>
__global__ __launch_bounds__(kFstatThreads) void fstat_kernel(const FstatArgs A) {
  extern __shared__ __attribute__((aligned(16))) uint32_t fstat_lds[];
  constexpr uint32_t RPP = kFstatThreads / LPR;  // rows of a pass
  const uint32_t G = A.n_groups, stride = G + 1, M = A.slots;
  const uint32_t n_vectors = A.vec_end - A.vec_begin;
  uint32_t* s_skip = fstat_lds;
  uint32_t* s_flags = fstat_lds + kFstatLdsHead;
  uint32_t* s_cnt = s_flags + RPP;
  const uint32_t state = fstat_lds_state_dwords(RPP, G);
  uint4* l_mask = reinterpret_cast<uint4*>(fstat_lds + state);
  uint32_t* l_group = fstat_lds + state + 4u * A.n_entries;
  uint32_t* l_off = l_group + A.n_entries;
  const uint32_t tid = threadIdx.x, sub = tid % LPR, slot_row = tid / LPR;

  if constexpr (LDS_MASKS) {
    for (uint32_t e = tid; e < A.n_entries; e += kFstatThreads) { l_mask[e] = A.ent_mask[e]; l_group[e] = A.ent_group[e]; }
    for (uint32_t i = tid; i <= n_vectors; i += kFstatThreads) l_off[i] = A.ent_off[i];
  }
  if (tid < kFstatLdsHead) s_skip[tid] = 0;
  if (tid < RPP) s_cnt[tid * stride + G] = 1;  // the constant column: written once, never cleared

  // the slots of this thread and the rows of a pass it takes them from
  const bool shared_rows = M <= kFstatThreads;
  const uint32_t row_groups = shared_rows ? kFstatThreads / M : 1;
  const uint32_t row_first = shared_rows ? tid / M : 0;
  const uint32_t slot0 = shared_rows ? tid % M : tid;
  const bool works = row_first < row_groups;
  uint32_t slot[kFstatSlotsPerThread], ci[kFstatSlotsPerThread], cj[kFstatSlotsPerThread];
#pragma unroll
  for (int k = 0; k < kFstatSlotsPerThread; ++k) {
    slot[k] = works ? slot0 + (uint32_t)k * kFstatThreads : M;
    fstat_slot_columns(slot[k], G, M, &ci[k], &cj[k]);
  }
  __syncthreads();

  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const FstatItem item = A.items[it];
    unsigned long long* out = A.moments + (size_t)item.block * M;
    unsigned long long acc[kFstatSlotsPerThread];
#pragma unroll
    for (int k = 0; k < kFstatSlotsPerThread; ++k) acc[k] = 0;

    for (uint32_t base = 0; base < item.rows; base += RPP) {
      // clear the row's counts and flags (the product phase of the pass before is behind a barrier)
      for (uint32_t c = sub; c < G; c += LPR) s_cnt[slot_row * stride + c] = 0;
      if (sub == 0) s_flags[slot_row] = 0;
      __syncthreads();

      // count: flags 1 = a called member above allele 1, 2 = an uncalled member
      const uint32_t r = base + slot_row;
      if (r < item.rows) {
        const size_t row = (size_t)item.row_begin + r;
        const bool read_called = A.pc && (!A.row_gap || A.row_gap[row] != 0);
        const bool read_high = (A.p1 || A.p2) && (!A.row_hi || A.row_hi[row] != 0);
        const size_t row_off = row * A.plane_pitch;
        uint32_t flags = 0;
        for (uint32_t v = A.vec_begin + sub; v < A.vec_end; v += LPR) {
          uint32_t e0, e1;
          if constexpr (LDS_MASKS) { e0 = l_off[v - A.vec_begin]; e1 = l_off[v - A.vec_begin + 1]; }
          else { e0 = A.ent_off[v - A.vec_begin]; e1 = A.ent_off[v - A.vec_begin + 1]; }
          if (e0 == e1) continue;  // nobody's vector: not read, its flaws do not count
          const size_t at = row_off + (size_t)v * 16;
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
          for (uint32_t e = e0; e < e1; ++e) {
            uint4 mk;
            uint32_t g;
            if constexpr (LDS_MASKS) { mk = l_mask[e]; g = l_group[e]; }
            else { mk = A.ent_mask[e]; g = A.ent_group[e]; }
            const uint32_t c = popc128(and128(a, mk), 0u);
            if (c != 0) atomicAdd(&s_cnt[slot_row * stride + g], c);
            flags |= sfs_any128(and128(high, mk)) | (sfs_any128(sfs_andn128(mk, called)) << 1);
          }
        }
        if (flags != 0) atomicOr(&s_flags[slot_row], flags);
      }
      __syncthreads();

      // products of the pass's usable rows
      const uint32_t live_rows = min(RPP, item.rows - base);
      if (works) {
        for (uint32_t q = row_first; q < live_rows; q += row_groups) {
          if (s_flags[q] != 0) continue;
          const uint32_t* c = s_cnt + q * stride;
#pragma unroll
          for (int k = 0; k < kFstatSlotsPerThread; ++k) acc[k] += (unsigned long long)c[ci[k]] * (unsigned long long)c[cj[k]];
        }
      }
      if (tid < live_rows) {
        const uint32_t f = s_flags[tid];
        if (f & 1u) atomicAdd(&s_skip[0], 1u);
        else if (f & 2u) atomicAdd(&s_skip[1], 1u);
      }
      __syncthreads();
    }

    // flush: every non-zero accumulator into the block's slice
#pragma unroll
    for (int k = 0; k < kFstatSlotsPerThread; ++k)
      if (slot[k] < M && acc[k] != 0) atomicAdd(&out[slot[k]], acc[k]);
    if (tid < 2) {
      const uint32_t c = s_skip[tid];
      if (c != 0) {
        s_skip[tid] = 0;
        if (A.skipped) atomicAdd(&A.skipped[(size_t)item.block * 2 + tid], (unsigned long long)c);
      }
    }
    // (the next item's first barrier stands between this clear of s_skip and its next add)
  }
}

}  // namespace fmh
