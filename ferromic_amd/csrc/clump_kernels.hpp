// clump_kernels.hpp — gfx950 kernels of LD clumping (clump.hip; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.23):
// genotype-dosage LD between a list of candidate rows and the rows of their position windows, every count an integer from the bit planes.
//
// Fields of a row (clump_fields), per 32-bit word of 16 samples: C = both bits of every called selected genotype (the called plane, the
// upper allele planes and the column mask folded in; row_gap / row_hi honoured), A = p0 & C (the alt-allele bits), and from A:
// SA = swap(A) (the two bits of every sample exchanged) and H = A & (A >> 1) on the even bits (hom-alt).  Then over jointly called samples
//   n = popc(C_i & C_j) / 2, sum_i = popc(A_i & C_j), sq_i = sum_i + 2 popc(H_i & C_j), cross = popc(A_i & A_j) + popc(SA_i & A_j).
//
// Tile kernel (clump_ld_kernel<MISSING>).  A 256-thread workgroup walks items on the persistent grid; an item is TC consecutive candidates x
// 64 consecutive participants (TC = 64 in the complete core, 32 in the MISSING core, whose pairs carry six accumulators).  Rows are gathered
// through the participant table; per K slab of four 16-byte vectors the workgroup stages the combined fields into LDS (row stride five
// vectors, so that the rows a 16-lane group reads lie in different 16-byte slots) and every thread counts an interleaved micro-tile of
// (TC / 16) x 4 pairs: candidates ti + 16 a, partners tj + 16 b.  The complete core counts the cross term only: n is the number of
// selected samples and the rows' sums come from clump_row_sums_kernel.  Epilogue: r^2 in f64 by THE formula, then a ballot of `inside the
// candidate's [lo, hi) && j != i && r^2 >= r2`; for a fixed b a wave's ballot holds 16 consecutive partner bits of four candidates, so the
// first lane of each 16-lane group assembles the candidate's 64-bit word and stores it whole: no zero fill, no atomics.
//
// Pair kernel (geno_ld_pairs_kernel): one wave per pair over the same fields and the same count routine; lane 0 writes the record.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ferromic_hip.h"
#include "plane_rows.hpp"

namespace fmh {

constexpr uint32_t kClumpThreads = 256;
constexpr uint32_t kClumpTileP = 64;    // participants of an item
constexpr uint32_t kClumpSlabVecs = 4;  // 16-byte vectors of a row per K slab
constexpr uint32_t kClumpStride = kClumpSlabVecs + 1;
constexpr uint32_t kClumpEven = 0x55555555u;
constexpr uint32_t clump_tile_candidates(bool missing) { return missing ? 32u : 64u; }
// the tile kernel's static LDS: the candidates' A and SA and the partners' A, in the MISSING core also C and H of both (and four one-vector stubs otherwise)
constexpr size_t clump_lds_bytes(bool missing) {
  return (missing ? 4 * clump_tile_candidates(true) + 3 * kClumpTileP : 2 * clump_tile_candidates(false) + kClumpTileP + 0) * kClumpStride * 16 + 4 * 16;
}

struct ClumpArgs : PlaneRows {  // the packed image first (plane_rows.hpp)
  size_t row_begin;
  const uint32_t* rows;     // [K] participant -> row of the range
  const uint32_t* mask;     // [plane_pitch / 4] both bits of every selected sample
  uint32_t vec0, vec1;      // the 16-byte vectors of a row the selected samples lie in
  const uint32_t* cand;     // [n_cand] candidate -> participant
  const uint32_t* lo;       // [n_cand] partner range of a candidate in participants
  const uint32_t* hi;
  uint32_t n_cand, K, n;
  const uint2* items;       // [n_items] (first candidate of the tile, partner tile)
  uint32_t n_items;
  const uint32_t* row_sum;  // [K] popc(A) and popc(H) of a participant: the complete core's sums
  const uint32_t* row_hom;
  double r2;
  unsigned long long* bits;  // [n_items][TC]: bit j of word c = candidate c of the item claims participant 64 * tile + j
};

struct ClumpPairArgs : PlaneRows {
  const uint32_t* mask;
  uint32_t vec0, vec1;
  const uint32_t* rows_a;  // [P] matrix rows
  const uint32_t* rows_b;
  uint32_t P;
  fmh_geno_ld_counts* counts;
};

struct ClumpFields { uint4 A, C; };

__device__ __forceinline__ uint32_t clump_swap(uint32_t a) { return ((a >> 1) & kClumpEven) | ((a & kClumpEven) << 1); }
__device__ __forceinline__ uint32_t clump_hom(uint32_t a) { return a & (a >> 1) & kClumpEven; }
__device__ __forceinline__ uint4 clump_swap4(uint4 a) { return make_uint4(clump_swap(a.x), clump_swap(a.y), clump_swap(a.z), clump_swap(a.w)); }
__device__ __forceinline__ uint4 clump_hom4(uint4 a) { return make_uint4(clump_hom(a.x), clump_hom(a.y), clump_hom(a.z), clump_hom(a.w)); }
__device__ __forceinline__ uint32_t clump_popc_and(uint4 a, uint4 b) { return __popc(a.x & b.x) + __popc(a.y & b.y) + __popc(a.z & b.z) + __popc(a.w & b.w); }
__device__ __forceinline__ uint32_t clump_popc4(uint4 a) { return __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w); }

// vector `vec` of matrix row `row`; `on` false = zeros (a row past the table, a vector past the selected samples)
__device__ __forceinline__ ClumpFields clump_fields(const PlaneRows& R, size_t row, uint32_t vec, const uint32_t* __restrict__ mask, bool on) {
  ClumpFields f;
  f.A = make_uint4(0u, 0u, 0u, 0u);
  f.C = f.A;
  if (!on) return f;
  const size_t off = row * R.plane_pitch + (size_t)vec * 16;
  const uint4 m = *reinterpret_cast<const uint4*>(mask + (size_t)vec * 4);
  const uint4 b = *reinterpret_cast<const uint4*>(R.p0 + off);
  uint4 c = m;
  if (R.pc && (!R.row_gap || R.row_gap[row] != 0)) {
    const uint4 pc = *reinterpret_cast<const uint4*>(R.pc + off);
    const uint32_t w[4] = {pc.x & (pc.x >> 1) & kClumpEven, pc.y & (pc.y >> 1) & kClumpEven, pc.z & (pc.z >> 1) & kClumpEven, pc.w & (pc.w >> 1) & kClumpEven};
    c = make_uint4(c.x & (w[0] * 3u), c.y & (w[1] * 3u), c.z & (w[2] * 3u), c.w & (w[3] * 3u));
  }
  if ((R.p1 || R.p2) && (!R.row_hi || R.row_hi[row] != 0)) {
    uint4 hi = make_uint4(0u, 0u, 0u, 0u);
    if (R.p1) hi = *reinterpret_cast<const uint4*>(R.p1 + off);
    if (R.p2) {
      const uint4 h2 = *reinterpret_cast<const uint4*>(R.p2 + off);
      hi = make_uint4(hi.x | h2.x, hi.y | h2.y, hi.z | h2.z, hi.w | h2.w);
    }
    const uint32_t w[4] = {(hi.x | (hi.x >> 1)) & kClumpEven, (hi.y | (hi.y >> 1)) & kClumpEven, (hi.z | (hi.z >> 1)) & kClumpEven, (hi.w | (hi.w >> 1)) & kClumpEven};
    c = make_uint4(c.x & ~(w[0] * 3u), c.y & ~(w[1] * 3u), c.z & ~(w[2] * 3u), c.w & ~(w[3] * 3u));
  }
  f.C = c;
  f.A = make_uint4(b.x & c.x, b.y & c.y, b.z & c.z, b.w & c.w);
  return f;
}

// The word-pair count routine both kernels share.  acc: the cross term, and in the MISSING core also popc(C_i & C_j), popc(A_i & C_j),
// popc(A_j & C_i), popc(H_i & C_j), popc(H_j & C_i).
template <bool MISSING>
__device__ __forceinline__ void clump_count_pair(uint4 a_i, uint4 sa_i, uint4 c_i, uint4 h_i, uint4 a_j, uint4 c_j, uint4 h_j, uint32_t* acc) {
  acc[0] += clump_popc_and(a_i, a_j) + clump_popc_and(sa_i, a_j);
  if (MISSING) {
    acc[1] += clump_popc_and(c_i, c_j);
    acc[2] += clump_popc_and(a_i, c_j);
    acc[3] += clump_popc_and(a_j, c_i);
    acc[4] += clump_popc_and(h_i, c_j);
    acc[5] += clump_popc_and(h_j, c_i);
  }
}
__device__ __forceinline__ fmh_geno_ld_counts clump_counts_of(const uint32_t* acc) {
  fmh_geno_ld_counts c;
  c.n = acc[1] >> 1; c.sum_a = acc[2]; c.sum_b = acc[3]; c.sq_a = acc[2] + 2u * acc[4]; c.sq_b = acc[3] + 2u * acc[5]; c.cross = acc[0];
  c.reserved[0] = c.reserved[1] = 0;
  return c;
}

// THE formula (clump_host.hpp: geno_ld_r2) and its threshold: NaN never qualifies
__device__ __forceinline__ bool clump_reaches(const fmh_geno_ld_counts& c, double threshold) {
  const long long n = c.n;
  const long long cov = n * (long long)c.cross - (long long)c.sum_a * (long long)c.sum_b;
  const long long va = n * (long long)c.sq_a - (long long)c.sum_a * (long long)c.sum_a;
  const long long vb = n * (long long)c.sq_b - (long long)c.sum_b * (long long)c.sum_b;
  if (va == 0 || vb == 0) return false;
  const double r2 = ((double)cov * (double)cov) / ((double)va * (double)vb);
  return r2 >= threshold;
}

// one wave per participant: popc(A) and popc(H) over the selected samples
static __global__ __launch_bounds__(kClumpThreads) void clump_row_sums_kernel(const ClumpArgs A, uint32_t* __restrict__ row_sum, uint32_t* __restrict__ row_hom) {
  const uint32_t lane = threadIdx.x & 63u;
  const size_t waves = (size_t)gridDim.x * (kClumpThreads / 64);
  for (size_t k = (size_t)blockIdx.x * (kClumpThreads / 64) + (threadIdx.x >> 6); k < A.K; k += waves) {
    const size_t row = A.row_begin + A.rows[k];
    uint32_t sum = 0, hom = 0;
    for (uint32_t vec = A.vec0 + lane; vec < A.vec1; vec += 64) {
      const ClumpFields f = clump_fields(A, row, vec, A.mask, true);
      sum += clump_popc4(f.A);
      hom += clump_popc4(clump_hom4(f.A));
    }
    for (uint32_t o = 32; o; o >>= 1) { sum += __shfl_xor(sum, o); hom += __shfl_xor(hom, o); }
    if (lane == 0) { row_sum[k] = sum; row_hom[k] = hom; }
  }
}

// Launched with kClumpThreads threads; static LDS: 15 KiB (complete), 25 KiB (MISSING).
template <bool MISSING>
static __global__ __launch_bounds__(kClumpThreads) void clump_ld_kernel(const ClumpArgs A) {
  constexpr uint32_t TC = clump_tile_candidates(MISSING), CI = TC / 16, NACC = MISSING ? 6 : 1;
  constexpr uint32_t EXTRA = MISSING ? 1 : 0;  // the C and H images exist in the MISSING core only
  __shared__ uint4 s_ca[TC * kClumpStride], s_cs[TC * kClumpStride];
  __shared__ uint4 s_cc[EXTRA * TC * kClumpStride + 1], s_ch[EXTRA * TC * kClumpStride + 1];
  __shared__ uint4 s_pa[kClumpTileP * kClumpStride];
  __shared__ uint4 s_pc[EXTRA * kClumpTileP * kClumpStride + 1], s_ph[EXTRA * kClumpTileP * kClumpStride + 1];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t srow = tid >> 2, spart = tid & 3u;  // the staging thread's row of the tile and vector of the slab
  const uint32_t ti = tid >> 4, tj = tid & 15u;      // the counting thread's candidates ti + 16 a and partners tj + 16 b
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);

  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const uint2 item = A.items[it];
    const uint32_t c0 = item.x, j0 = item.y * kClumpTileP;
    // the rows this thread stages: partner j0 + srow and (srow < TC) candidate c0 + srow
    const bool p_on = j0 + srow < A.K;
    const size_t p_row = A.row_begin + A.rows[p_on ? j0 + srow : 0];
    const bool c_on = srow < TC && c0 + srow < A.n_cand;
    const size_t c_row = A.row_begin + A.rows[c_on ? A.cand[c0 + srow] : 0];

    uint32_t acc[CI][4][NACC];
#pragma unroll
    for (uint32_t a = 0; a < CI; ++a)
#pragma unroll
      for (uint32_t b = 0; b < 4; ++b)
#pragma unroll
        for (uint32_t q = 0; q < NACC; ++q) acc[a][b][q] = 0;

    for (uint32_t v = A.vec0; v < A.vec1; v += kClumpSlabVecs) {
      const uint32_t vec = v + spart;
      const bool inside = vec < A.vec1;
      const ClumpFields fp = clump_fields(A, p_row, vec, A.mask, inside && p_on);
      const ClumpFields fc = clump_fields(A, c_row, vec, A.mask, inside && c_on);
      __syncthreads();  // every thread has counted the slab before this one
      s_pa[srow * kClumpStride + spart] = fp.A;
      if (MISSING) {
        s_pc[srow * kClumpStride + spart] = fp.C;
        s_ph[srow * kClumpStride + spart] = clump_hom4(fp.A);
      }
      if (srow < TC) {
        s_ca[srow * kClumpStride + spart] = fc.A;
        s_cs[srow * kClumpStride + spart] = clump_swap4(fc.A);
        if (MISSING) {
          s_cc[srow * kClumpStride + spart] = fc.C;
          s_ch[srow * kClumpStride + spart] = clump_hom4(fc.A);
        }
      }
      __syncthreads();
#pragma unroll
      for (uint32_t q = 0; q < kClumpSlabVecs; ++q) {
        uint4 pa[4], pc[4], ph[4];
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b) {
          pa[b] = s_pa[(tj + 16 * b) * kClumpStride + q];
          pc[b] = MISSING ? s_pc[(tj + 16 * b) * kClumpStride + q] : zero;
          ph[b] = MISSING ? s_ph[(tj + 16 * b) * kClumpStride + q] : zero;
        }
#pragma unroll
        for (uint32_t a = 0; a < CI; ++a) {
          const uint32_t at = (ti + 16 * a) * kClumpStride + q;
          const uint4 ca = s_ca[at], cs = s_cs[at];
          const uint4 cc = MISSING ? s_cc[at] : zero, ch = MISSING ? s_ch[at] : zero;
#pragma unroll
          for (uint32_t b = 0; b < 4; ++b) clump_count_pair<MISSING>(ca, cs, cc, ch, pa[b], pc[b], ph[b], acc[a][b]);
        }
      }
    }

    // ---- epilogue: r^2, the ballot, one whole 64-bit word per candidate ----
#pragma unroll
    for (uint32_t a = 0; a < CI; ++a) {
      const uint32_t c = c0 + ti + 16 * a;
      const bool c_in = c < A.n_cand;
      const uint32_t i = c_in ? A.cand[c] : 0u, lo = c_in ? A.lo[c] : 0u, hi = c_in ? A.hi[c] : 0u;
      uint32_t sum_i = 0, hom_i = 0;
      if (!MISSING && c_in) { sum_i = A.row_sum[i]; hom_i = A.row_hom[i]; }
      unsigned long long word = 0;
#pragma unroll
      for (uint32_t b = 0; b < 4; ++b) {
        const uint32_t j = j0 + tj + 16 * b;
        const bool in = c_in && j >= lo && j < hi && j != i;  // hi <= K: j is a participant
        bool reaches = false;
        if (in) {
          fmh_geno_ld_counts k;
          if (MISSING) k = clump_counts_of(acc[a][b]);
          else {
            const uint32_t sum_j = A.row_sum[j], hom_j = A.row_hom[j];
            k.n = A.n; k.sum_a = sum_i; k.sum_b = sum_j; k.sq_a = sum_i + 2u * hom_i; k.sq_b = sum_j + 2u * hom_j; k.cross = acc[a][b][0];
          }
          reaches = clump_reaches(k, A.r2);
        }
        const unsigned long long ballot = __ballot(reaches);  // lanes 16 g .. 16 g + 15: candidate ti = 4 wave + g, partners 16 b + (0 .. 15)
        word |= ((ballot >> (16u * (lane >> 4))) & 0xFFFFull) << (16u * b);
      }
      if (tj == 0) A.bits[(size_t)it * TC + ti + 16 * a] = word;
    }
  }
}

// one wave per pair, four pairs per workgroup and round of the grid
static __global__ __launch_bounds__(kClumpThreads) void geno_ld_pairs_kernel(const ClumpPairArgs A) {
  const uint32_t lane = threadIdx.x & 63u;
  const size_t waves = (size_t)gridDim.x * (kClumpThreads / 64);
  for (size_t p = (size_t)blockIdx.x * (kClumpThreads / 64) + (threadIdx.x >> 6); p < A.P; p += waves) {
    const size_t ra = A.rows_a[p], rb = A.rows_b[p];
    uint32_t acc[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t vec = A.vec0 + lane; vec < A.vec1; vec += 64) {
      const ClumpFields fa = clump_fields(A, ra, vec, A.mask, true), fb = clump_fields(A, rb, vec, A.mask, true);
      clump_count_pair<true>(fa.A, clump_swap4(fa.A), fa.C, clump_hom4(fa.A), fb.A, fb.C, clump_hom4(fb.A), acc);
    }
#pragma unroll
    for (uint32_t q = 0; q < 6; ++q)
      for (uint32_t o = 32; o; o >>= 1) acc[q] += __shfl_xor(acc[q], o);
    if (lane == 0) A.counts[p] = clump_counts_of(acc);
  }
}

}  // namespace fmh
