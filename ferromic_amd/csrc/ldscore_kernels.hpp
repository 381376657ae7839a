// ldscore_kernels.hpp — the gfx950 kernel of the LD scores (ldscore.hip; definition in include/ferromic_hip.h, scheme in DESIGN.md section
// 3.26): per kept row the fixed-point sum of genotype r^2 over the kept rows of its position window, the contraction over samples on
// v_mfma_i32_16x16x64_i8 with i32 accumulators.
//
// Items.  The participants are the kept rows, numbered ascending.  An item is a pair (I, J >= I) of 64-participant tiles in which some row of
// I has a partner in J; a 256-thread workgroup walks items on the persistent grid.  Wave w owns rows 16 w .. 16 w + 15 of I against all 64
// rows of J: four 16 x 16 MFMA tiles.
//
// Operands.  Both sides of the contraction are rows of the matrix, so ONE expansion serves both: the B operand of a 16-row tile has the lane
// map of the A operand of the same rows (lane l: row l & 15, the 16 K bytes of chunk l >> 4).  Per slab of two 16-byte vectors (128 samples)
// every thread reads one (row, vector) of the 128 rows of the two tiles through clump_fields - the called plane, the upper planes, the
// column mask and row_gap / row_hi folded in - widens its four words of 2-bit dosages to bytes (assoc_operand) and stores them to LDS, where
// all four waves read them: a J row is expanded once per workgroup and read by four waves, an I row once and read for four J tiles.  The
// next slab's plane words are fetched before the current slab's MFMAs.  LDS row stride: nine 16-byte slots, so that the 16 rows a quarter
// wave reads lie in different slots.
//
// Cores, each built with and without the correction.  ADJUST is a template argument and the lane's term counts are popcounts of one 16-bit
// mask: with `adjust` as a kernel argument and eight per-lane counters, hipcc of ROCm 7.2.0 (HIP 7.2.26015, AMD clang 22.0.0git roc-7.2.0
// 26014) left the column counter of the second J tile unset on the corrected path (deviation 4): re-check the
// operand-map test on the device after any change to the epilogue.   The complete core (no called plane, no upper planes) contracts g.g only: n is the number of selected samples and the rows' sums
// come from clump_row_sums_kernel.  The MISSING core stages g, c (called, 0 / 1) and s = g^2 (0 / 1 / 4), all zero where the genotype is not
// called, and runs six products per tile: g.g, g.c, c.g, c.c, s.c, c.s = cross, sum_a, sum_b, n, sq_a, sq_b over the jointly called samples.
//
// Epilogue.  C/D has column = lane & 15 (the J row) and row = 4 (lane >> 4) + register (the I row).  Per pair: the six integers, r^2 by THE
// formula, the correction, q - as ldscore_host.hpp - and the window test on the participants' positions.  q and the `counted` flag of a pair
// go to the I row and, in an off-diagonal item, to the J row as well (r^2 is symmetric bit for bit); a diagonal item holds every ordered pair
// of its tile once.  A wave reduces its rows over the 16 lanes of a quarter and its columns over the four quarters, then adds with 64-bit
// (Q) and 32-bit (counted) integer atomics into arrays the host zeroed: integer sums, the same bits in every order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ferromic_hip.h"
#include "assoc_kernels.hpp"
#include "clump_kernels.hpp"

namespace fmh {

constexpr uint32_t kLdScoreThreads = 256;
constexpr uint32_t kLdScoreTile = 64;      // participants of a tile: TM of both cores
constexpr uint32_t kLdScoreSlabVecs = 2;   // 16-byte vectors (64 samples each) of a row per slab
constexpr uint32_t kLdScoreStride = 4 * kLdScoreSlabVecs + 1;  // 16-byte slots of a staged row: 16 bytes per word of 16 samples
constexpr size_t ldscore_lds_bytes(bool missing) { return (size_t)(missing ? 3 : 1) * 2 * kLdScoreTile * kLdScoreStride * 16; }  // the complete core's two stubs are never read

struct LdScoreArgs : PlaneRows {  // the packed image first (plane_rows.hpp)
  size_t row_begin;
  const uint32_t* rows;     // [K] participant -> row of the range
  const uint32_t* x;        // [K] its position
  const uint32_t* mask;     // [plane_pitch / 4] both bits of every selected sample
  uint32_t vec0, vec1;      // the 16-byte vectors of a row the selected samples lie in
  uint32_t K, n, window;
  const uint2* items;       // [n_items] (tile I, tile J >= I)
  uint32_t n_items;
  const uint32_t* row_sum;  // [K] popc(A) and popc(H) of a participant: the complete core's sums
  const uint32_t* row_hom;
  unsigned long long* q;    // [K] zeroed by the host
  uint32_t* counted;        // [K] zeroed by the host
};

// the pair term (ldscore_host.hpp: ld_score_term): false = skipped
template <bool ADJUST> __device__ __forceinline__ bool ldscore_term(const fmh_geno_ld_counts& c, long long* q) {
  const long long n = c.n;
  const long long cov = n * (long long)c.cross - (long long)c.sum_a * (long long)c.sum_b;
  const long long va = n * (long long)c.sq_a - (long long)c.sum_a * (long long)c.sum_a;
  const long long vb = n * (long long)c.sq_b - (long long)c.sum_b * (long long)c.sum_b;
  if (va == 0 || vb == 0) return false;
  const double r2 = ((double)cov * (double)cov) / ((double)va * (double)vb);
  double t = r2;
  if constexpr (ADJUST) {
    if (n < 3) return false;
    t = r2 - (1.0 - r2) / (double)(n - 2);
  }
  *q = __double2ll_rn(t * 0x1p40);  // the power of two is exact: ldexp(t, 40); round half to even
  return true;
}

// Launched with kLdScoreThreads threads; static LDS: 18 KiB (complete), 54 KiB (MISSING).
template <bool MISSING, bool ADJUST>
static __global__ __launch_bounds__(kLdScoreThreads) void ldscore_kernel(const LdScoreArgs A) {
  constexpr uint32_t NP = MISSING ? 6 : 1, EXTRA = MISSING ? 1 : 0;
  constexpr uint32_t ROWS = 2 * kLdScoreTile;
  __shared__ uint4 s_g[ROWS * kLdScoreStride];
  __shared__ uint4 s_c[EXTRA * ROWS * kLdScoreStride + 1 - EXTRA], s_s[EXTRA * ROWS * kLdScoreStride + 1 - EXTRA];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t srow = tid >> 1, svec = tid & 1u;  // the staging thread's row of the 128 (I rows, then J rows) and vector of the slab
  const uint32_t orow = lane & 15u, chunk = lane >> 4;

  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const uint2 item = A.items[it];
    const uint32_t i0 = item.x * kLdScoreTile, j0 = item.y * kLdScoreTile;
    const bool diagonal = item.x == item.y;
    const uint32_t spart = srow < kLdScoreTile ? i0 + srow : j0 + (srow - kLdScoreTile);  // the participant this thread stages
    const bool s_on = spart < A.K;
    const size_t s_matrix_row = A.row_begin + A.rows[s_on ? spart : 0];

    assoc_v4i acc[NP][4];
#pragma unroll
    for (uint32_t p = 0; p < NP; ++p)
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t) acc[p][t] = assoc_v4i{0, 0, 0, 0};

    ClumpFields f = clump_fields(A, s_matrix_row, A.vec0 + svec, A.mask, s_on && A.vec0 + svec < A.vec1);
    for (uint32_t v = A.vec0; v < A.vec1; v += kLdScoreSlabVecs) {
      __syncthreads();  // every wave has read the slab before this one
      {
        const uint32_t a[4] = {f.A.x, f.A.y, f.A.z, f.A.w}, c[4] = {f.C.x, f.C.y, f.C.z, f.C.w};
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
          const uint32_t at = srow * kLdScoreStride + svec * 4u + w;
          const assoc_v4i g = assoc_operand((a[w] & kEvenBits) + ((a[w] >> 1) & kEvenBits));  // A is masked with C already
          s_g[at] = make_uint4((uint32_t)g[0], (uint32_t)g[1], (uint32_t)g[2], (uint32_t)g[3]);
          if constexpr (MISSING) {
            const assoc_v4i k = assoc_operand(c[w] & kEvenBits);
            s_c[at] = make_uint4((uint32_t)k[0], (uint32_t)k[1], (uint32_t)k[2], (uint32_t)k[3]);
            // g^2: 0, 1, 4 = g + (g & 2) per byte
            s_s[at] = make_uint4((uint32_t)g[0] + ((uint32_t)g[0] & 0x02020202u), (uint32_t)g[1] + ((uint32_t)g[1] & 0x02020202u),
                                 (uint32_t)g[2] + ((uint32_t)g[2] & 0x02020202u), (uint32_t)g[3] + ((uint32_t)g[3] & 0x02020202u));
          }
        }
      }
      __syncthreads();
      const uint32_t next = v + kLdScoreSlabVecs + svec;
      f = clump_fields(A, s_matrix_row, next, A.mask, s_on && next < A.vec1);  // in flight during the MFMAs
#pragma unroll
      for (uint32_t step = 0; step < kLdScoreSlabVecs; ++step) {
        const uint32_t ia = (16u * wave + orow) * kLdScoreStride + step * 4u + chunk;
        const uint4 ug = s_g[ia];
        const assoc_v4i ig = assoc_v4i{(int)ug.x, (int)ug.y, (int)ug.z, (int)ug.w};
        assoc_v4i ic = ig, is = ig;
        if constexpr (MISSING) {
          const uint4 uc = s_c[ia], us = s_s[ia];
          ic = assoc_v4i{(int)uc.x, (int)uc.y, (int)uc.z, (int)uc.w};
          is = assoc_v4i{(int)us.x, (int)us.y, (int)us.z, (int)us.w};
        }
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
          const uint32_t ja = (kLdScoreTile + 16u * t + orow) * kLdScoreStride + step * 4u + chunk;
          const uint4 vg = s_g[ja];
          const assoc_v4i jg = assoc_v4i{(int)vg.x, (int)vg.y, (int)vg.z, (int)vg.w};
          acc[0][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ig, jg, acc[0][t], 0, 0, 0);
          if constexpr (MISSING) {
            const uint4 vc = s_c[ja], vs = s_s[ja];
            const assoc_v4i jc = assoc_v4i{(int)vc.x, (int)vc.y, (int)vc.z, (int)vc.w};
            const assoc_v4i js = assoc_v4i{(int)vs.x, (int)vs.y, (int)vs.z, (int)vs.w};
            acc[1][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ig, jc, acc[1][t], 0, 0, 0);  // sum_a
            acc[2][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ic, jg, acc[2][t], 0, 0, 0);  // sum_b
            acc[3][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ic, jc, acc[3][t], 0, 0, 0);  // n
            acc[4][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(is, jc, acc[4][t], 0, 0, 0);  // sq_a
            acc[5][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ic, js, acc[5][t], 0, 0, 0);  // sq_b
          }
        }
      }
    }

    // ---- epilogue: the lane's pairs are I rows i0 + 16 wave + 4 chunk + r against J rows j0 + 16 t + orow ----
    long long row_q[4] = {0, 0, 0, 0}, col_q[4] = {0, 0, 0, 0};
    uint32_t used = 0;  // bit 4 r + t: the pair of register r and tile t has a term
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t i = i0 + 16u * wave + 4u * chunk + r;
      const bool i_in = i < A.K;
      const long long xi = i_in ? (long long)A.x[i] : 0;
      uint32_t sum_i = 0, hom_i = 0;
      if (!MISSING && i_in) { sum_i = A.row_sum[i]; hom_i = A.row_hom[i]; }
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t) {
        const uint32_t j = j0 + 16u * t + orow;
        if (!i_in || j >= A.K) continue;
        const long long gap = (long long)A.x[j] - xi;
        if ((gap < 0 ? -gap : gap) > (long long)A.window) continue;
        fmh_geno_ld_counts k;
        if constexpr (MISSING) {
          k.cross = (uint32_t)acc[0][t][r]; k.sum_a = (uint32_t)acc[1][t][r]; k.sum_b = (uint32_t)acc[2][t][r];
          k.n = (uint32_t)acc[3][t][r]; k.sq_a = (uint32_t)acc[4][t][r]; k.sq_b = (uint32_t)acc[5][t][r];
        } else {
          const uint32_t sum_j = A.row_sum[j], hom_j = A.row_hom[j];
          k.n = A.n; k.sum_a = sum_i; k.sum_b = sum_j; k.sq_a = sum_i + 2u * hom_i; k.sq_b = sum_j + 2u * hom_j; k.cross = (uint32_t)acc[0][t][r];
        }
        long long q = 0;
        if (!ldscore_term<ADJUST>(k, &q)) continue;
        row_q[r] += q;
        col_q[t] += q;
        used |= 1u << (4u * r + t);
      }
    }
    // rows: over the 16 lanes of the quarter wave
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      uint32_t row_n = __popc((used >> (4u * r)) & 0xFu);
      for (uint32_t o = 1; o < 16; o <<= 1) { row_q[r] += __shfl_xor(row_q[r], o); row_n += __shfl_xor(row_n, o); }
      const uint32_t i = i0 + 16u * wave + 4u * chunk + r;
      if (orow == 0 && i < A.K && row_n != 0) {
        atomicAdd(A.q + i, (unsigned long long)row_q[r]);
        atomicAdd(A.counted + i, row_n);
      }
    }
    // columns of an off-diagonal item: over the four quarters of the wave (the four waves add one after another)
    if (!diagonal) {
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t) {
        uint32_t col_n = __popc(used & (0x1111u << t));
        for (uint32_t o = 16; o < 64; o <<= 1) { col_q[t] += __shfl_xor(col_q[t], o); col_n += __shfl_xor(col_n, o); }
        const uint32_t j = j0 + 16u * t + orow;
        if (chunk == 0 && j < A.K && col_n != 0) {
          atomicAdd(A.q + j, (unsigned long long)col_q[t]);
          atomicAdd(A.counted + j, col_n);
        }
      }
    }
  }
}

}  // namespace fmh
