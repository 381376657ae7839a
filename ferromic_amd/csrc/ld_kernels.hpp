// ld_kernels.hpp — linkage disequilibrium between nearby sites from the packed bit planes: the haplotype counts of a site pair are
// popcounts of the AND of two rows (site x site over haplotypes - the transpose of what the sweeps and the Gram kernels count).
// Pairs are addressed as (i, d), partner j = i + d, 1 <= d <= band; DESIGN.md section 3.11 has the definition and the tiling.
//
// One 256-thread workgroup owns 64 rows x 64 values of d.  Per K slab it stages the 64 i-rows and the 127 partner rows
// i0 + d0 .. i0 + d0 + 126 into LDS as A = (p0 | p1 | p2) & called & mask (and C = called & mask when calls can be missing); the row
// stride is the slab plus one 16-byte slot, an odd number of slots, so that the ds_read_b128 of 16 consecutive rows touch 16 different
// slots.  Thread (ti, td) of the 16 x 16 grid owns rows ti + 16 a and offsets td + 16 b (a, b < 4): per 16 bytes of K it reads 4 i-row and
// 7 partner fragments (the partner of (a, b) is staged row ti + td + 16 (a + b)) and runs 64 and + popcount pairs (4 x that when MISSING).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sweep_kernels.hpp"  // bcnt_add, and128, popc128

namespace fmh {

constexpr int kLdRows = 64;                         // i rows of a tile
constexpr int kLdBand = 64;                         // values of d of a tile
constexpr int kLdPartners = kLdRows + kLdBand - 1;  // partner rows a tile can reach
constexpr int kLdStaged = kLdRows + kLdPartners;    // rows in LDS

struct LdArgs {
  const uint8_t *p0, *p1, *p2, *pc;  // planes (p1 / p2 / pc may be null)
  const uint8_t* mask;               // the group's membership as one bit per column, or null = every column
  size_t plane_pitch;
  uint32_t vec_begin, vec_end;       // the 16-byte vectors of a row that can hold a member
  uint32_t n_const;                  // MISSING = false: |C|, the same for every row
  uint32_t d_tiles;                  // tiles along d; blockIdx.x = row tile * d_tiles + d tile
  size_t row_begin, row_end;         // rows asked for
  size_t partner_end;                // partners j < partner_end
  size_t band;
  size_t over_words;                 // ceil(band / 32)
  double threshold;
  double* r2;                        // [row_count][band] or null
  uint32_t* n_ab;
  uint32_t* n_joint;
  uint32_t* over;                    // [row_count][over_words] or null
  uint32_t* site_n;                  // [row_count] or null
  uint32_t* site_alt;
};

// r^2 of one pair from its four counts; the integer products are exact in 64 bits and below 2^53, so the value has three roundings
// (two products, one quotient; the library is built with -ffp-contract=off)
__device__ __forceinline__ double ld_r2_from_counts(uint32_t n, uint32_t nA, uint32_t nB, uint32_t nAB) {
  const long long vA = (long long)nA * (long long)(n - nA), vB = (long long)nB * (long long)(n - nB);
  if (vA == 0 || vB == 0) return __longlong_as_double(0x7ff8000000000000ll);
  const long long D = (long long)n * (long long)nAB - (long long)nA * (long long)nB;
  const double num = (double)D * (double)D;
  const double den = (double)vA * (double)vB;
  return num / den;
}

template <bool MISSING>
__global__ __launch_bounds__(256) void ld_band_kernel(const LdArgs A) {
  constexpr int KS = MISSING ? 128 : 256;  // K bytes of a row per slab
  constexpr int STRIDE = KS + 16;          // 9 / 17 slots of 16 bytes: odd
  constexpr int VPR = KS / 16;             // lanes that stage one row
  constexpr int RPP = 256 / VPR;           // rows per staging pass
  constexpr int PASSES = (kLdStaged + RPP - 1) / RPP;
  __shared__ __attribute__((aligned(16))) uint8_t sA[kLdStaged * STRIDE];
  __shared__ __attribute__((aligned(16))) uint8_t sC[MISSING ? kLdStaged * STRIDE : 16];
  __shared__ uint32_t s_alt[kLdStaged], s_n[kLdStaged];  // |A| and |C| of every staged row over the K window

  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t td = tid & 15, ti = tid >> 4;
  const uint32_t d_tile = blockIdx.x % A.d_tiles;
  const size_t i0 = A.row_begin + (size_t)(blockIdx.x / A.d_tiles) * kLdRows;
  const size_t e0 = (size_t)d_tile * kLdBand;  // e = d - 1
  const size_t j0 = i0 + e0 + 1;               // first partner row of the tile
  // no partner inside the range: nothing to count, the epilogue writes the tile's NaN / 0 entries (the first d tile still counts its rows)
  const bool counts_needed = d_tile == 0 || j0 < A.partner_end;

  uint32_t acc[4][4], acc_n[MISSING ? 4 : 1][MISSING ? 4 : 1], acc_a[MISSING ? 4 : 1][MISSING ? 4 : 1], acc_b[MISSING ? 4 : 1][MISSING ? 4 : 1];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      acc[a][b] = 0;
      if constexpr (MISSING) { acc_n[a][b] = 0; acc_a[a][b] = 0; acc_b[a][b] = 0; }
    }
  uint32_t cnt_alt[PASSES], cnt_n[PASSES];
#pragma unroll
  for (int q = 0; q < PASSES; ++q) { cnt_alt[q] = 0; cnt_n[q] = 0; }

  if (counts_needed) {
    const uint32_t sv = tid % VPR, sr = tid / VPR;
    const size_t k_end = (size_t)A.vec_end * 16;
    for (size_t k0 = (size_t)A.vec_begin * 16; k0 < k_end; k0 += KS) {
      __syncthreads();  // the previous slab has been read
      const size_t off = k0 + (size_t)sv * 16;
      uint4 mk = make_uint4(~0u, ~0u, ~0u, ~0u);
      if (A.mask && off < k_end) mk = *reinterpret_cast<const uint4*>(A.mask + off);
#pragma unroll
      for (int q = 0; q < PASSES; ++q) {
        const uint32_t s = (uint32_t)q * RPP + sr;
        const size_t row = s < (uint32_t)kLdRows ? i0 + s : j0 + (s - kLdRows);
        const size_t limit = s < (uint32_t)kLdRows ? A.row_end : A.partner_end;
        uint4 va = make_uint4(0, 0, 0, 0), vc = make_uint4(0, 0, 0, 0);
        if (s < (uint32_t)kLdStaged && row < limit && off < k_end) {
          const size_t at = row * A.plane_pitch + off;
          va = *reinterpret_cast<const uint4*>(A.p0 + at);
          if (A.p1) { const uint4 t = *reinterpret_cast<const uint4*>(A.p1 + at); va.x |= t.x; va.y |= t.y; va.z |= t.z; va.w |= t.w; }
          if (A.p2) { const uint4 t = *reinterpret_cast<const uint4*>(A.p2 + at); va.x |= t.x; va.y |= t.y; va.z |= t.z; va.w |= t.w; }
          vc = mk;
          if constexpr (MISSING) vc = and128(vc, *reinterpret_cast<const uint4*>(A.pc + at));
          va = and128(va, vc);
        }
        if (s < (uint32_t)kLdStaged) {
          *reinterpret_cast<uint4*>(sA + s * STRIDE + sv * 16) = va;
          if constexpr (MISSING) *reinterpret_cast<uint4*>(sC + s * STRIDE + sv * 16) = vc;
        }
        cnt_alt[q] = popc128(va, cnt_alt[q]);
        if constexpr (MISSING) cnt_n[q] = popc128(vc, cnt_n[q]);
      }
      __syncthreads();
      const uint8_t* pi = sA + ti * STRIDE;
      const uint8_t* pj = sA + (kLdRows + ti + td) * STRIDE;
      const uint8_t* ci = sC + ti * STRIDE;
      const uint8_t* cj = sC + (kLdRows + ti + td) * STRIDE;
#pragma unroll 2
      for (int kk = 0; kk < VPR; ++kk) {
        uint4 ai[4], aj[7];
#pragma unroll
        for (int a = 0; a < 4; ++a) ai[a] = *reinterpret_cast<const uint4*>(pi + a * 16 * STRIDE + kk * 16);
#pragma unroll
        for (int c = 0; c < 7; ++c) aj[c] = *reinterpret_cast<const uint4*>(pj + c * 16 * STRIDE + kk * 16);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = popc128(and128(ai[a], aj[a + b]), acc[a][b]);
        if constexpr (MISSING) {
          uint4 xi[4], xj[7];
#pragma unroll
          for (int a = 0; a < 4; ++a) xi[a] = *reinterpret_cast<const uint4*>(ci + a * 16 * STRIDE + kk * 16);
#pragma unroll
          for (int c = 0; c < 7; ++c) xj[c] = *reinterpret_cast<const uint4*>(cj + c * 16 * STRIDE + kk * 16);
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              acc_n[a][b] = popc128(and128(xi[a], xj[a + b]), acc_n[a][b]);
              acc_a[a][b] = popc128(and128(ai[a], xj[a + b]), acc_a[a][b]);
              acc_b[a][b] = popc128(and128(xi[a], aj[a + b]), acc_b[a][b]);
            }
        }
      }
    }
  }

  // row totals: the VPR lanes of a row are consecutive lanes of one wave
#pragma unroll
  for (int q = 0; q < PASSES; ++q) {
#pragma unroll
    for (int o = VPR / 2; o > 0; o >>= 1) {
      cnt_alt[q] += __shfl_xor(cnt_alt[q], o);
      if constexpr (MISSING) cnt_n[q] += __shfl_xor(cnt_n[q], o);
    }
    const uint32_t s = (uint32_t)q * RPP + tid / VPR;
    if (tid % VPR == 0 && s < (uint32_t)kLdStaged) { s_alt[s] = cnt_alt[q]; s_n[s] = MISSING ? cnt_n[q] : A.n_const; }
  }
  __syncthreads();

  if (d_tile == 0 && tid < (uint32_t)kLdRows && i0 + tid < A.row_end) {
    if (A.site_n) A.site_n[i0 + tid - A.row_begin] = s_n[tid];
    if (A.site_alt) A.site_alt[i0 + tid - A.row_begin] = s_alt[tid];
  }

  const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const size_t i = i0 + ti + 16 * a;
    const bool in_row = i < A.row_end;
    uint32_t word[2] = {0, 0};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const size_t e = e0 + td + 16 * b;
      const bool in_band = e < A.band;
      const bool valid = in_row && in_band && i + e + 1 < A.partner_end;
      uint32_t n = 0, nAB = 0;
      double r2 = nan;
      if (valid) {
        nAB = acc[a][b];
        uint32_t nA, nB;
        if constexpr (MISSING) { n = acc_n[a][b]; nA = acc_a[a][b]; nB = acc_b[a][b]; }
        else { n = A.n_const; nA = s_alt[ti + 16 * a]; nB = s_alt[kLdRows + ti + td + 16 * (a + b)]; }
        r2 = ld_r2_from_counts(n, nA, nB, nAB);
      }
      if (in_row && in_band) {
        const size_t at = (i - A.row_begin) * A.band + e;
        if (A.r2) A.r2[at] = r2;
        if (A.n_ab) A.n_ab[at] = nAB;
        if (A.n_joint) A.n_joint[at] = n;
      }
      // the 16 lanes of a row hold 16 consecutive values of d: a wave's ballot is four rows x 16 bits
      const unsigned long long bal = __ballot(valid && r2 > A.threshold);
      word[b >> 1] |= (uint32_t)((bal >> (16 * (lane >> 4))) & 0xffffull) << (16 * (b & 1));
    }
    // lane td = 0 writes the tile's first word of the row, td = 1 the second: whole words, padding bits zero
    const size_t w = e0 / 32 + td;
    if (A.over && in_row && td < 2 && w < A.over_words) A.over[(i - A.row_begin) * A.over_words + w] = td == 0 ? word[0] : word[1];
  }
}

}  // namespace fmh
