// grm_kernels.hpp — device side of the genomic relationship matrix (grm.hip; definition in include/ferromic_hip.h, scheme in DESIGN.md
// section 3.24): the 2-bit genotype codes of the usable rows as a sample-major bit image, the f64 matrix-core Gram of the per-site values
// those codes choose, and the addition of the finished products into the caller's matrix.
//
// Codes (grm_codes_kernel, in geno_codes.hpp since admix.hip reads the same image).  code[plane][w][sample]: one u64 per (word w of 64 listed rows, selected sample at its list position), two planes,
// the sample fastest and padded to kPcaTile, w padded to kPcaStageWords.  Code of a genotype = bit of plane 0 + 2 * bit of plane 1:
// 0 hom-ref, 1 het, 2 hom-alt, 3 not called.  The fetch is the segment statistics' (segment_kernels.hpp: plane_fetch, PlaneFields, the
// per-row plane flags, the rank table): an item = (word, group of 256 matrix samples), 16 bytes per thread and plane, the 2-bit fields parked
// in LDS, a lane then gathers ITS sample's bit of the 64 rows.  Rows past the list read as not called; the words of the padding samples and of
// the padding words are whatever the host left there (zero): their products are never stored, and the padding rows carry z = (0, 0, 0).
//
// Gram (grm_gram_kernel).  S = Z Z^T, Z[i][k] = {z0_k, z1_k, z2_k, 0}[code(i, k)].  Tiling, staging and stores are pca_gram_kernel's: a
// workgroup of four waves owns one 128 x 128 tile on or above the diagonal and one K split, a wave 64 x 64 of it as 4 x 4
// v_mfma_f64_16x16x4_f64 accumulators; the per-site values are staged 256 sites at a time in LDS, double-buffered; the tile leaves with its
// mirror or goes to the split's slab for pca_slab_reduce_kernel.  What differs:
//   * the operand is chosen among three staged values and zero by two bits.  It is built with bit-field inserts on the 32-bit halves of the
//     doubles: L, H = the two code bits spread over a register (one signed bit-field extract each), then per half
//     bfi(L, bfi(H, 0, z1), bfi(H, z2, z0)): 8 VALU instructions per operand, 64 per 16 MFMAs;
//   * a lane holds 2 planes x 8 samples of bit words.  They are held as 32-bit halves: the low halves serve sites 0 .. 31 of a word, the high
//     halves sites 32 .. 63, and the NEXT word's low halves are fetched into the registers of the low halves as soon as site 31 is done (the
//     high halves likewise at the word's end) - the prefetch of pca_gram_kernel at half a word's distance, in 32 registers instead of 64.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "geno_codes.hpp"  // grm_codes_kernel, shared with admix.hip
#include "pca_kernels.hpp"
#include "plane_rows.hpp"
#include "segment_kernels.hpp"

namespace fmh {

// ---- Gram ---------------------------------------------------------------------------------------------------------------------------------
struct alignas(32) GrmSiteValues { double z0, z1, z2, pad; };  // the values of one site; pad keeps a site one 32-byte LDS slot
static_assert(sizeof(GrmSiteValues) == 32, "a site is 32 bytes");

// {z0, z1, z2, 0}[code], code = (bit `off` of lo) + 2 * (bit `off` of hi), on the halves of the doubles
__device__ __forceinline__ double grm_operand(uint32_t lo, uint32_t hi, uint32_t off, const uint32_t (&z)[6]) {
  const uint32_t L = (uint32_t)__builtin_amdgcn_sbfe((int)lo, off, 1u), H = (uint32_t)__builtin_amdgcn_sbfe((int)hi, off, 1u);
  uint32_t r[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t odd = ~H & z[2 + h];                      // code 1 or 3
    const uint32_t even = (H & z[4 + h]) | (~H & z[h]);      // code 0 or 2
    r[h] = (L & odd) | (~L & even);
  }
  return __hiloint2double((int)r[1], (int)r[0]);
}

// 32 sites of a word: 8 steps of 4 sites.  `sv` = the staged values of the first site of the half that lane group kq takes.
__device__ __forceinline__ void grm_half_word(const double4* sv, const uint32_t (&a_lo)[4], const uint32_t (&a_hi)[4], const uint32_t (&b_lo)[4],
                                              const uint32_t (&b_hi)[4], uint32_t kq, pca_f64x4 (&acc)[4][4]) {
#pragma unroll
  for (int step = 0; step < 8; ++step) {
    const double* site = reinterpret_cast<const double*>(sv + step * 4);  // (z0, z1, z2, pad) of site step * 4 + kq of the half
    const double2 z01 = *reinterpret_cast<const double2*>(site);
    const double z2 = site[2];
    const uint32_t z[6] = {(uint32_t)__double2loint(z01.x), (uint32_t)__double2hiint(z01.x), (uint32_t)__double2loint(z01.y),
                           (uint32_t)__double2hiint(z01.y), (uint32_t)__double2loint(z2), (uint32_t)__double2hiint(z2)};
    const uint32_t off = kq + 4u * step;
    double oa[4], ob[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      oa[a] = grm_operand(a_lo[a], a_hi[a], off, z);
      ob[a] = grm_operand(b_lo[a], b_hi[a], off, z);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(oa[a], ob[b], acc[a][b], 0, 0, 0);
  }
}

// grid (tiles, splits); words [split * words_per_split, ...) of the K range, words_per_split a multiple of kPcaStageWords.
// slabs == null: the tile goes to `gram` with its mirror (WRITTEN); otherwise to slabs[split][tile][128][128] for pca_slab_reduce_kernel.
// code32 = the image as 32-bit halves: half h of word w, sample s of plane p at ((p * kwords + w) * n_pad + s) * 2 + h.
__global__ __launch_bounds__(256, 2) void grm_gram_kernel(const uint32_t* __restrict__ code32, const GrmSiteValues* __restrict__ vals, uint32_t n_pad,
                                                       uint32_t kwords, uint32_t nt, uint32_t words_per_split, uint32_t n, double* __restrict__ gram,
                                                       double* __restrict__ slabs) {
  __shared__ double4 s_vals[2][kPcaStageSites];  // a site's GrmSiteValues, moved as one 32-byte vector
  const double4* vals4 = reinterpret_cast<const double4*>(vals);
  const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t ti, tj;
  pca_tile_of(blockIdx.x, nt, &ti, &tj);
  const uint32_t row0 = ti * kPcaTile + (wave >> 1) * kPcaWaveTile, col0 = tj * kPcaTile + (wave & 1) * kPcaWaveTile;
  // the lower-left wave block of a diagonal tile is the mirror of the upper-right one: it stages and waits, but computes nothing
  const bool active = row0 <= col0;
  const uint32_t w_begin = blockIdx.y * words_per_split;
  const uint32_t w_end = min(kwords, w_begin + words_per_split);
  const unsigned kq = lane >> 4, r16 = lane & 15;

  pca_f64x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = pca_f64x4{0.0, 0.0, 0.0, 0.0};

  const size_t plane = (size_t)kwords * n_pad * 2;  // 32-bit halves of a plane
  const uint32_t* pa = code32 + (size_t)(row0 + r16) * 2;
  const uint32_t* pb = code32 + (size_t)(col0 + r16) * 2;
  // the bits in flight: the low halves (sites 0 .. 31 of a word) and the high halves (sites 32 .. 63), [plane 0 | plane 1] x 4 samples a side
  uint32_t al[2][4] = {}, ah[2][4] = {}, bl[2][4] = {}, bh[2][4] = {};
  auto fetch = [&](uint32_t w, uint32_t half, uint32_t (&a)[2][4], uint32_t (&b)[2][4]) {
    const size_t at = (size_t)w * n_pad * 2 + half;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) { a[p][q] = pa[p * plane + at + q * 32]; b[p][q] = pb[p * plane + at + q * 32]; }
  };
  if (active && w_begin < w_end) { fetch(w_begin, 0, al, bl); fetch(w_begin, 1, ah, bh); }
  if (w_begin < w_end) s_vals[0][tid] = vals4[(size_t)w_begin * 64 + tid];
  __syncthreads();
  int buf = 0;
  for (uint32_t ws = w_begin; ws < w_end; ws += kPcaStageWords, buf ^= 1) {
    // the next stage's values travel in registers under this stage's MFMAs and reach LDS just before the barrier
    const bool more = ws + kPcaStageWords < w_end;
    double4 next_vals = make_double4(0.0, 0.0, 0.0, 0.0);
    if (more) next_vals = vals4[(size_t)(ws + kPcaStageWords) * 64 + tid];
    if (active) {
#pragma unroll 1
      for (int wi = 0; wi < kPcaStageWords; ++wi) {
        const uint32_t w = ws + wi;
        const bool next = w + 1 < w_end;
        grm_half_word(&s_vals[buf][wi * 64 + kq], al[0], al[1], bl[0], bl[1], kq, acc);
        if (next) fetch(w + 1, 0, al, bl);  // the low halves are done: the next word's take their registers
        grm_half_word(&s_vals[buf][wi * 64 + 32 + kq], ah[0], ah[1], bh[0], bh[1], kq, acc);
        if (next) fetch(w + 1, 1, ah, bh);
      }
    }
    if (more) s_vals[buf ^ 1][tid] = next_vals;  // last read in the stage before this one, which the previous barrier closed
    __syncthreads();
  }
  if (!active) return;
  if (slabs) {
    double* tile = slabs + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kPcaTile * kPcaTile);
    const uint32_t lr0 = (wave >> 1) * kPcaWaveTile, lc0 = (wave & 1) * kPcaWaveTile;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) tile[(size_t)(lr0 + a * 16 + kq + 4 * reg) * kPcaTile + lc0 + b * 16 + r16] = acc[a][b][reg];
    return;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) pca_store_entry(gram, n, row0 + a * 16 + kq + 4 * reg, col0 + b * 16 + r16, acc[a][b][reg]);
}

// S += the call's products: one thread per entry (both triangles of `products` hold the same bits, so S stays symmetric bit for bit)
__global__ __launch_bounds__(256) void grm_accumulate_kernel(const double* __restrict__ products, size_t total, double* __restrict__ S) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < total) S[e] += products[e];
}

}  // namespace fmh
