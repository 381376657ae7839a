// pca_kernels.hpp — device side of the haplotype PCA (pca.hip): the site scan, the gather + transpose of the kept sites into
// haplotype-major bit words, the f64 matrix-core Gram of the STANDARDISED matrix expanded from those bits, and the fixed-order
// reduction of the split-K partial tiles.  Reference: src/pca.rs (filter :205-413, fast_exact_pca_transform :541-803).
//
// Data flow of the Gram  G = Z Z^T / (n - 1),  Z[h][k] = bit(h, k) ? set_k : clear_k  (set_k = (1 - mean_k) / sd_k, clear_k = -mean_k / sd_k):
//   bitsT[w][h]   one u64 per (word w of 64 kept sites, haplotype h), h padded to kPcaTile, w padded to kPcaStageWords: 8 bytes per 64
//                 operands - Z itself (8 bytes per operand) is never materialised
//   vals[k]       (set_k, clear_k) per kept site, zero on the padding sites (a padding site contributes 0 * 0)
// A workgroup of four waves owns one kPcaTile x kPcaTile tile on or above the diagonal and one K split; a wave owns 64 x 64 of it as
// 4 x 4 v_mfma_f64_16x16x4_f64 accumulators (128 VGPRs).  Per 4 sites a wave expands 4 A and 4 B operands (a bit test and a two-register
// select each) and issues 16 MFMAs, so the expansion hides under the matrix pipe.  The f64 MFMA's register map (NOT that of the other shapes):
// A: lane l holds A[row l & 15][k = l >> 4]; B: lane l holds B[k = l >> 4][col l & 15]; C/D: col = l & 15, row = (l >> 4) + 4 * reg.
// (The kernels are static: grm_kernels.hpp takes the tile geometry, the mirror store and pca_slab_reduce_kernel from here, so two units
// include this header.)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace fmh {

constexpr int kPcaTile = 128;        // workgroup tile edge, haplotypes
constexpr int kPcaWaveTile = 64;     // wave tile edge
constexpr int kPcaStageWords = 4;    // 64-site words per LDS stage of (set, clear) pairs: 256 sites, 4 KiB
constexpr int kPcaStageSites = kPcaStageWords * 64;
constexpr uint8_t kPcaFlagUncalled = 1, kPcaFlagHighAllele = 2;  // fmh_pca_scan_sites' d_flags bits

typedef double pca_f64x4 __attribute__((ext_vector_type(4)));

__device__ inline unsigned long long pca_wave_sum(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ inline unsigned pca_wave_or(unsigned v) {
  for (int off = 32; off > 0; off >>= 1) v |= (unsigned)__shfl_xor((int)v, off, 64);
  return v;
}

// ---- site scan ------------------------------------------------------------------------------------------------------------------
// One wave per row.  alt = called entries whose allele is exactly 1; flags: kPcaFlagUncalled when a column is not called,
// kPcaFlagHighAllele when a called entry is above 1.  row_gap / row_hi (one byte per row, may be null) spare the called / high planes
// of the rows that have nothing there.
static __global__ __launch_bounds__(256) void pca_scan_packed_kernel(const uint8_t* __restrict__ p0, const uint8_t* __restrict__ p1, const uint8_t* __restrict__ p2,
                                                              const uint8_t* __restrict__ pc, const uint8_t* __restrict__ row_gap,
                                                              const uint8_t* __restrict__ row_hi, size_t plane_pitch, uint32_t columns, size_t row_begin,
                                                              size_t row_count, uint32_t* __restrict__ alt, uint8_t* __restrict__ flags) {
  const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= row_count) return;
  const unsigned lane = threadIdx.x & 63;
  const size_t row = row_begin + r;
  const bool read_called = pc && (!row_gap || row_gap[row] != 0);
  const bool read_high = (p1 || p2) && (!row_hi || row_hi[row] != 0);
  const uint32_t words = (columns + 63) / 64;  // plane_pitch is a multiple of 16 bytes: whole u64 words
  const unsigned long long* q0 = (const unsigned long long*)(p0 + row * plane_pitch);
  const unsigned long long* q1 = p1 ? (const unsigned long long*)(p1 + row * plane_pitch) : nullptr;
  const unsigned long long* q2 = p2 ? (const unsigned long long*)(p2 + row * plane_pitch) : nullptr;
  const unsigned long long* qc = pc ? (const unsigned long long*)(pc + row * plane_pitch) : nullptr;
  unsigned long long count = 0;
  unsigned f = 0;
  for (uint32_t w = lane; w < words; w += 64) {
    const uint32_t left = columns - w * 64;
    const unsigned long long valid = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    const unsigned long long called = read_called ? (qc[w] & valid) : valid;
    unsigned long long high = 0;
    if (read_high) high = ((q1 ? q1[w] : 0ull) | (q2 ? q2[w] : 0ull)) & called;
    if (called != valid) f |= kPcaFlagUncalled;
    if (high) f |= kPcaFlagHighAllele;
    count += (unsigned long long)__popcll(q0[w] & called & ~high);
  }
  count = pca_wave_sum(count);
  f = pca_wave_or(f);
  if (lane == 0) { alt[r] = (uint32_t)count; flags[r] = (uint8_t)f; }
}

static __global__ __launch_bounds__(256) void pca_scan_bytes_kernel(const uint8_t* __restrict__ data, size_t pitch, const uint8_t* __restrict__ bits,
                                                             size_t bits_pitch, uint32_t columns, size_t row_begin, size_t row_count,
                                                             uint32_t* __restrict__ alt, uint8_t* __restrict__ flags) {
  const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= row_count) return;
  const unsigned lane = threadIdx.x & 63;
  const size_t row = row_begin + r;
  const uint8_t* d = data + row * pitch;
  const uint8_t* b = bits ? bits + row * bits_pitch : nullptr;
  unsigned long long count = 0;
  unsigned f = 0;
  for (uint32_t c = lane; c < columns; c += 64) {
    const bool called = b ? ((b[c >> 3] >> (c & 7)) & 1) != 0 : true;
    const uint8_t v = d[c];
    if (!called) f |= kPcaFlagUncalled;
    else if (v > 1) f |= kPcaFlagHighAllele;
    else count += v;
  }
  count = pca_wave_sum(count);
  f = pca_wave_or(f);
  if (lane == 0) { alt[r] = (uint32_t)count; flags[r] = (uint8_t)f; }
}

// ---- gather + transpose ---------------------------------------------------------------------------------------------------------
// One wave per (64-site word w, block of 64 haplotypes hb): lane k reads the 64 haplotype bits of kept site w * 64 + k (zero beyond
// n_kept), the wave transposes the 64 x 64 bit block with ballots, lane j writes the word of haplotype hb * 64 + j.  Kept sites are
// biallelic with nothing missing, so plane 0 (or the low bit of a u8 entry) is the allele.
__device__ inline void pca_transpose_store(unsigned long long word, unsigned lane, unsigned long long* __restrict__ dst) {
  unsigned long long out = 0;
#pragma unroll 8
  for (int j = 0; j < 64; ++j) {
    const unsigned long long mask = __ballot((word >> j) & 1ull);
    if (lane == (unsigned)j) out = mask;
  }
  *dst = out;
}

static __global__ __launch_bounds__(256) void pca_transpose_packed_kernel(const uint8_t* __restrict__ p0, size_t plane_pitch, const unsigned long long* __restrict__ kept,
                                                                   size_t n_kept, uint32_t n_pad, unsigned long long* __restrict__ bitsT) {
  const unsigned lane = threadIdx.x & 63;
  const uint32_t hb = blockIdx.y * 4 + (threadIdx.x >> 6);  // n_pad is a multiple of 128: whole waves are in or out
  if (hb * 64 >= n_pad) return;
  const size_t w = blockIdx.x, s = w * 64 + lane;
  unsigned long long word = 0;
  if (s < n_kept && (size_t)hb * 8 + 8 <= plane_pitch) word = *(const unsigned long long*)(p0 + kept[s] * plane_pitch + (size_t)hb * 8);
  pca_transpose_store(word, lane, bitsT + w * n_pad + (size_t)hb * 64 + lane);
}

static __global__ __launch_bounds__(256) void pca_transpose_bytes_kernel(const uint8_t* __restrict__ data, size_t pitch, uint32_t columns,
                                                                  const unsigned long long* __restrict__ kept, size_t n_kept, uint32_t n_pad,
                                                                  unsigned long long* __restrict__ bitsT) {
  const unsigned lane = threadIdx.x & 63;
  const uint32_t hb = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (hb * 64 >= n_pad) return;
  const size_t w = blockIdx.x, s = w * 64 + lane;
  unsigned long long word = 0;
  if (s < n_kept) {
    const uint8_t* d = data + kept[s] * pitch;
    for (uint32_t j = 0; j < 64; ++j) {
      const uint32_t c = hb * 64 + j;
      if (c < columns) word |= (unsigned long long)(d[c] & 1) << j;
    }
  }
  pca_transpose_store(word, lane, bitsT + w * n_pad + (size_t)hb * 64 + lane);
}

// ---- Gram ---------------------------------------------------------------------------------------------------------------------
// Upper-triangular tile index t -> (ti <= tj) of an nt x nt tile grid, row by row.
__device__ inline void pca_tile_of(uint32_t t, uint32_t nt, uint32_t* ti, uint32_t* tj) {
  uint32_t i = 0, row_len = nt;
  while (t >= row_len) { t -= row_len; ++i; --row_len; }
  *ti = i;
  *tj = i + t;
}

// (row, col) of a tile's entry -> the output: an entry on or above the diagonal is written together with its mirror, one below (the
// lower halves of the diagonal wave blocks) not at all - so G == G^T bit for bit whatever order the matrix pipe sums in.
__device__ inline void pca_store_entry(double* __restrict__ gram, uint32_t n, uint32_t row, uint32_t col, double v) {
  if (row > col || col >= n) return;
  gram[(size_t)row * n + col] = v;
  gram[(size_t)col * n + row] = v;
}

// grid (tiles, splits); words [split * words_per_split, ...) of the K range, words_per_split a multiple of kPcaStageWords.
// splits == 1: the tile goes straight to `gram` (divided by `denom`); otherwise to slabs[split][tile][128][128] for pca_slab_reduce_kernel.
static __global__ __launch_bounds__(256, 2) void pca_gram_kernel(const unsigned long long* __restrict__ bitsT, const double2* __restrict__ vals, uint32_t n_pad,
                                                       uint32_t kwords, uint32_t nt, uint32_t words_per_split, uint32_t n, double denom,
                                                       double* __restrict__ gram, double* __restrict__ slabs) {
  __shared__ double2 s_vals[2][kPcaStageSites];
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

  const unsigned long long* pa = bitsT + row0 + r16;
  const unsigned long long* pb = bitsT + col0 + r16;
  unsigned long long na[4] = {0, 0, 0, 0}, nb[4] = {0, 0, 0, 0};
  if (active && w_begin < w_end) {
#pragma unroll
    for (int a = 0; a < 4; ++a) { na[a] = pa[(size_t)w_begin * n_pad + a * 16]; nb[a] = pb[(size_t)w_begin * n_pad + a * 16]; }
  }
  if (w_begin < w_end) s_vals[0][tid] = vals[(size_t)w_begin * 64 + tid];
  __syncthreads();
  int buf = 0;
  for (uint32_t ws = w_begin; ws < w_end; ws += kPcaStageWords, buf ^= 1) {
    // the next stage's pairs travel in a register under this stage's MFMAs and reach LDS just before the barrier
    const bool more = ws + kPcaStageWords < w_end;
    double2 next_vals = double2{0.0, 0.0};
    if (more) next_vals = vals[(size_t)(ws + kPcaStageWords) * 64 + tid];
    if (active) {
#pragma unroll 1
      for (int wi = 0; wi < kPcaStageWords; ++wi) {
        const uint32_t w = ws + wi;
        unsigned long long wa[4], wb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) { wa[a] = na[a] >> kq; wb[a] = nb[a] >> kq; }
        if (w + 1 < w_end) {  // the next word's bits travel while this one is multiplied
#pragma unroll
          for (int a = 0; a < 4; ++a) { na[a] = pa[(size_t)(w + 1) * n_pad + a * 16]; nb[a] = pb[(size_t)(w + 1) * n_pad + a * 16]; }
        }
        const double2* sv = &s_vals[buf][wi * 64 + kq];
#pragma unroll 4
        for (int step = 0; step < 16; ++step) {
          const double2 v = sv[step * 4];  // (set, clear) of site w * 64 + step * 4 + kq
          double oa[4], ob[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            oa[a] = (wa[a] & 1ull) ? v.x : v.y;
            ob[a] = (wb[a] & 1ull) ? v.x : v.y;
            wa[a] >>= 4;
            wb[a] >>= 4;
          }
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(oa[a], ob[b], acc[a][b], 0, 0, 0);
        }
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
      for (int reg = 0; reg < 4; ++reg) pca_store_entry(gram, n, row0 + a * 16 + kq + 4 * reg, col0 + b * 16 + r16, acc[a][b][reg] / denom);
}

// One thread per entry of every upper-triangular tile: the splits' partials summed in split order (a fixed order: two runs give the
// same bits), divided, written with the mirror.
static __global__ __launch_bounds__(256) void pca_slab_reduce_kernel(const double* __restrict__ slabs, uint32_t tiles, uint32_t splits, uint32_t nt, uint32_t n,
                                                              double denom, double* __restrict__ gram) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t per_tile = (size_t)kPcaTile * kPcaTile;
  if (idx >= (size_t)tiles * per_tile) return;
  const uint32_t t = (uint32_t)(idx / per_tile), e = (uint32_t)(idx % per_tile);
  uint32_t ti, tj;
  pca_tile_of(t, nt, &ti, &tj);
  const uint32_t lr = e / kPcaTile, lc = e % kPcaTile;
  const uint32_t row = ti * kPcaTile + lr, col = tj * kPcaTile + lc;
  if (row > col || col >= n) return;  // (also skips the lower-left wave block of a diagonal tile, which no split wrote)
  double sum = 0.0;
  for (uint32_t s = 0; s < splits; ++s) sum += slabs[((size_t)s * tiles + t) * per_tile + e];
  pca_store_entry(gram, n, row, col, sum / denom);
}

// ---- upper triangle <-> full matrix (fmh_pca_gram_sharded: only the triangle travels between the ranks) ----------------------------
// Packed layout: row i holds columns i..n-1 at offset i n - i (i - 1) / 2, n (n + 1) / 2 doubles in all.  Both kernels are streams
// over kPcaTriRows x kPcaTriCols tiles of the FULL matrix, one workgroup per tile (the grid follows the bytes, whatever n is): a
// thread owns two neighbouring columns of one row, so consecutive lanes run along a row and a pair moves as one 16-byte access when
// its address is 16-byte aligned.  No LDS, no scratch.
constexpr int kPcaTriRows = 16, kPcaTriCols = 32;

__device__ inline size_t pca_tri_offset(size_t i, size_t n) { return i * n - i * (i - 1) / 2 - i; }  // + column = index of (i, column)

// full[n][n] -> tri: tiles wholly below the diagonal have nothing to write
static __global__ __launch_bounds__(256) void pca_pack_triangle_kernel(const double* __restrict__ full, uint32_t n, uint32_t tiles_x, double* __restrict__ tri) {
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
  const uint32_t r = ty * kPcaTriRows + (threadIdx.x >> 4), c = tx * kPcaTriCols + 2 * (threadIdx.x & 15);
  if (r >= n || c >= n || c + 1 < r) return;
  const size_t src = (size_t)r * n + c, dst = pca_tri_offset(r, n) + c;
  const bool both = c >= r && c + 1 < n;
  if (both && !(((uintptr_t)(full + src) | (uintptr_t)(tri + dst)) & 15)) {
    *reinterpret_cast<double2*>(tri + dst) = *reinterpret_cast<const double2*>(full + src);
    return;
  }
  if (c >= r) tri[dst] = full[src];
  if (c + 1 < n) tri[dst + 1] = full[src + 1];  // (c + 1 >= r holds for every thread that came this far)
}

// tri -> full[n][n]: entry (r, c) reads the packed (min, max) element, so (r, c) and (c, r) carry the same bits whatever order the
// transport added in.  The writes are whole row segments; below the diagonal the reads of a tile walk down packed rows, 16
// neighbouring rows of one column = one 128-byte line.
static __global__ __launch_bounds__(256) void pca_unpack_triangle_kernel(const double* __restrict__ tri, uint32_t n, uint32_t tiles_x, double* __restrict__ full) {
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
  const uint32_t r = ty * kPcaTriRows + (threadIdx.x >> 4), c = tx * kPcaTriCols + 2 * (threadIdx.x & 15);
  if (r >= n || c >= n) return;
  const size_t dst = (size_t)r * n + c;
  const bool two = c + 1 < n;
  double2 v;
  if (c >= r && two && !((uintptr_t)(tri + pca_tri_offset(r, n) + c) & 15)) {
    v = *reinterpret_cast<const double2*>(tri + pca_tri_offset(r, n) + c);
  } else {
    v.x = c >= r ? tri[pca_tri_offset(r, n) + c] : tri[pca_tri_offset(c, n) + r];
    v.y = !two ? 0.0 : (c + 1 >= r ? tri[pca_tri_offset(r, n) + c + 1] : tri[pca_tri_offset(c + 1, n) + r]);
  }
  if (two && !((uintptr_t)(full + dst) & 15)) { *reinterpret_cast<double2*>(full + dst) = v; return; }
  full[dst] = v.x;
  if (two) full[dst + 1] = v.y;
}

}  // namespace fmh
