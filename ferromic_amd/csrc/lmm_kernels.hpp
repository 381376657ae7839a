// lmm_kernels.hpp — gfx950 kernels of the mixed-model scan's device projections (lmm.hip; definition in include/ferromic_hip.h, scheme in
// DESIGN.md section 3.25): for every row r of the range
//   T[r][k] = sum over the selected samples i of basis[i][k] x_i(r),   x = the dosage where the genotype is called, else the row's mu
//   quad[r][p] = sum_k weights[p][k] T[r][k]^2          lin[r][j] = sum_k linear[j][k] T[r][k]
// on v_mfma_f64_16x16x4_f64, straight from the bit planes; T is never stored.
//
// The f64 MFMA's register map (pca_kernels.hpp): A: lane l holds A[row l & 15][k = l >> 4]; B: lane l holds B[k = l >> 4][col l & 15];
// C/D: col = l & 15, row = (l >> 4) + 4 * reg.
//
// Projection.  M = 16 components, N = 16 rows of the matrix, the MFMA's K = 4 samples.
//   B (samples x rows) is built in registers: lane (row r = l & 15, quarter q = l >> 4) reads ONE 32-bit word of its row per group of 64
//     samples - word q of the group's 16 bytes, the 16 samples 64 g + 16 q + j - and step j = 0 .. 15 feeds {0, 1, 2, mu_r}[code of sample j],
//     the code as grm_codes_kernel derives it (lo = not called | het, hi = not called | hom-alt; the called and upper planes are read only
//     where the row's row_gap / row_hi say they hold something) and the value chosen on the halves of the double by bit selects
//     (section 3.24).  No f64 image of the genotypes exists anywhere but in these registers.
//   A (components x samples) is the basis, staged through LDS.  lmm_basis_image_kernel writes it once per call in exactly the order a stage is
//     read: [component group of 64][sample group g of 64][step j][component tile ta of 4][quarter q][component c of 16], the sample being
//     MATRIX sample 64 g + 16 q + j.  A sample that is not selected (or past the matrix) has a zero row, so a sample list costs no gather
//     and the junk bits of a row's padding meet zeros; components past K are zero columns.  A stage is 32 KiB, a plain copy, double-buffered;
//     a wave's A read of (j, ta) is 64 consecutive doubles.
//
// Work.  A workgroup of 256 threads = 4 waves owns a row block (item) on the persistent grid and walks it in passes of 128 rows: a wave holds
//   two 16-row tiles against the four component tiles of a component group, 8 accumulators.  Per pass it walks the component groups in
//   ascending order and, per component group, the sample groups in ascending order: 2 * 128 * 64 flops per 512 bytes of basis read from
//   L2 / the Infinity Cache, 32 flops per byte.
//
// Reduction over components, on the matrix pipe.  When a component group is done a lane holds T[component (l >> 4) + 4 i][row l & 15] in
//   register i of each accumulator: exactly a B operand (k = l >> 4, col = l & 15) of component 4 i + k.  Step i feeds D value i (for quad
//   its square) against a coefficient tile A2[j = l & 15][k = l >> 4] = coef[j][component base + 4 i + k], which lmm_coef_image_kernel laid
//   out to match: [component group][ta][i][coefficient tile][lane].  ceil(L / 16) + 1 accumulators per row tile collect lin and quad over all
//   component groups; at the end of the pass D2 has col = row of the matrix and row = output (l >> 4) + 4 reg of the tile, and every (row,
//   output) entry is stored once.  A row past the item's end computes on the item's last row and stores nothing.  Nothing is zeroed, nothing is atomic; the order of every sum is fixed by this file alone.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pca_kernels.hpp"  // pca_f64x4
#include "plane_rows.hpp"

namespace fmh {

constexpr uint32_t kLmmThreads = 256;
constexpr uint32_t kLmmPassRows = 128;       // 4 waves x 2 tiles x 16 rows
constexpr uint32_t kLmmGroupSamples = 64;    // samples of one stage: 16 bytes of a plane row
constexpr uint32_t kLmmGroupComps = 64;      // components of one stage: 4 tiles
constexpr uint32_t kLmmStageDoubles = kLmmGroupSamples * kLmmGroupComps;  // 32 KiB
constexpr uint32_t kLmmMaxLinTiles = 4;      // L <= 64: lmm_project_kernel<1 .. 4>
constexpr uint32_t kLmmCoefTileDoubles = 64; // one (ta, i, coefficient tile): a double per lane

struct LmmArgs : PlaneRows {  // the packed image first (plane_rows.hpp)
  uint32_t groups;            // sample groups: 16-byte vectors of a row through the last selected sample (<= plane_pitch / 16)
  uint32_t cgroups;           // component groups: ceil(K / 64)
  uint32_t lin_tiles;         // ceil(L / 16)
  uint32_t P, L;
  const double* basis_image;  // [cgroups][groups][kLmmStageDoubles]
  const double* coef_image;   // [cgroups][4 ta][4 i][lin_tiles + 1][64 lanes]; the last tile is the weights'
  const double* mu;           // [row_count]
  size_t row_begin, row_count;
  uint32_t item_rows;         // a multiple of kLmmPassRows unless one item holds every row
  uint32_t n_items;
  double *quad, *lin;         // [row_count][P], [row_count][L]
};

// The basis in stage order.  One thread per double of the image.  rank[s] = the list position of matrix sample s or -1 (null: s itself while
// s < n); basis [n][K].
static __global__ __launch_bounds__(256) void lmm_basis_image_kernel(const double* __restrict__ basis, const int32_t* __restrict__ rank, uint32_t n,
                                                                     uint32_t covered, uint32_t K, uint32_t groups, size_t total,
                                                                     double* __restrict__ image) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const uint32_t c = (uint32_t)idx & 15u, q = (uint32_t)(idx >> 4) & 3u, ta = (uint32_t)(idx >> 6) & 3u, j = (uint32_t)(idx >> 8) & 15u;
  const size_t stage = idx >> 12;
  const uint32_t g = (uint32_t)(stage % groups);
  const size_t cg = stage / groups;
  const size_t s = (size_t)g * kLmmGroupSamples + 16u * q + j, k = cg * kLmmGroupComps + 16u * ta + c;
  double v = 0.0;
  if (k < K && s < covered) {
    const int64_t r = rank ? (int64_t)rank[s] : (s < n ? (int64_t)s : -1);
    if (r >= 0) v = basis[(size_t)r * K + k];
  }
  image[idx] = v;
}

// The coefficients in the order the reduction reads them.  One thread per double.  linear [L][K], weights [P][K]; outputs past L (or P) and
// components past K are zero.
static __global__ __launch_bounds__(256) void lmm_coef_image_kernel(const double* __restrict__ linear, const double* __restrict__ weights, uint32_t L,
                                                                    uint32_t P, uint32_t K, uint32_t lin_tiles, size_t total, double* __restrict__ image) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const uint32_t lane = (uint32_t)idx & 63u, tiles = lin_tiles + 1u;
  size_t rest = idx >> 6;
  const uint32_t t = (uint32_t)(rest % tiles);
  rest /= tiles;
  const uint32_t i = (uint32_t)rest & 3u, ta = (uint32_t)(rest >> 2) & 3u;
  const size_t cg = rest >> 4;
  const size_t k = cg * kLmmGroupComps + 16u * ta + 4u * i + (lane >> 4);
  const uint32_t j = 16u * t + (lane & 15u);
  double v = 0.0;
  if (k < K) {
    if (t < lin_tiles) { if (j < L) v = linear[(size_t)j * K + k]; }
    else if ((lane & 15u) < P) v = weights[(size_t)(lane & 15u) * K + k];
  }
  image[idx] = v;
}

// {0, 1, 2, mu}[code], code = (bit `off` of lo) + 2 * (bit `off` of hi), on the halves of the double
__device__ __forceinline__ double lmm_operand(uint32_t lo, uint32_t hi, uint32_t off, uint32_t mu_lo, uint32_t mu_hi) {
  const uint32_t L = (uint32_t)__builtin_amdgcn_sbfe((int)lo, off, 1u), H = (uint32_t)__builtin_amdgcn_sbfe((int)hi, off, 1u);
  const uint32_t both = L & H;
  const uint32_t high = (both & mu_hi) | (~both & ((L & 0x3FF00000u) | (H & 0x40000000u)));  // 1.0, 2.0 or mu; 0.0 where neither bit is set
  return __hiloint2double((int)high, (int)(both & mu_lo));
}

// the plane words of one lane's row for one sample group
struct LmmWords { uint32_t b, pc, hi; };

// Launched with kLmmThreads threads; 64 KiB of static LDS (two stages).  LT = ceil(L / 16), the coefficient tiles of lin: the reduction's
// accumulators are registers, so their number is the instantiation's.
template <uint32_t LT>
__global__ __launch_bounds__(kLmmThreads, 2) void lmm_project_kernel(const LmmArgs A) {
  __shared__ double2 s_stage[2][kLmmStageDoubles / 2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t r16 = lane & 15u, kq = lane >> 4;
  const uint32_t n_stages = A.cgroups * A.groups;  // per pass: the image, front to back
  const double2* image = reinterpret_cast<const double2*>(A.basis_image);
  constexpr uint32_t kVecs = kLmmStageDoubles / 2 / kLmmThreads;  // 16-byte vectors of a stage per thread: 8
  constexpr uint32_t kCoefTiles = LT + 1u;
  const uint8_t *p0 = A.p0, *p1 = A.p1, *p2 = A.p2, *pc = A.pc;  // (locals: a lambda that named A would have its copy put in memory)

  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const size_t first = (size_t)it * A.item_rows;  // of the range
    const uint32_t rows = (uint32_t)(A.row_count - first < A.item_rows ? A.row_count - first : A.item_rows);
    for (uint32_t base = 0; base < rows; base += kLmmPassRows) {
      // this lane's row of each of the wave's two tiles (a row past the item stands in for the item's last row: its sums are never
      // stored), its mu, and whether its called / upper planes hold anything
      size_t at[2];
      uint32_t gap[2], high[2];  // all ones where the row's called / upper planes hold something
      uint32_t mu_lo[2], mu_hi[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const uint32_t r = base + wave * 32u + (uint32_t)m * 16u + r16;
        const size_t rel = first + (r < rows ? r : rows - 1);
        const size_t row = A.row_begin + rel;
        at[m] = row * A.plane_pitch + 4u * kq;  // word kq of a group's 16 bytes
        gap[m] = (A.row_gap ? A.row_gap[row] != 0 : true) ? ~0u : 0u;
        high[m] = (A.row_hi ? A.row_hi[row] != 0 : true) ? ~0u : 0u;
        const double mu = A.mu[rel];
        mu_lo[m] = (uint32_t)__double2loint(mu);
        mu_hi[m] = (uint32_t)__double2hiint(mu);
      }
      // the called and the upper planes are fetched by the whole wave or not at all (every address is a row of the matrix); a lane whose
      // row holds nothing there takes the fill instead of what it read
      const bool wave_gap = pc && __any((int)(gap[0] | gap[1])), wave_high = (p1 || p2) && __any((int)(high[0] | high[1]));
      auto fetch = [p0, p1, p2, pc, wave_gap, wave_high, &at, &gap, &high](uint32_t g, LmmWords (&w)[2]) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const size_t off = at[m] + (size_t)g * 16;
          w[m].b = *reinterpret_cast<const uint32_t*>(p0 + off);
          uint32_t c = ~0u, h = 0u;
          if (wave_gap) c = *reinterpret_cast<const uint32_t*>(pc + off);
          if (wave_high) {
            if (p1) h = *reinterpret_cast<const uint32_t*>(p1 + off);
            if (p2) h |= *reinterpret_cast<const uint32_t*>(p2 + off);
          }
          w[m].pc = c | ~gap[m];
          w[m].hi = h & high[m];
        }
      };

      pca_f64x4 acc[4][2], red[kCoefTiles][2];  // red[LT]: quad
#pragma unroll
      for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int ta = 0; ta < 4; ++ta) acc[ta][m] = pca_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (uint32_t t = 0; t < kCoefTiles; ++t) red[t][m] = pca_f64x4{0.0, 0.0, 0.0, 0.0};
      }

      // (the barrier that closed the pass before has every wave past its last stage)
#pragma unroll
      for (uint32_t v = 0; v < kVecs; ++v) s_stage[0][tid + v * kLmmThreads] = image[tid + v * kLmmThreads];
      LmmWords cur[2], nxt[2];
      fetch(0, cur);
      __syncthreads();
      uint32_t buf = 0, g = 0, cg = 0;
      for (uint32_t stage = 0; stage < n_stages; ++stage, buf ^= 1u) {
        // the next stage travels in registers under this stage's MFMAs and reaches LDS just before the barrier
        // (the last stage fetches itself again and nobody reads the copy: no branch, and the registers stay registers)
        const uint32_t ahead = stage + 1 < n_stages ? stage + 1 : stage;
        const uint32_t g_next = g + 1 == A.groups ? 0u : g + 1;
        const double2* src = image + (size_t)ahead * (kLmmStageDoubles / 2);
        double2 next[kVecs];
#pragma unroll
        for (uint32_t v = 0; v < kVecs; ++v) next[v] = src[tid + v * kLmmThreads];
        fetch(g_next, nxt);

        uint32_t lo[2], hi[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const uint32_t b = cur[m].b, pc = cur[m].pc, h = cur[m].hi;
          const uint32_t cal = pc & (pc >> 1) & ~(h | (h >> 1)) & kEvenBits, uncalled = ~cal & kEvenBits;
          lo[m] = uncalled | (cal & (b ^ (b >> 1)));  // het
          hi[m] = uncalled | (cal & b & (b >> 1));    // hom-alt
        }
        const double* sa = reinterpret_cast<const double*>(s_stage[buf]) + lane;
#pragma unroll 2
        for (uint32_t j = 0; j < 16; ++j) {
          double x[2];
#pragma unroll
          for (int m = 0; m < 2; ++m) x[m] = lmm_operand(lo[m], hi[m], 2u * j, mu_lo[m], mu_hi[m]);
#pragma unroll
          for (int ta = 0; ta < 4; ++ta) {
            const double a = sa[(j * 4u + (uint32_t)ta) * 64u];
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[ta][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, x[m], acc[ta][m], 0, 0, 0);
          }
        }

        if (g + 1 == A.groups) {
          // the component group is done: contract its T (and T^2) with the coefficient tiles, then start the next group from zero
          const double* coef = A.coef_image + (size_t)cg * (16u * kCoefTiles * kLmmCoefTileDoubles) + lane;
#pragma unroll
          for (int ta = 0; ta < 4; ++ta) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const double* tile = coef + (ta * 4 + i) * (kCoefTiles * kLmmCoefTileDoubles);
#pragma unroll
              for (uint32_t t = 0; t < kCoefTiles; ++t) {
                const double cf = tile[t * kLmmCoefTileDoubles];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                  const double tv = acc[ta][m][i];
                  red[t][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(cf, t == LT ? tv * tv : tv, red[t][m], 0, 0, 0);
                }
              }
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) acc[ta][m] = pca_f64x4{0.0, 0.0, 0.0, 0.0};
          }
          ++cg;
        }

#pragma unroll
        for (uint32_t v = 0; v < kVecs; ++v) s_stage[buf ^ 1u][tid + v * kLmmThreads] = next[v];  // last read in the stage before this one
        cur[0] = nxt[0];
        cur[1] = nxt[1];
        g = g_next;
        __syncthreads();
      }

      // D2: col = the row of the matrix (l & 15), row = output (l >> 4) + 4 reg of the coefficient tile
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const uint32_t r = base + wave * 32u + (uint32_t)m * 16u + r16;
        if (r >= rows) continue;
        const size_t row = first + r;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const uint32_t o = kq + 4u * (uint32_t)reg;
          if (o < A.P) A.quad[row * A.P + o] = red[LT][m][reg];
#pragma unroll
          for (uint32_t t = 0; t < LT; ++t)
            if (16u * t + o < A.L) A.lin[row * A.L + 16u * t + o] = red[t][m][reg];
        }
      }
    }
  }
}

}  // namespace fmh
