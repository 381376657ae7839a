// admix_kernels.hpp — gfx950 kernels of the admixture model's EM step (admix.hip; definition in include/ferromic_hip.h, scheme in DESIGN.md
// section 3.27).  One step reads the 2-bit code image of the usable rows (geno_codes.hpp) and the state Q [n][K], F [m][K] and writes Q', F'
// and, where wanted, the log-likelihood of the input, all on v_mfma_f64_16x16x4_f64.
//
// The f64 MFMA's register map (pca_kernels.hpp): A: lane l holds A[row l & 15][k = l >> 4]; B: lane l holds B[k = l >> 4][col l & 15];
// C/D: col = l & 15, row = (l >> 4) + 4 * reg.  Below r16 = l & 15, kq = l >> 4.
//
// Unit of work: a tile of 16 usable rows j0 .. j0 + 15 against 16 samples i0 .. i0 + 15.
//   h0 = F Q^T, h1 = G Q^T (G = 1 - F): A operand F[j0 + r16][4 s + kq], B operand Q[i0 + r16][4 s + kq], s < KS = ceil(K / 4): 2 KS MFMAs.
//     D: the lane holds h[row j0 + kq + 4 reg][sample i0 + r16], reg = 0 .. 3.
//   u = g / h0, v = (2 - g) / h1 in that layout from the sample's code bits of the four rows (0 where the genotype is not called): the two
//     divisions per genotype.  With logarithms the lane multiplies the eight factors h^g of its four genotypes and takes one log per tile.
//   E^T[k][i] += sum_j F[j][k] u[j][i] + G[j][k] v[j][i]: the D registers of u and v ARE B operands (k index = kq <-> row 4 reg + kq,
//     col = sample), against A operands F[j0 + 4 reg + kq][k = r16]: 8 MFMAs.  D: E[sample r16][component kq + 4 reg].
//   A^T[k][j] += sum_i Q[i][k] u[j][i] (B^T with v): A operand Q[i0 + 4 t + kq][k = r16]; the B operand wants u[row r16][sample 4 t + kq],
//     the transpose of what the lane holds.  The tile goes through a 16 x 17 LDS block private to the wave (4 stores, 4 loads per matrix,
//     no workgroup barrier): 8 MFMAs.  D: A[row r16][component kq + 4 reg].  The tile is computed once.
//   2 KS + 16 MFMAs per tile.
//
// Work split.  A workgroup of 256 threads = 4 waves owns a block (item) of usable rows on the persistent grid and walks it in passes of 128
//   rows; a wave holds two row tiles, their F and G operands and their A, B accumulators in registers while it walks ALL sample tiles, so A and
//   B are complete inside the wave and f' is stored once.  Per sample tile the four waves' E (their 32 rows each) are added in wave order
//   through LDS and go to the slab [item][n_pad][16]: written by the first pass, added into by the later ones, always by the same thread.
//   The lanes' log sums are reduced per item in a fixed tree to one partial.  admix_reduce_kernel adds the slabs over the items in ascending
//   order, applies q E / (2 m_i), the clamp and the renormalisation, and sums the items' log partials in a fixed order.
//   Nothing is zeroed by the caller, nothing is atomic: the order of every sum is fixed by the item size alone.
// Padding.  Q and F are first copied into images of 16 components (q_pad [n_pad][16], f_pad [m_pad][16]): components past K are zero columns,
//   samples past n zero rows, rows past m hold 0.5.  Codes of padding samples and rows read as not called, which selects u = v = 0 and a
//   divisor of one, so no padding value reaches a stored number.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pca_kernels.hpp"  // pca_f64x4

namespace fmh {

constexpr uint32_t kAdmixThreads = 256;
constexpr uint32_t kAdmixPassRows = 128;  // 4 waves x 2 tiles x 16 rows
constexpr uint32_t kAdmixComps = 16;      // components of the padded images
constexpr double kAdmixEpsDev = 1e-5;

struct AdmixArgs {
  const uint32_t* code32;  // the code image as 32-bit halves: half h of word w, sample s of plane p at ((p * kwords + w) * n_pad + s) * 2 + h
  size_t plane_halves;     // halves of a plane: kwords * n_pad * 2
  uint32_t n_pad, n_tiles; // samples of the image (a multiple of 16) and its tiles
  uint32_t m, K;           // usable rows; components
  uint32_t item_rows;      // a multiple of kAdmixPassRows
  uint32_t n_items;
  uint32_t update_q, update_f;
  const double* q_pad;     // [n_pad][16]
  const double* f_pad;     // [round_up(m, 128)][16]
  double* f_out;           // [m][K]
  double* slab;            // [n_items][n_pad][16]
  double* ll_part;         // [n_items]
};

// dst [rows_pad][16] from src [rows][K]: zero columns past K; rows past `rows` hold `fill` in the first K columns.  One thread per double.
static __global__ __launch_bounds__(256) void admix_pad_kernel(const double* __restrict__ src, size_t rows, uint32_t K, size_t rows_pad, double fill,
                                                               double* __restrict__ dst) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows_pad * kAdmixComps) return;
  const size_t r = idx >> 4;
  const uint32_t k = (uint32_t)idx & 15u;
  double v = 0.0;
  if (k < K) v = r < rows ? src[r * K + k] : fill;
  dst[idx] = v;
}

// m_i: the called genotypes of a sample over the image (rows past the list and padding words read as not called).  One thread per sample.
static __global__ __launch_bounds__(256) void admix_sites_kernel(const unsigned long long* __restrict__ code, size_t kwords, size_t n_pad, uint32_t n,
                                                                 uint32_t* __restrict__ sites) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  uint32_t count = 0;
  for (size_t w = 0; w < kwords; ++w) {
    const unsigned long long lo = code[w * n_pad + s], hi = code[(kwords + w) * n_pad + s];
    count += (uint32_t)__popcll(~(lo & hi));
  }
  sites[s] = count;
}

__device__ __forceinline__ double admix_clamp_dev(double x) { return x < kAdmixEpsDev ? kAdmixEpsDev : (x > 1.0 - kAdmixEpsDev ? 1.0 - kAdmixEpsDev : x); }

// Launched with kAdmixThreads threads; 35 KiB of static LDS.  KS = ceil(K / 4); LOGS: the log-likelihood partials are formed.
template <uint32_t KS, bool LOGS>
__global__ __launch_bounds__(kAdmixThreads, 2) void admix_step_kernel(const AdmixArgs A) {
  __shared__ double s_t[4][2][16 * 17];  // per wave: u and v of a tile, [row][sample] with a padded pitch
  __shared__ double s_e[2][4][256];      // per sample tile (double-buffered): the waves' E, [reg][lane]
  __shared__ double s_ll[kAdmixThreads];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t r16 = lane & 15u, kq = lane >> 4;
  const uint32_t* code_lo = A.code32;
  const uint32_t* code_hi = A.code32 + A.plane_halves;
  const double* q_pad = A.q_pad;
  const double* f_pad = A.f_pad;
  double* tu = s_t[wave][0];
  double* tv = s_t[wave][1];
  const bool update_q = A.update_q != 0, update_f = A.update_f != 0;
  uint32_t ebuf = 0;

  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const uint32_t first = it * A.item_rows;
    const uint32_t rows = A.m - first < A.item_rows ? A.m - first : A.item_rows;
    double ll = 0.0;
    for (uint32_t base = 0; base < rows; base += kAdmixPassRows) {
      const uint32_t row0 = first + base + wave * 32u;  // the wave's 32 rows: one 32-bit half of a code word
      // the operands of the wave's two row tiles, held over all sample tiles
      double fA[2][KS], gA[2][KS], fT[2][4], gT[2][4];
      pca_f64x4 accA[2], accB[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const size_t j0 = (size_t)row0 + 16u * (uint32_t)t;
#pragma unroll
        for (uint32_t s = 0; s < KS; ++s) {
          fA[t][s] = f_pad[(j0 + r16) * kAdmixComps + 4u * s + kq];
          gA[t][s] = 1.0 - fA[t][s];
        }
#pragma unroll
        for (uint32_t reg = 0; reg < 4; ++reg) {
          fT[t][reg] = f_pad[(j0 + 4u * reg + kq) * kAdmixComps + r16];
          gT[t][reg] = 1.0 - fT[t][reg];
        }
        accA[t] = pca_f64x4{0.0, 0.0, 0.0, 0.0};
        accB[t] = pca_f64x4{0.0, 0.0, 0.0, 0.0};
      }
      const size_t cbase = (size_t)(row0 >> 6) * A.n_pad * 2u + ((row0 >> 5) & 1u);

      for (uint32_t st = 0; st < A.n_tiles; ++st) {
        const uint32_t i0 = st * 16u;
        const uint32_t lo = code_lo[cbase + (size_t)(i0 + r16) * 2u], hi = code_hi[cbase + (size_t)(i0 + r16) * 2u];
        double qB[KS], qA[4];
#pragma unroll
        for (uint32_t s = 0; s < KS; ++s) qB[s] = q_pad[(size_t)(i0 + r16) * kAdmixComps + 4u * s + kq];
#pragma unroll
        for (uint32_t t4 = 0; t4 < 4; ++t4) qA[t4] = q_pad[(size_t)(i0 + 4u * t4 + kq) * kAdmixComps + r16];
        pca_f64x4 E = pca_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          pca_f64x4 h0 = pca_f64x4{0.0, 0.0, 0.0, 0.0}, h1 = pca_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (uint32_t s = 0; s < KS; ++s) {
            h0 = __builtin_amdgcn_mfma_f64_16x16x4f64(fA[t][s], qB[s], h0, 0, 0, 0);
            h1 = __builtin_amdgcn_mfma_f64_16x16x4f64(gA[t][s], qB[s], h1, 0, 0, 0);
          }
          const uint32_t l16 = lo >> (16u * (uint32_t)t), h16 = hi >> (16u * (uint32_t)t);
          double u[4], v[4], prod = 1.0;
#pragma unroll
          for (uint32_t reg = 0; reg < 4; ++reg) {
            const uint32_t bit = kq + 4u * reg;
            const bool L = (l16 >> bit) & 1u, H = (h16 >> bit) & 1u;
            const bool called = !(L && H);
            // g = L + 2 H where called: u = g / h0, v = (2 - g) / h1
            const double nu = called ? (H ? 2.0 : (L ? 1.0 : 0.0)) : 0.0;
            const double nv = called ? (H ? 0.0 : (L ? 1.0 : 2.0)) : 0.0;
            const double d0 = called ? h0[reg] : 1.0, d1 = called ? h1[reg] : 1.0;
            u[reg] = nu / d0;
            v[reg] = nv / d1;
            if (LOGS) {
              const double a = (L || H) ? d0 : d1;  // g >= 1: a factor h0
              const double b = H ? d0 : d1;         // g == 2: a second one
              prod *= a * b;                        // (not called: d0 = d1 = 1)
            }
          }
          if (LOGS) ll += log(prod);
          if (update_q) {
#pragma unroll
            for (uint32_t reg = 0; reg < 4; ++reg) {
              E = __builtin_amdgcn_mfma_f64_16x16x4f64(fT[t][reg], u[reg], E, 0, 0, 0);
              E = __builtin_amdgcn_mfma_f64_16x16x4f64(gT[t][reg], v[reg], E, 0, 0, 0);
            }
          }
          if (update_f) {
            // the wave's own transposition: [row kq + 4 reg][sample r16] in, [row r16][sample 4 t4 + kq] out
            __builtin_amdgcn_wave_barrier();  // the loads of the tile before are done with the block
#pragma unroll
            for (uint32_t reg = 0; reg < 4; ++reg) {
              tu[(kq + 4u * reg) * 17u + r16] = u[reg];
              tv[(kq + 4u * reg) * 17u + r16] = v[reg];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (uint32_t t4 = 0; t4 < 4; ++t4) {
              const double ut = tu[r16 * 17u + 4u * t4 + kq], vt = tv[r16 * 17u + 4u * t4 + kq];
              accA[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(qA[t4], ut, accA[t], 0, 0, 0);
              accB[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(qA[t4], vt, accB[t], 0, 0, 0);
            }
          }
        }
        if (update_q) {
          // the four waves' E of this sample tile, added in wave order; thread (sample tid >> 4, component tid & 15) owns the slab entry
#pragma unroll
          for (uint32_t reg = 0; reg < 4; ++reg) s_e[ebuf][wave][reg * 64u + lane] = E[reg];
          __syncthreads();  // (a buffer is written again two tiles on: every thread has passed the barrier between)
          const uint32_t sample = tid >> 4, comp = tid & 15u;
          const uint32_t src = (comp >> 2) * 64u + (comp & 3u) * 16u + sample;
          const double sum = ((s_e[ebuf][0][src] + s_e[ebuf][1][src]) + s_e[ebuf][2][src]) + s_e[ebuf][3][src];
          double* entry = A.slab + ((size_t)it * A.n_pad + i0 + sample) * kAdmixComps + comp;
          *entry = base == 0 ? sum : *entry + sum;
          ebuf ^= 1u;
        }
      }

      // f' of the pass: the lane holds A, B of [row r16][component kq + 4 reg]
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const uint32_t j = row0 + 16u * (uint32_t)t + r16;
        if (j >= A.m) continue;
#pragma unroll
        for (uint32_t reg = 0; reg < 4; ++reg) {
          const uint32_t k = kq + 4u * reg;
          if (k >= A.K) continue;
          const double f = f_pad[(size_t)j * kAdmixComps + k];
          double out = f;
          if (update_f) {
            const double fa = f * accA[t][reg], gb = (1.0 - f) * accB[t][reg];
            out = admix_clamp_dev(fa / (fa + gb));
          }
          A.f_out[(size_t)j * A.K + k] = out;
        }
      }
    }

    if (LOGS) {
      // the item's log partial: a fixed tree over the 256 lanes
      s_ll[tid] = ll;
      __syncthreads();
#pragma unroll
      for (uint32_t half = kAdmixThreads / 2; half > 0; half >>= 1) {
        if (tid < half) s_ll[tid] = s_ll[tid] + s_ll[tid + half];
        __syncthreads();
      }
      if (tid == 0) A.ll_part[it] = s_ll[0];
      __syncthreads();
    }
  }
}

// Q' and the log-likelihood.  Block b takes samples 16 b .. 16 b + 15, thread (sample tid >> 4, component tid & 15).  sites [n] = m_i.
// q, q_out [n][K]; slab [n_items][n_pad][16]; ll_out (may be null) = the items' partials: lane t adds items t, t + 256, .. ascending, then a
// fixed tree (block 0).
static __global__ __launch_bounds__(256) void admix_reduce_kernel(const double* __restrict__ slab, uint32_t n_items, uint32_t n_pad, uint32_t n, uint32_t K,
                                                                  const double* __restrict__ q, const uint32_t* __restrict__ sites, uint32_t update_q,
                                                                  double* __restrict__ q_out, const double* __restrict__ ll_part,
                                                                  double* __restrict__ ll_out) {
  __shared__ double s_q[16][17];
  __shared__ double s_l[256];
  const uint32_t tid = threadIdx.x, local = tid >> 4, k = tid & 15u;
  const uint32_t sample = blockIdx.x * 16u + local;
  const bool live = sample < n && k < K;
  double qo = 0.0;
  bool moved = false;
  if (live) {
    qo = q[(size_t)sample * K + k];
    const uint32_t mi = sites[sample];
    moved = update_q != 0 && mi != 0;
    if (moved) {
      double e = 0.0;
      for (uint32_t b = 0; b < n_items; ++b) e += slab[((size_t)b * n_pad + sample) * kAdmixComps + k];
      qo = admix_clamp_dev(qo * e / (2.0 * (double)mi));
    }
  }
  s_q[local][k] = qo;
  __syncthreads();
  if (live) {
    if (moved) {
      double sum = 0.0;
      for (uint32_t kk = 0; kk < K; ++kk) sum += s_q[local][kk];
      qo = qo / sum;
    }
    q_out[(size_t)sample * K + k] = qo;
  }
  if (ll_out && blockIdx.x == 0) {
    double l = 0.0;
    for (uint32_t b = tid; b < n_items; b += 256u) l += ll_part[b];
    s_l[tid] = l;
    __syncthreads();
    for (uint32_t half = 128; half > 0; half >>= 1) {
      if (tid < half) s_l[tid] = s_l[tid] + s_l[tid + half];
      __syncthreads();
    }
    if (tid == 0) *ll_out = s_l[0];
  }
}

}  // namespace fmh
