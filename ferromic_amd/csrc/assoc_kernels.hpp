// assoc_kernels.hpp — gfx950 kernels of the association scan's device sums (assoc.hip; definition in include/ferromic_hip.h, scheme in
// DESIGN.md section 3.18): for every row r and value column k
//   S[r][k] = sum over the selected samples i of c_i(r) g_i(r) V[i][k]        C[r][k] = sum of c_i(r) V[i][k]
// exactly, as an int8 contraction over samples on v_mfma_i32_16x16x64_i8 with i32 accumulators.
//
// Operands.  V is i32 fixed point, |V| <= 2^30, split into four SIGNED base-256 digits, V = d0 + 256 d1 + 65 536 d2 + 16 777 216 d3 with
// d in [-128, 127]; the dosage g in {0, 1, 2} (and, for C, the called flag in {0, 1}) is the other int8 operand, so a digit accumulator holds
// at most 2 * 2^22 * 128 = 2^30 in magnitude and the four are recombined in i64.
//   A (16 rows x 64 samples per MFMA): lane l supplies row l & 15 and the 16 samples of ONE 32-bit word of that row - a word of a diploid
//     plane row holds 16 samples, sample j at bits 2 j and 2 j + 1.  lo = w & 0x55555555 and hi = (w >> 1) & 0x55555555 are the two alleles,
//     lo + hi the dosage in 2-bit fields, masked with "both entries called and no upper-plane bit"; the 16 fields widened to bytes are the 16
//     consecutive K bytes the lane feeds (assoc_widen, five integer operations per four samples).  No byte image of the genotypes exists
//     anywhere but in these registers.  A lane fetches 16 bytes of its row at once - four words, the operands of four MFMA steps t = 0 .. 3:
//     the word of (group g of 256 samples, lane chunk c = l >> 4, step t) is word 16 g + 4 c + t of the row.
//   B (64 samples x 16 columns): written once per call by assoc_digits_kernel in exactly that order, [g][value group][t][digit j][lane] x 16
//     bytes: lane l holds, for value column 16 vg + (l & 15), digit j of the 16 samples of word 16 g + 4 (l >> 4) + t.  Rows are MATRIX sample
//     numbers; a sample that is not selected (or past the matrix) has zero digits, so a sample list costs no gather and the junk bits of the
//     row's padding meet zeros.  Both operands follow one (sample -> lane, byte) rule, so the sum over K is the plain dot product whatever
//     order the instruction walks K in.
//   The four digits of a value column sit in four B tiles at the SAME lane: C/D has column = lane & 15 and row = 4 (lane >> 4) + register, so
//     a lane recombines its own four accumulators and stores S[row][column] with plain 64-bit stores.
//
// Work.  A workgroup of 256 threads = 4 waves owns a row block (item) on the persistent grid and walks it in passes of 128 rows: a wave holds
// two 16-row tiles.  Per pass and value group (16 value columns = 4 digit tiles) it walks the sample groups; the 16 KiB of B of a (group, value
// group) are staged in LDS once and read by all four waves for both of their tiles (and for both A operands when C is wanted): eight to
// sixteen MFMAs per KiB read from LDS.  More than 16 value columns re-read the pass's rows (128 x the row's bytes, L2-resident at cohort
// widths) once per further value group.  Nothing is zeroed and nothing is added atomically: every output entry has one writer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plane_rows.hpp"  // kEvenBits

namespace fmh {

constexpr uint32_t kAssocThreads = 256;
constexpr uint32_t kAssocPassRows = 128;          // 4 waves x 2 tiles x 16 rows
constexpr uint32_t kAssocGroupSamples = 256;      // samples of one staged B chunk: 64 bytes of a plane row
constexpr uint32_t kAssocChunkVecs = 16 * 64;     // 16-byte vectors of one (group, value group) of B: [4 t][4 digits][64 lanes] = 16 KiB
constexpr uint32_t kAssocMaxColumns = 64;

typedef int assoc_v4i __attribute__((ext_vector_type(4)));

struct AssocArgs : PlaneRows {  // the packed image first (plane_rows.hpp)
  uint32_t nvec;                     // 16-byte vectors of a row through the last selected sample (<= plane_pitch / 16)
  uint32_t groups;                   // ceil(nvec / 4)
  uint32_t columns;                  // K
  uint32_t vgroups;                  // ceil(K / 16)
  const uint4* digits;               // [groups][vgroups][kAssocChunkVecs]
  size_t row_begin, row_count;
  uint32_t item_rows;
  uint32_t n_items;
  long long *dosage_sum, *called_sum;  // [row_count][K]; called_sum may be null (then CALLED is false)
};

// digit j (0 .. 3) of the signed base-256 expansion of v, as a byte
__host__ __device__ inline uint32_t assoc_digit(int32_t v, uint32_t j) {
  for (uint32_t i = 0; i < j; ++i) v = (v - (int32_t)(int8_t)(v & 0xFF)) >> 8;
  return (uint32_t)(v & 0xFF);
}

// B in MFMA operand order.  One thread per 16-byte vector.  rank[s] = the position of matrix sample s in the list or -1 (null: s itself
// while s < n); values [n][K].  `static`: logistic.hip includes this header too (as pairwise_kernels.hpp's plain kernels are for kinship.hip).
static __global__ __launch_bounds__(256) void assoc_digits_kernel(const int32_t* __restrict__ values, const int32_t* __restrict__ rank, uint32_t n,
                                                           uint32_t covered, uint32_t K, uint32_t vgroups, size_t n_vectors, uint4* __restrict__ digits) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_vectors) return;
  const uint32_t lane = (uint32_t)(idx & 63), j = (uint32_t)(idx >> 6) & 3u, t = (uint32_t)(idx >> 8) & 3u;
  const size_t chunk = idx >> 10;
  const uint32_t vg = (uint32_t)(chunk % vgroups);
  const size_t g = chunk / vgroups;
  const uint32_t k = 16u * vg + (lane & 15u);
  const size_t first = (16 * g + 4 * (lane >> 4) + t) * 16;  // the word's first sample
  uint32_t out[4] = {0, 0, 0, 0};
  if (k < K) {
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b) {
      const size_t s = first + b;
      int64_t r = -1;
      if (s < covered) r = rank ? (int64_t)rank[s] : (s < n ? (int64_t)s : -1);
      if (r >= 0) out[b / 4] |= assoc_digit(values[(size_t)r * K + k], j) << (8 * (b % 4));
    }
  }
  digits[idx] = make_uint4(out[0], out[1], out[2], out[3]);
}

// C of a matrix that is biallelic with nothing missing: every row's called sum is the column total
static __global__ __launch_bounds__(256) void assoc_fill_kernel(const long long* __restrict__ totals, uint32_t K, size_t count, long long* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) out[i] = totals[i % K];
}

// four 2-bit fields (the low 8 bits of x) -> four bytes
__device__ __forceinline__ uint32_t assoc_widen(uint32_t x) {
  const uint32_t y = (x | (x << 12)) & 0x000F000Fu;
  return (y | (y << 6)) & 0x03030303u;
}
__device__ __forceinline__ assoc_v4i assoc_operand(uint32_t fields) {
  return assoc_v4i{(int)assoc_widen(fields & 0xFFu), (int)assoc_widen((fields >> 8) & 0xFFu), (int)assoc_widen((fields >> 16) & 0xFFu),
                   (int)assoc_widen(fields >> 24)};
}

__device__ __forceinline__ uint32_t assoc_word(const uint4& v, uint32_t t) { return t == 0 ? v.x : t == 1 ? v.y : t == 2 ? v.z : v.w; }

// Launched with kAssocThreads threads; 16 KiB of static LDS.
template <bool CALLED>
__global__ __launch_bounds__(kAssocThreads) void assoc_sums_kernel(const AssocArgs A) {
  __shared__ uint4 s_b[kAssocChunkVecs];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t arow = lane & 15u, chunk = lane >> 4;
  const bool upper = A.p1 || A.p2;

  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const size_t first = (size_t)it * A.item_rows;  // of the range
    const uint32_t rows = (uint32_t)(A.row_count - first < A.item_rows ? A.row_count - first : A.item_rows);
    for (uint32_t base = 0; base < rows; base += kAssocPassRows) {
      // this lane's row of each of the wave's two tiles, and whether its called / upper planes hold anything
      size_t at[2];
      bool live[2], gap[2], high[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const uint32_t r = base + wave * 32u + (uint32_t)m * 16u + arow;
        live[m] = r < rows;
        const size_t row = A.row_begin + first + (live[m] ? r : rows - 1);
        at[m] = row * A.plane_pitch;
        gap[m] = A.pc && (A.row_gap ? A.row_gap[row] != 0 : true);
        high[m] = upper && (A.row_hi ? A.row_hi[row] != 0 : true);
      }
      for (uint32_t vg = 0; vg < A.vgroups; ++vg) {
        assoc_v4i acc_s[2][4], acc_c[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc_s[m][j] = acc_c[m][j] = assoc_v4i{0, 0, 0, 0};

        for (uint32_t g = 0; g < A.groups; ++g) {
          // the 16 bytes of this lane's rows: four words = the A operands of steps t = 0 .. 3.  A vector past the covered samples is zero.
          const uint32_t vec = 4u * g + chunk;
          uint4 w0[2], wc[2], wh[2];
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            const bool ok = live[m] && vec < A.nvec;
            const size_t off = at[m] + (size_t)vec * 16;
            w0[m] = ok ? *reinterpret_cast<const uint4*>(A.p0 + off) : make_uint4(0, 0, 0, 0);
            wc[m] = ok ? (gap[m] ? *reinterpret_cast<const uint4*>(A.pc + off) : make_uint4(~0u, ~0u, ~0u, ~0u)) : make_uint4(0, 0, 0, 0);
            wh[m] = make_uint4(0, 0, 0, 0);
            if (ok && high[m]) {
              if (A.p1) wh[m] = *reinterpret_cast<const uint4*>(A.p1 + off);
              if (A.p2) {
                const uint4 h2 = *reinterpret_cast<const uint4*>(A.p2 + off);
                wh[m].x |= h2.x; wh[m].y |= h2.y; wh[m].z |= h2.z; wh[m].w |= h2.w;
              }
            }
          }
          __syncthreads();  // every wave has read the chunk before this one
          const uint4* src = A.digits + ((size_t)g * A.vgroups + vg) * kAssocChunkVecs;
#pragma unroll
          for (uint32_t q = 0; q < kAssocChunkVecs / kAssocThreads; ++q) s_b[tid + q * kAssocThreads] = src[tid + q * kAssocThreads];
          __syncthreads();
#pragma unroll
          for (uint32_t t = 0; t < 4; ++t) {
            assoc_v4i a_s[2], a_c[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
              const uint32_t b = assoc_word(w0[m], t), pc = assoc_word(wc[m], t), hi = assoc_word(wh[m], t);
              const uint32_t called = pc & (pc >> 1) & ~(hi | (hi >> 1)) & kEvenBits;
              const uint32_t dosage = ((b & kEvenBits) + ((b >> 1) & kEvenBits)) & (called * 3u);
              a_s[m] = assoc_operand(dosage);
              if constexpr (CALLED) a_c[m] = assoc_operand(called);
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
              const uint4 bv = s_b[(t * 4u + j) * 64u + lane];
              const assoc_v4i b = assoc_v4i{(int)bv.x, (int)bv.y, (int)bv.z, (int)bv.w};
#pragma unroll
              for (int m = 0; m < 2; ++m) {
                acc_s[m][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_s[m], b, acc_s[m][j], 0, 0, 0);
                if constexpr (CALLED) acc_c[m][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_c[m], b, acc_c[m][j], 0, 0, 0);
              }
            }
          }
        }

        // C/D: column (value) = lane & 15, row = 4 (lane >> 4) + register.  The lane's four digit accumulators of a value, recombined in i64.
        const uint32_t k = 16u * vg + arow;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const uint32_t r = base + wave * 32u + (uint32_t)m * 16u + 4u * chunk + (uint32_t)i;
            if (r < rows && k < A.columns) {
              const size_t o = (first + r) * A.columns + k;
              A.dosage_sum[o] = (long long)acc_s[m][0][i] + 256ll * acc_s[m][1][i] + 65536ll * acc_s[m][2][i] + 16777216ll * acc_s[m][3][i];
              if constexpr (CALLED)
                A.called_sum[o] = (long long)acc_c[m][0][i] + 256ll * acc_c[m][1][i] + 65536ll * acc_c[m][2][i] + 16777216ll * acc_c[m][3][i];
            }
          }
      }
    }
  }
}

}  // namespace fmh
