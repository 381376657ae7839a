// logistic_kernels.hpp — gfx950 kernels of the logistic association scan (logistic.hip; definition in include/ferromic_hip.h, scheme in
// DESIGN.md section 3.19).
//
// assoc_homalt_kernel: for every row r and value column k
//   H[r][k] = sum over the selected samples i of c_i(r) [g_i(r) = 2] V[i][k]
// exactly, the contraction of assoc_kernels.hpp with another A operand: the same row blocks, passes, B layout (assoc_digits_kernel), LDS
// staging, accumulators and stores.  Of a plane word w, lo = w & 0x55555555 and hi = (w >> 1) & 0x55555555 are the two alleles of 16
// samples; lo & hi is 1 in the 2-bit field of a sample whose alleles are both 1, masked with "both entries called and no upper-plane bit" and
// widened to bytes by assoc_widen.  The operand is 0 or 1, so a digit accumulator holds at most n * 128 in magnitude.  A kernel of its own:
// the two assoc_sums_kernel instantiations are not touched.
//
// logistic_score_kernel: one thread per (row, phenotype of the batch); the arithmetic is logistic_score_one (logistic_host.hpp), which the
// host twin calls too.  No LDS.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "assoc_kernels.hpp"
#include "logistic_host.hpp"

namespace fmh {

// Launched with kAssocThreads threads; 16 KiB of static LDS.  A.dosage_sum receives H; A.called_sum is not read.
__global__ __launch_bounds__(kAssocThreads) void assoc_homalt_kernel(const AssocArgs A) {
  __shared__ uint4 s_b[kAssocChunkVecs];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t arow = lane & 15u, chunk = lane >> 4;
  const bool upper = A.p1 || A.p2;

  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const size_t first = (size_t)it * A.item_rows;  // of the range
    const uint32_t rows = (uint32_t)(A.row_count - first < A.item_rows ? A.row_count - first : A.item_rows);
    for (uint32_t base = 0; base < rows; base += kAssocPassRows) {
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
        assoc_v4i acc[2][4];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[m][j] = assoc_v4i{0, 0, 0, 0};

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
            assoc_v4i a[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
              const uint32_t b = assoc_word(w0[m], t), pc = assoc_word(wc[m], t), hi = assoc_word(wh[m], t);
              const uint32_t called = pc & (pc >> 1) & ~(hi | (hi >> 1)) & kEvenBits;
              a[m] = assoc_operand(b & (b >> 1) & called);  // both alleles 1, the genotype called: 0 or 1 per 2-bit field
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
              const uint4 bv = s_b[(t * 4u + j) * 64u + lane];
              const assoc_v4i b = assoc_v4i{(int)bv.x, (int)bv.y, (int)bv.z, (int)bv.w};
#pragma unroll
              for (int m = 0; m < 2; ++m) acc[m][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m], b, acc[m][j], 0, 0, 0);
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
            if (r < rows && k < A.columns)
              A.dosage_sum[(first + r) * A.columns + k] =
                  (long long)acc[m][0][i] + 256ll * acc[m][1][i] + 65536ll * acc[m][2][i] + 16777216ll * acc[m][3][i];
          }
      }
    }
  }
}

struct LogisticScoreArgs {
  const long long *S, *C;   // [rows][K], K = Pb * (c + 3)
  const long long* H;       // [rows][Pb]
  const uint32_t *hom_ref, *het, *hom_alt;  // [rows]
  const long long* T;       // [K]
  const int32_t* e;         // [K]
  size_t rows;
  uint32_t c, Pb;
  double *score, *variance;  // [rows][Pb]
};

__global__ __launch_bounds__(256) void logistic_score_kernel(const LogisticScoreArgs A) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= A.rows * A.Pb) return;
  const size_t r = idx / A.Pb, p = idx % A.Pb, W = (size_t)A.c + 3, K = W * A.Pb;
  fmh_host::logistic_score_one(A.S + r * K, A.C + r * K, A.H[idx], A.hom_ref[r], A.het[r], A.hom_alt[r], A.T, A.e, A.c, p * W, A.score + idx,
                               A.variance + idx);
}

}  // namespace fmh
