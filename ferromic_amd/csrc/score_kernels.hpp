// score_kernels.hpp — gfx950 kernels of the polygenic score's device sums (score.hip; definition in include/ferromic_hip.h, scheme in
// DESIGN.md section 3.20): for every selected sample i and value column k
//   S[i][k] = sum over the rows r of the range of c_i(r) g_i(r) V[r][k]        C[i][k] = sum of c_i(r) U[r][k]
// exactly - the contraction of assoc_kernels.hpp transposed: K of the matrix instruction runs over ROWS, the output is per sample.
//
// Operands of v_mfma_i32_16x16x64_i8 (16 samples x 16 value columns per instruction, 64 rows per step).
//   A (16 samples x 64 rows): lane l supplies sample l & 15 of a tile and rows 16 (l >> 4) .. + 15 of the step.  A 32-bit word of a diploid
//     plane row holds exactly the 16 samples of a tile (sample j at bits 2 j and 2 j + 1), so the lane needs ITS 2-bit field of 16 different
//     rows.  The step's [64 rows][64 bytes] block of every plane is fetched once per workgroup, one 16-byte load per thread; the thread turns
//     its four words into `called` and `dosage` in 2-bit fields exactly as assoc_sums_kernel does (upper planes, row_gap / row_hi honoured) and
//     parks THOSE in LDS.  A lane then reads the 16 bytes of a row that hold its wave's four tiles - the 16 lanes of a chunk at one broadcast
//     address, the four chunks 65 vectors apart, so in different banks - and extracts its field of each tile with a bit-field extract and a
//     shift-or: two integer operations per (row, tile, operand).
//   B (64 rows x 16 value columns): V (and U) as four signed base-256 digits, written once per call by score_digits_kernel in operand order,
//     [step][value group][digit j][lane] x 16 bytes: lane l holds, for value column 16 vg + (l & 15), digit j of rows 64 step + 16 (l >> 4)
//     .. + 15 of the RANGE.  Rows past row_count are zero, so a partial last step meets zeros.  A step's 4 KiB (8 KiB with U) are staged in
//     LDS once per workgroup and read by its four waves.
//   C/D: column (value column) = lane & 15, row (sample of the tile) = 4 (lane >> 4) + register: the four digits of a value column sit in
//     four B tiles at the SAME lane, so a lane recombines its own four accumulators in i64, and the 16 lanes of a chunk store 16 consecutive
//     i64 of one sample's slab row.
//
// Work.  A workgroup of 256 threads owns (row block of item_rows rows, sample group of 256 samples) on the persistent grid, items ordered
// row-block-major so that the sample groups of a row block run side by side and share the block's digits - and the halves of a 128-byte line
// of the planes - in L2.  A wave owns 64 samples = 4 tiles x 4 digits x (S, C) accumulators.  More than 16 value columns are further passes
// over the item.  The next step's global loads are issued before the current step's matrix instructions.
// Reduction.  An item writes its i64 partials to the slab [row block][sample of the covered groups][K]; score_reduce_kernel adds the slabs in
// row-block order and writes the selected samples in list order: one writer per entry, no atomics, nothing zeroed.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "assoc_kernels.hpp"  // assoc_digit, assoc_v4i
#include "plane_rows.hpp"  // plane_load, kEvenBits

namespace fmh {

constexpr uint32_t kScoreThreads = 256;
constexpr uint32_t kScoreStepRows = 64;           // K of one matrix instruction
constexpr uint32_t kScoreGroupSamples = 256;      // 4 waves x 4 tiles x 16 samples: 64 bytes of a plane row
constexpr uint32_t kScoreStepVecs = 4 * 64;       // 16-byte vectors of one (step, value group) of digits: [4 digits][64 lanes] = 4 KiB
constexpr uint32_t kScoreFieldVecs = 64 * 4 + 4;  // a step's fields in LDS: [64 rows][4 vectors], one vector of padding per 16 rows
constexpr uint32_t kScoreMaxColumns = 64;

struct ScoreArgs : PlaneRows {  // the packed image first (plane_rows.hpp)
  uint32_t nvec;                     // 16-byte vectors of a row through the last selected sample (<= plane_pitch / 16)
  uint32_t groups;                   // sample groups: ceil(nvec / 4)
  uint32_t columns;                  // K
  uint32_t vgroups;                  // ceil(K / 16)
  const uint4 *digits_v, *digits_u;  // [steps][vgroups][kScoreStepVecs]; digits_u null unless CALLED
  size_t row_begin, row_count;
  uint32_t item_rows;                // a multiple of kScoreStepRows
  uint32_t n_blocks;                 // row blocks
  uint32_t n_items;                  // n_blocks * groups
  long long *slab_s, *slab_c;        // [n_blocks][groups * 256][K]; slab_c null unless CALLED
};

// V (or U) [row_count][K] in MFMA operand order.  One thread per (step, value group, lane): the four digit vectors of its 16 rows.
static __global__ __launch_bounds__(256) void score_digits_kernel(const int32_t* __restrict__ values, size_t row_count, uint32_t K, uint32_t vgroups,
                                                           size_t n_threads, uint4* __restrict__ digits) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_threads) return;
  const uint32_t lane = (uint32_t)(idx & 63);
  const size_t chunk = idx >> 6;  // step * vgroups + vg
  const uint32_t k = 16u * (uint32_t)(chunk % vgroups) + (lane & 15u);
  const size_t first = (chunk / vgroups) * kScoreStepRows + 16u * (lane >> 4);
  uint32_t out[4][4] = {};
  if (k < K) {
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b) {
      const size_t r = first + b;
      if (r >= row_count) break;
      const int32_t v = values[r * K + k];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) out[j][b / 4] |= assoc_digit(v, j) << (8 * (b % 4));
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) digits[(chunk * 4 + j) * 64 + lane] = make_uint4(out[j][0], out[j][1], out[j][2], out[j][3]);
}

// out[i][k] = the sum over the row blocks, in their order, of slab[block][sample of entry i][k]; rank-free: `samples` null = entry i is sample i
static __global__ __launch_bounds__(256) void score_reduce_kernel(const long long* __restrict__ slab, const uint32_t* __restrict__ samples, size_t count,
                                                           uint32_t K, uint32_t n_blocks, size_t block_pitch, long long* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= count) return;
  const size_t i = idx / K;
  const uint32_t k = (uint32_t)(idx % K);
  const size_t s = samples ? samples[i] : i;
  const long long* src = slab + s * K + k;
  long long sum = 0;
  for (uint32_t b = 0; b < n_blocks; ++b) sum += src[(size_t)b * block_pitch];
  out[idx] = sum;
}

// what a thread fetches for one step: its 16 bytes of a row of every plane and its vector of the step's digits
struct ScoreStage {
  uint4 w0, wc, w1, w2, dv, du;
};

__device__ __forceinline__ uint32_t score_field(uint32_t word, uint32_t shift, uint32_t width) { return __builtin_amdgcn_ubfe(word, shift, width); }

// Launched with kScoreThreads threads; static LDS: fields 4 160 B (x 2 when CALLED) + digits 4 KiB (x 2).
template <bool CALLED>
__global__ __launch_bounds__(kScoreThreads, 2) void score_sums_kernel(const ScoreArgs A) {
  __shared__ uint4 s_dos[kScoreFieldVecs];
  __shared__ uint4 s_cal[CALLED ? kScoreFieldVecs : 1];
  __shared__ uint4 s_v[kScoreStepVecs];
  __shared__ uint4 s_u[CALLED ? kScoreStepVecs : 1];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t chunk = lane >> 4, shift = 2u * (lane & 15u);
  const uint32_t srow = tid >> 2, spart = tid & 3u;  // the staging thread's row of the step and 16-byte part of the group's 64 bytes
  const bool upper = A.p1 || A.p2;
  const size_t spad = (size_t)A.groups * kScoreGroupSamples;

  for (uint32_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const uint32_t rb = it / A.groups, sg = it % A.groups;
    const size_t first = (size_t)rb * A.item_rows;  // of the range
    const uint32_t rows = (uint32_t)(A.row_count - first < A.item_rows ? A.row_count - first : A.item_rows);
    const uint32_t steps = (rows + kScoreStepRows - 1) / kScoreStepRows;
    const size_t step0 = first / kScoreStepRows;
    const uint32_t vec = 4u * sg + spart;
    const bool inside = vec < A.nvec;  // a vector past the covered samples is zero

    for (uint32_t vg = 0; vg < A.vgroups; ++vg) {
      assoc_v4i acc_s[4][4], acc_c[4][4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc_s[t][j] = acc_c[t][j] = assoc_v4i{0, 0, 0, 0};

      // whether the called / upper planes of this thread's row of a step hold anything: the raw bytes, compared where they are used
      auto flags = [&](uint32_t s, uint32_t& gap, uint32_t& high) {
        const uint32_t r = s * kScoreStepRows + srow;
        const size_t row = A.row_begin + first + (r < rows ? r : rows - 1);
        gap = A.pc ? (A.row_gap ? (uint32_t)A.row_gap[row] : 1u) : 0u;
        high = upper ? (A.row_hi ? (uint32_t)A.row_hi[row] : 1u) : 0u;
      };
      auto fetch = [&](uint32_t s, uint32_t gap, uint32_t high) {
        const uint32_t r = s * kScoreStepRows + srow;
        const bool ok = inside && r < rows;
        const size_t off = (A.row_begin + first + (r < rows ? r : rows - 1)) * A.plane_pitch + (size_t)(inside ? vec : 0) * 16;
        ScoreStage g;
        g.w0 = plane_load(A.p0, off, ok, 0u);
        g.wc = plane_load(A.pc, off, ok && gap != 0, ok ? ~0u : 0u);
        g.w1 = plane_load(A.p1, off, ok && high != 0 && A.p1, 0u);
        g.w2 = plane_load(A.p2, off, ok && high != 0 && A.p2, 0u);
        const size_t d = ((step0 + s) * A.vgroups + vg) * kScoreStepVecs + tid;
        g.dv = A.digits_v[d];
        g.du = CALLED ? A.digits_u[d] : g.dv;
        return g;
      };

      // the row flags run one step ahead of the planes they gate, so that no fetch waits for a load issued just before it
      uint32_t gap = 0, high = 0;
      flags(0, gap, high);
      ScoreStage g = fetch(0, gap, high);
      flags(1, gap, high);
      for (uint32_t s = 0; s < steps; ++s) {
        // this thread's four words -> `called` and `dosage` in 2-bit fields, parked in LDS with the step's digits
        uint32_t dos[4], cal[4];
        const uint32_t b[4] = {g.w0.x, g.w0.y, g.w0.z, g.w0.w}, pc[4] = {g.wc.x, g.wc.y, g.wc.z, g.wc.w};
        const uint32_t hi[4] = {g.w1.x | g.w2.x, g.w1.y | g.w2.y, g.w1.z | g.w2.z, g.w1.w | g.w2.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          cal[q] = pc[q] & (pc[q] >> 1) & ~(hi[q] | (hi[q] >> 1)) & kEvenBits;
          dos[q] = ((b[q] & kEvenBits) + ((b[q] >> 1) & kEvenBits)) & (cal[q] * 3u);
        }
        __syncthreads();  // every wave has read the step before this one
        const uint32_t at = srow * 4u + spart + (srow >> 4);
        s_dos[at] = make_uint4(dos[0], dos[1], dos[2], dos[3]);
        if constexpr (CALLED) s_cal[at] = make_uint4(cal[0], cal[1], cal[2], cal[3]);
        s_v[tid] = g.dv;
        if constexpr (CALLED) s_u[tid] = g.du;
        __syncthreads();
        if (s + 1 < steps) {  // the next step's loads fly under this step's matrix instructions
          g = fetch(s + 1, gap, high);
          flags(s + 2, gap, high);
        }

        // A: this lane's field of rows 16 chunk .. + 15, for the wave's four tiles
        assoc_v4i a_s[4], a_c[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) a_s[t] = a_c[t] = assoc_v4i{0, 0, 0, 0};
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
          const uint32_t src = (16u * chunk + i) * 4u + wave + chunk;
          const uint4 d = s_dos[src];
          const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
          for (int t = 0; t < 4; ++t) a_s[t][i / 4] |= (int)(score_field(w[t], shift, 2) << (8 * (i % 4)));
          if constexpr (CALLED) {
            const uint4 c = s_cal[src];
            const uint32_t x[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) a_c[t][i / 4] |= (int)(score_field(x[t], shift, 1) << (8 * (i % 4)));
          }
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          const uint4 bv = s_v[j * 64u + lane];
          const assoc_v4i bs = assoc_v4i{(int)bv.x, (int)bv.y, (int)bv.z, (int)bv.w};
#pragma unroll
          for (int t = 0; t < 4; ++t) acc_s[t][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_s[t], bs, acc_s[t][j], 0, 0, 0);
          if constexpr (CALLED) {
            const uint4 bu = s_u[j * 64u + lane];
            const assoc_v4i bc = assoc_v4i{(int)bu.x, (int)bu.y, (int)bu.z, (int)bu.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) acc_c[t][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_c[t], bc, acc_c[t][j], 0, 0, 0);
          }
        }
      }

      // C/D: column (value column) = lane & 15, row (sample of the tile) = 4 (lane >> 4) + register; the lane's four digit accumulators in i64
      const uint32_t k = 16u * vg + (lane & 15u);
      if (k < A.columns) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const size_t sample = (size_t)sg * kScoreGroupSamples + wave * 64u + (uint32_t)t * 16u + 4u * chunk + (uint32_t)i;
            const size_t o = ((size_t)rb * spad + sample) * A.columns + k;
            A.slab_s[o] = (long long)acc_s[t][0][i] + 256ll * acc_s[t][1][i] + 65536ll * acc_s[t][2][i] + 16777216ll * acc_s[t][3][i];
            if constexpr (CALLED)
              A.slab_c[o] = (long long)acc_c[t][0][i] + 256ll * acc_c[t][1][i] + 65536ll * acc_c[t][2][i] + 16777216ll * acc_c[t][3][i];
          }
      }
    }
  }
}

}  // namespace fmh
