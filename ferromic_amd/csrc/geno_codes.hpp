// geno_codes.hpp — the 2-bit genotype codes of a list of rows as a sample-major bit image: what the relationship matrix (grm.hip) and the
// admixture handle (admix.hip) read their genotypes from.  Moved unchanged from grm_kernels.hpp.
//
// Codes (grm_codes_kernel).  code[plane][w][sample]: one u64 per (word w of 64 listed rows, selected sample at its list position), two planes,
// the sample fastest and padded to `spad`, w padded as the caller needs.  Code of a genotype = bit of plane 0 + 2 * bit of plane 1:
// 0 hom-ref, 1 het, 2 hom-alt, 3 not called.  The fetch is the segment statistics' (segment_kernels.hpp: plane_fetch, PlaneFields, the
// per-row plane flags, the rank table): an item = (word, group of 256 matrix samples), 16 bytes per thread and plane, the 2-bit fields parked
// in LDS, a lane then gathers ITS sample's bit of the 64 rows.  Rows past the list read as not called; the words of the padding samples and of
// the padding words are whatever the host left there.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plane_rows.hpp"
#include "segment_kernels.hpp"

namespace fmh {

constexpr uint32_t kGrmCodeThreads = 256;

struct GrmCodeArgs : PlaneRows {  // the packed image first (plane_rows.hpp)
  uint32_t nvec;    // 16-byte vectors of a row through the last selected sample (<= plane_pitch / 16)
  uint32_t groups;  // sample groups: ceil(nvec / 4)
  size_t row_begin;
  const uint32_t* rows;   // [K] listed rows, relative to row_begin
  const uint8_t* flags;   // [K] plane flags (plane_flags_kernel); null = the matrix has neither a called nor an upper plane
  const uint32_t* rank;   // [groups * 256] list position of a matrix sample, kSegNone where it is not selected
  uint32_t K, words;      // words = ceil(K / 64): the words that hold a listed row
  uint64_t n_items;       // words * groups
  size_t spad;            // samples of the image
  size_t plane_words;     // u64 words of a plane: (padded words) * spad
  unsigned long long* code;  // [2][padded words][spad]
};

// Launched with kGrmCodeThreads threads; static LDS: 2 x 4 KiB of fields.
static __global__ __launch_bounds__(kGrmCodeThreads) void grm_codes_kernel(const GrmCodeArgs A) {
  __shared__ uint4 s_lo4[64 * 4];  // [row of the word][16-byte part]: a row's 16 words of 2-bit fields
  __shared__ uint4 s_hi4[64 * 4];
  const uint32_t* s_lo = reinterpret_cast<const uint32_t*>(s_lo4);
  const uint32_t* s_hi = reinterpret_cast<const uint32_t*>(s_hi4);
  const uint32_t tid = threadIdx.x;
  const uint32_t srow = tid >> 2, spart = tid & 3u;          // the staging thread's row of the word and 16-byte part of the group's 64 bytes
  const uint32_t word = tid >> 4, shift = 2u * (tid & 15u);  // the gathering lane's word of a row's 16 and its field in it
  for (uint64_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
    const uint32_t w = (uint32_t)(it / A.groups), sg = (uint32_t)(it % A.groups);
    const uint64_t k = (uint64_t)w * 64 + srow;
    const uint32_t kk = k < A.K ? (uint32_t)k : A.K - 1;
    const uint32_t row = A.rows[kk], fl = A.flags ? (uint32_t)A.flags[kk] : 0u;
    const uint32_t vec = 4u * sg + spart;
    const bool inside = vec < A.nvec;  // a vector past the covered samples is not called
    const bool ok = inside && k < A.K;
    const size_t off = (A.row_begin + row) * A.plane_pitch + (size_t)(inside ? vec : 0) * 16;
    const PlaneFields f(plane_fetch(A, off, ok, fl));
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t cal = f.called(q), uncalled = ~cal & kEvenBits;
      lo[q] = uncalled | (cal & (f.b[q] ^ (f.b[q] >> 1)));  // het
      hi[q] = uncalled | (cal & f.b[q] & (f.b[q] >> 1));    // hom-alt
    }
    __syncthreads();  // every lane has gathered the item before this one
    s_lo4[tid] = make_uint4(lo[0], lo[1], lo[2], lo[3]);  // tid = srow * 4 + spart
    s_hi4[tid] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    __syncthreads();
    const uint32_t rank = A.rank[(size_t)sg * kSegGroupSamples + tid];
    if (rank == kSegNone) continue;
    uint64_t lm = 0, hm = 0;
#pragma unroll
    for (uint32_t i = 0; i < 64; ++i) {
      lm |= (uint64_t)((s_lo[i * 16u + word] >> shift) & 1u) << i;
      hm |= (uint64_t)((s_hi[i * 16u + word] >> shift) & 1u) << i;
    }
    unsigned long long* t = A.code + (size_t)w * A.spad + rank;
    t[0] = lm;
    t[A.plane_words] = hm;
  }
}

}  // namespace fmh
