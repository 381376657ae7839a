// geno_ld_call.hpp — what the host entry points of the genotype-LD statistics share (clump.hip, ldscore.hip): the column mask of the selected
// samples, the refusal of a matrix that is not diploid or not packed, and the grid of the wave-per-item kernels of clump_kernels.hpp.
#pragma once

#include <algorithm>
#include <vector>

#include "clump_kernels.hpp"
#include "stat_call.hpp"

namespace fmhi {

// both bits of every selected sample, one u32 per 16 samples over the whole pitch, and the 16-byte vectors the samples lie in
struct ColumnMask {
  std::vector<uint32_t> words;
  uint32_t vec0 = 0, vec1 = 0;
};
inline ColumnMask column_mask(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n) {
  ColumnMask out;
  out.words.assign(m->plane_pitch / 4, 0u);
  for (size_t i = 0; i < n; ++i) {
    const size_t s = h_samples_or_null ? h_samples_or_null[i] : i;
    out.words[s / 16] |= 3u << (2 * (s % 16));
  }
  const size_t first = h_samples_or_null ? h_samples_or_null[0] : 0, last = h_samples_or_null ? h_samples_or_null[n - 1] : n - 1;
  out.vec0 = (uint32_t)(first / 64);
  out.vec1 = (uint32_t)(last / 64 + 1);  // within the row: sample `last` exists
  return out;
}

inline int check_genotype_matrix(const fmh_matrix* m, const char* who) {
  if (m->ploidy != 2) return fail(FMH_ERR_UNSUPPORTED, "%s diploid genotypes (ploidy 2), got ploidy %zu", who, m->ploidy);
  return check_packed(m, "genotype LD reads");
}

// workgroups of the two wave-per-item kernels (no LDS): four items per workgroup and round, at most eight workgroups per CU
inline size_t wave_grid(size_t n_items, int cus) {
  return std::max<size_t>(1, std::min<size_t>((n_items + fmh::kClumpThreads / 64 - 1) / (fmh::kClumpThreads / 64), (size_t)std::max(cus, 1) * 8));
}

}  // namespace fmhi
