// segment_host.hpp — the host arithmetic the segment statistics share (runs of homozygosity: roh.hip, roh_host.hpp; IBD segments: ibd.hip,
// ibd_host.hpp): the kept rows of a range and their positions, the break bitmap the kernels read, and the rule a run qualifies by - the
// one definition the kernels use too (segment_kernels.hpp).  Plain C++: no HIP, no library state, so that a stand-alone program can run
// it under a sanitizer.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#define FMH_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define FMH_HOST_DEVICE inline
#endif

namespace fmh_host {

// the kept rows of a range of row_count rows, relative to its first row, and their positions x (without positions: the row itself).
// `positions` is indexed by matrix row: the range starts at positions[row_begin].
struct KeptRows {
  std::vector<uint32_t> rows, x;
};
inline KeptRows kept_rows(const uint8_t* keep_or_null, const uint32_t* positions_or_null, size_t row_begin, size_t row_count) {
  KeptRows kept;
  kept.rows.reserve(row_count);
  for (size_t r = 0; r < row_count; ++r)
    if (!keep_or_null || keep_or_null[r]) kept.rows.push_back((uint32_t)r);
  kept.x.resize(kept.rows.size());
  for (size_t k = 0; k < kept.rows.size(); ++k) kept.x[k] = positions_or_null ? positions_or_null[row_begin + kept.rows[k]] : kept.rows[k];
  return kept;
}

// break(k) - a run does not continue from kept row k - 1 to k: max_gap > 0 and x[k] - x[k - 1] > max_gap - at bit k + bit_offset of
// `n_words` words (>= ceil((K + bit_offset) / 64)); every other bit is zero
inline std::vector<unsigned long long> break_bitmap(const std::vector<uint32_t>& x, uint32_t max_gap, size_t bit_offset, size_t n_words) {
  std::vector<unsigned long long> brk(n_words, 0ull);
  if (max_gap > 0)
    for (size_t k = 1; k < x.size(); ++k)
      if (x[k] - x[k - 1] > max_gap) brk[(k + bit_offset) >> 6] |= 1ull << ((k + bit_offset) & 63);
  return brk;
}

// whether a run of n_sites kept rows over `length` positions with n_missing missing calls is a segment; Params is fmh_roh_params or
// fmh_ibd_params.  A statistic that also limits the heterozygous calls of a run (ROH) passes their number and its limit.
template <class Params>
FMH_HOST_DEVICE bool run_qualifies(const Params& p, uint64_t n_sites, uint64_t length, uint64_t n_missing, uint64_t n_het = 0, uint32_t max_het = 0xFFFFFFFFu) {
  return n_sites >= p.min_sites && length >= p.min_length && n_het <= max_het && n_missing <= p.max_missing &&
         (p.max_bp_per_site == 0 || length <= (uint64_t)p.max_bp_per_site * n_sites);
}

}  // namespace fmh_host
