// segment_host_check.hpp — what roh_host_check.cpp and ibd_host_check.cpp run before their own cohort: the kept rows and the break bitmap
// of segment_host.hpp against their definition, read row by row, on exact-size heap blocks.  Every bit of the bitmap is read, so a bit the
// definition does not set - in the padding a layout promises as much as between the rows - fails the check.  Silent when all is well.
#pragma once

#include <cstdio>
#include <vector>

#include "segment_host.hpp"

namespace fmh_host {

// bit_offset and n_words(K) are the statistic's layout; false (and a line on stderr) at the first disagreement
template <class Words>
inline bool check_kept_rows_and_breaks(size_t bit_offset, Words n_words) {
  const size_t row_begin = 3;  // positions are indexed by matrix row
  for (size_t K : {0, 1, 63, 64, 65, 128, 129})
    for (int masked = 0; masked < 2; ++masked)
      for (uint32_t max_gap : {0u, 1u}) {
        // masked: every third row of the range is dropped; the positions step by 0 to 4 between kept rows, so max_gap 1 breaks some
        std::vector<uint8_t> keep;
        std::vector<uint32_t> rows, x, positions(row_begin);
        for (size_t r = 0; rows.size() < K; ++r) {
          positions.push_back((uint32_t)(r + r / 2 + (r * 7 % 5 == 0)));
          if (masked) keep.push_back(r % 3 != 1);
          if (masked && r % 3 == 1) continue;
          rows.push_back((uint32_t)r);
          x.push_back(positions.back());
        }
        const KeptRows kept = kept_rows(masked ? keep.data() : nullptr, positions.data(), row_begin, positions.size() - row_begin);
        const std::vector<unsigned long long> brk = break_bitmap(kept.x, max_gap, bit_offset, n_words(K));
        bool ok = kept.rows == rows && kept.x == x && brk.size() == n_words(K);
        for (size_t bit = 0; ok && bit < 64 * brk.size(); ++bit) {
          const size_t k = bit - bit_offset;  // wraps below the offset: no row then
          const bool want = bit >= bit_offset && k >= 1 && k < K && max_gap > 0 && x[k] - x[k - 1] > max_gap;
          ok = (((brk[bit >> 6] >> (bit & 63)) & 1ull) != 0) == want;
        }
        if (!ok) {
          fprintf(stderr, "kept_rows / break_bitmap: K %zu, masked %d, max_gap %u, bit offset %zu disagree with their definition\n", K, masked, max_gap, bit_offset);
          return false;
        }
      }
  return true;
}

}  // namespace fmh_host
