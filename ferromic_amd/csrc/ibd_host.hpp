// ibd_host.hpp — the host side of the IBD segments (ibd.hip): the parameter check fmh_ibd_scan and fmh_ibd_scan_host share, the rule that
// sizes the row blocks, the segment order (fmh_ibd_sort_segments) and the host twin of the scan (fmh_ibd_scan_host) - a serial loop per
// pair over the whole range, one kept row at a time: NO words, NO blocks and NO stitch, so that it checks the device's decomposition
// instead of repeating it.  The definition is include/ferromic_hip.h's (IBD segments).  Plain C++: no HIP, no library state, so that a
// stand-alone program can run it under a sanitizer.  A refusal is returned as its message (nullptr = none).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/ferromic_hip.h"
#include "segment_host.hpp"

namespace fmh_host {

constexpr size_t kIbdItemsPerWorkgroup = 4;  // the default row blocks give every workgroup of the grid this many items

inline const char* ibd_check_params(const fmh_ibd_params& p) {
  if (p.mode != FMH_IBD1 && p.mode != FMH_IBD2) return "mode is neither FMH_IBD1 nor FMH_IBD2";
  return nullptr;
}

// Kept rows per row block, a multiple of 64.  `option` > 0 forces it (rounded up).  Otherwise one block when the `tiles` pair tiles alone
// give each of the `grid` workgroups kIbdItemsPerWorkgroup items, else as many equal blocks as reach that - but never more blocks than
// `max_blocks` (what the budget leaves for the block records; >= 1).
inline size_t ibd_item_rows(long long option, size_t K, size_t tiles, size_t grid, size_t max_blocks) {
  const size_t words = (K + 63) / 64;
  if (option > 0) return (std::min<size_t>((size_t)option, (size_t)1 << 30) + 63) / 64 * 64;
  size_t blocks = (kIbdItemsPerWorkgroup * grid + tiles - 1) / std::max<size_t>(tiles, 1);
  blocks = std::max<size_t>(1, std::min({blocks, max_blocks, std::max<size_t>(words, 1)}));
  return std::max<size_t>(1, (words + blocks - 1) / blocks) * 64;
}

inline bool ibd_segment_less(const fmh_ibd_segment& s, const fmh_ibd_segment& t) {
  if (s.a != t.a) return s.a < t.a;
  if (s.b != t.b) return s.b < t.b;
  return s.first_row < t.first_row;
}

// 0 CONC, 1 MISS, 2 DISC of two dosages (3 = not called)
inline int ibd_state(uint32_t mode, uint8_t di, uint8_t dj) {
  if (di > 2 || dj > 2) return 1;
  const bool disc = mode == FMH_IBD1 ? (di + dj == 2 && di != dj) : di != dj;
  return disc ? 2 : 0;
}

// The host twin.  Every check but the NULL ones of the entry point is the caller's (ibd.hip); the tables may be null.
inline void ibd_scan_host(const uint8_t* dosage, const uint32_t* x_or_null, size_t K, size_t n, const fmh_ibd_params& p, const fmh_ibd_out& out,
                          fmh_ibd_segment* segments, size_t capacity, uint64_t* count_out) {
  uint64_t count = 0;
  auto x = [&](size_t k) { return x_or_null ? x_or_null[k] : (uint32_t)k; };
  auto put = [&](unsigned long long* t, size_t i, size_t j, uint64_t v) {
    if (t) t[i * n + j] = t[j * n + i] = v;
  };
  for (size_t i = 0; i < n; ++i) {
    put(out.d_n_segments, i, i, 0); put(out.d_sum_sites, i, i, 0); put(out.d_sum_length, i, i, 0); put(out.d_longest_length, i, i, 0);
    for (size_t j = i + 1; j < n; ++j) {
      uint64_t n_segments = 0, sum_sites = 0, sum_length = 0, longest = 0, n_missing = 0;
      bool open = false;
      size_t first = 0;
      auto close = [&](size_t last) {
        const uint64_t sites = last - first + 1, length = (uint64_t)x(last) - x(first) + 1;
        if (run_qualifies(p, sites, length, n_missing)) {
          ++n_segments; sum_sites += sites; sum_length += length; longest = std::max(longest, length);
          if (count < capacity && segments) segments[count] = fmh_ibd_segment{(uint32_t)i, (uint32_t)j, (uint32_t)sites, (uint32_t)n_missing, first, last};
          ++count;
        }
        open = false;
      };
      for (size_t k = 0; k < K; ++k) {
        const int state = ibd_state(p.mode, dosage[k * n + i], dosage[k * n + j]);
        if (open && (state == 2 || (p.max_gap > 0 && x(k) - x(k - 1) > p.max_gap))) close(k - 1);
        if (state != 2) {
          if (!open) { open = true; first = k; n_missing = 0; }
          n_missing += state == 1;
        }
      }
      if (open) close(K - 1);
      put(out.d_n_segments, i, j, n_segments); put(out.d_sum_sites, i, j, sum_sites);
      put(out.d_sum_length, i, j, sum_length); put(out.d_longest_length, i, j, longest);
    }
  }
  if (count_out) *count_out = count;
}

}  // namespace fmh_host
