// score_host.hpp — the host arithmetic of the polygenic score (score.hip: fmh_score_exponents, fmh_score_values, fmh_score_stats) and the
// device bytes one fmh_score_sums call takes, which ferromic.polygenic_score sizes its row chunks by (pymodule_score.inc).  The operation
// order is include/ferromic_hip.h's (polygenic score); every unit that includes this is built with -ffp-contract=off.  Plain C++: no HIP, no
// library state, so that a stand-alone program can run it under a sanitizer.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace fmh_host {

constexpr size_t kScoreMaxColumnsHost = 64;
constexpr size_t kScoreMaxRows = (size_t)1 << 21;  // |S + (T_U - C)| stays below 2^53
constexpr size_t kScoreDefaultItemRows = 4096;
constexpr int kScoreModeMean = 0, kScoreModeCenter = 1, kScoreModeZero = 2;

// rows per work item from the option's value (0 = the default): a multiple of the 64 rows of a matrix instruction, at most 2^21
inline size_t score_item_rows(long long option) {
  const size_t rows = option <= 0 ? kScoreDefaultItemRows : std::min<size_t>((size_t)option, kScoreMaxRows);
  return (rows + 63) / 64 * 64;
}

// the device bytes of one fmh_score_sums call over `rows` rows: the digits of V (and U) and the slabs of S (and C).  `covered` = the last
// selected sample + 1.
inline size_t score_call_bytes(size_t rows, size_t covered, size_t K, size_t item_rows, bool called) {
  const size_t steps = (rows + 63) / 64, vgroups = (K + 15) / 16, blocks = (rows + item_rows - 1) / item_rows;
  const size_t spad = (covered + 255) / 256 * 256;
  return (steps * vgroups * 4096 + blocks * spad * K * sizeof(long long)) * (called ? 2 : 1);
}

// the largest e with 2 * mx * 2^e <= 2^30, mx > 0 finite: mx = f * 2^x with f in [0.5, 1) gives 30 - x when f == 0.5, else 29 - x (the rule of
// fixed_point_exponent, assoc_host.hpp, at 2 * mx - without forming the product, which may overflow)
inline int score_exponent(double mx) {
  if (mx == 0.0) return 0;
  int ex = 0;
  const double f = std::frexp(mx, &ex);
  return f == 0.5 ? 30 - ex : 29 - ex;
}

}  // namespace fmh_host
