// roh_host.hpp — the host side of the runs of homozygosity (roh.hip): the parameter checks fmh_roh_scan and fmh_roh_scan_host share, the
// `need` table (fmh_roh_need), the segment order (fmh_roh_sort_segments) and the host twin of the scan (fmh_roh_scan_host) - a serial state
// machine over the whole range of one sample at a time, NOT the device's block / stitch scheme, so that it checks the decomposition instead
// of repeating it.  The definition is include/ferromic_hip.h's (runs of homozygosity).  Plain C++: no HIP, no library state, so that a
// stand-alone program can run it under a sanitizer.  A refusal is returned as its message (nullptr = none).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/ferromic_hip.h"
#include "segment_host.hpp"

namespace fmh_host {

constexpr size_t kRohDefaultItemRows = 4096;
constexpr uint32_t kRohMaxWindow = 64, kRohMaxBins = 8;

// kept rows per work item from the option's value (0 = the default): a multiple of the 64 kept rows of a step, at most 2^30
inline size_t roh_item_rows(long long option) {
  const size_t rows = option <= 0 ? kRohDefaultItemRows : std::min<size_t>((size_t)option, (size_t)1 << 30);
  return (rows + 63) / 64 * 64;
}

// The break bitmap of the scan kernel (break_bitmap): break(k) at bit k + 64, so that 64 zero bits stand in front, and zero words behind:
// the 64 bits a step of any window reads are two whole words
constexpr size_t kRohBreakOffset = 64;
inline size_t roh_break_words(size_t K, size_t window) { return (K + kRohBreakOffset + 2 * window + 63) / 64 + 2; }

// window and bins of the parameters, in the header's order
inline const char* roh_check_params(const fmh_roh_params& p) {
  if (p.window < 1 || p.window > kRohMaxWindow) return "window is outside 1..64";
  if (p.n_bins > kRohMaxBins) return "n_bins exceeds 8";
  for (uint32_t b = 1; b + 1 < p.n_bins; ++b)
    if (p.bin_edges[b] <= p.bin_edges[b - 1]) return "the bin edges are not strictly ascending";
  return nullptr;
}

inline const char* roh_need(double threshold, uint32_t window, uint8_t* need) {
  if (!need) return "NULL need";
  if (window < 1 || window > kRohMaxWindow) return "window is outside 1..64";
  if (!(threshold >= 0.0 && threshold <= 2.0)) return "threshold is not within 0 .. 2";
  std::fill(need, need + 65, (uint8_t)0);
  for (uint32_t c = 1; c <= window; ++c) {
    const double want = threshold * (double)c;
    uint32_t h = 1;
    while (!((double)h >= want)) ++h;
    need[c] = (uint8_t)h;
  }
  return nullptr;
}

inline bool roh_segment_less(const fmh_roh_segment& a, const fmh_roh_segment& b) {
  return a.sample != b.sample ? a.sample < b.sample : a.first_row < b.first_row;
}

// a run's length, whether it qualifies (rule 8) and its bin
inline uint64_t roh_length(uint32_t x_first, uint32_t x_last) { return (uint64_t)x_last - x_first + 1; }
FMH_HOST_DEVICE bool roh_qualifies(const fmh_roh_params& p, uint64_t n_sites, uint64_t length, uint64_t n_het, uint64_t n_missing) {
  return run_qualifies(p, n_sites, length, n_missing, n_het, p.max_het);
}
inline uint32_t roh_bin(const fmh_roh_params& p, uint64_t length) {
  uint32_t b = 0;
  for (uint32_t e = 0; e + 1 < p.n_bins; ++e) b += p.bin_edges[e] <= length ? 1u : 0u;
  return b;
}

// The host twin.  Every check but the NULL ones of the entry point is the caller's (roh.hip); the tables may be null.
inline void roh_scan_host(const uint8_t* state, const uint32_t* x_or_null, size_t K, size_t n, const fmh_roh_params& p, const fmh_roh_out& out,
                          fmh_roh_segment* segments, size_t capacity, uint64_t* count_out) {
  const size_t W = p.window, nb = p.n_bins;
  uint64_t count = 0;
  auto x = [&](size_t k) { return x_or_null ? x_or_null[k] : (uint32_t)k; };
  std::vector<uint8_t> window_hom, in_run;
  for (size_t i = 0; i < n; ++i) {
    uint64_t n_runs = 0, sum_sites = 0, sum_length = 0, longest = 0, bin_runs[kRohMaxBins] = {}, bin_length[kRohMaxBins] = {};
    if (K >= W) {
      // the windows, by a sliding count
      const size_t T = K - W + 1;
      window_hom.assign(T, 0);
      size_t het = 0, miss = 0;
      for (size_t k = 0; k < K; ++k) {
        het += state[k * n + i] == 1;
        miss += state[k * n + i] == 2;
        if (k >= W) {
          het -= state[(k - W) * n + i] == 1;
          miss -= state[(k - W) * n + i] == 2;
        }
        if (k + 1 >= W) window_hom[k + 1 - W] = het <= p.window_het && miss <= p.window_missing;
      }
      // the rows in a run, by a sliding count of the homozygous windows that cover the row
      in_run.assign(K, 0);
      size_t hom = 0;  // over the windows [lo, hi] of the row before
      size_t lo = 0, hi = 0;
      for (size_t k = 0; k < K; ++k) {
        const size_t nlo = k + 1 >= W ? k + 1 - W : 0, nhi = std::min(k, T - 1);
        if (k == 0) hom = window_hom[0];
        else {
          if (nhi > hi) hom += window_hom[nhi];
          if (nlo > lo) hom -= window_hom[lo];
        }
        lo = nlo; hi = nhi;
        in_run[k] = hom >= p.need[hi - lo + 1];
      }
      // the runs: one pass, a run open or not
      bool open = false;
      size_t first = 0;
      uint64_t n_het = 0, n_missing = 0;
      auto close = [&](size_t last) {
        const uint64_t sites = last - first + 1, length = roh_length(x(first), x(last));
        if (roh_qualifies(p, sites, length, n_het, n_missing)) {
          ++n_runs; sum_sites += sites; sum_length += length; longest = std::max(longest, length);
          if (nb) { const uint32_t b = roh_bin(p, length); ++bin_runs[b]; bin_length[b] += length; }
          if (count < capacity && segments) segments[count] = fmh_roh_segment{(uint32_t)i, (uint32_t)sites, (uint32_t)n_het, (uint32_t)n_missing, first, last};
          ++count;
        }
        open = false;
      };
      for (size_t k = 0; k < K; ++k) {
        if (open && (!in_run[k] || (p.max_gap > 0 && x(k) - x(k - 1) > p.max_gap))) close(k - 1);
        if (in_run[k]) {
          if (!open) { open = true; first = k; n_het = n_missing = 0; }
          n_het += state[k * n + i] == 1;
          n_missing += state[k * n + i] == 2;
        }
      }
      if (open) close(K - 1);
    }
    if (out.d_n_runs) out.d_n_runs[i] = n_runs;
    if (out.d_sum_sites) out.d_sum_sites[i] = sum_sites;
    if (out.d_sum_length) out.d_sum_length[i] = sum_length;
    if (out.d_longest_length) out.d_longest_length[i] = longest;
    for (size_t b = 0; b < nb; ++b) {
      if (out.d_bin_runs) out.d_bin_runs[i * nb + b] = bin_runs[b];
      if (out.d_bin_length) out.d_bin_length[i * nb + b] = bin_length[b];
    }
  }
  if (count_out) *count_out = count;
}

}  // namespace fmh_host
