// clump_host.hpp — the host side of LD clumping (clump.hip): the parameter check, the one f64 formula of genotype r^2 (fmh_geno_ld_r2), the
// participants, candidates and partner ranges of a request (clump_plan), the greedy rule over them (clump_greedy: rule 3 of the definition,
// shared by the device path, which answers `qualifies` from the kernel's threshold bits, and by the twin, which answers it from dosages),
// and the host twins fmh_geno_ld_pairs_host and fmh_clump_host - plain loops over a dosage table: NO bit planes, NO tiles.  The definition
// is include/ferromic_hip.h's (LD clumping).  Plain C++: no HIP, no library state, so that a stand-alone program can run it under a
// sanitizer.  Build with -ffp-contract=off.  A refusal is returned as its message (nullptr = none).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "../../include/ferromic_hip.h"

namespace fmh_host {

constexpr uint32_t kClumpNone = 0xFFFFFFFFu;

inline const char* clump_check_params(const fmh_clump_params& p) {
  if (p.p1 != p.p1 || p.p2 != p.p2 || p.r2 != p.r2) return "a parameter is NaN";
  if (!(0.0 <= p.p1 && p.p1 <= p.p2 && p.p2 <= 1.0)) return "0 <= p1 <= p2 <= 1 is required";
  if (!(0.0 <= p.r2 && p.r2 <= 1.0)) return "0 <= r2 <= 1 is required";
  return nullptr;
}

// the first row of the range whose p is neither NaN nor within [0, 1] (rows with keep == 0 are not looked at), or `count`
inline size_t clump_bad_p(const double* p, const uint8_t* keep_or_null, size_t count) {
  for (size_t r = 0; r < count; ++r)
    if ((!keep_or_null || keep_or_null[r]) && p[r] == p[r] && !(0.0 <= p[r] && p[r] <= 1.0)) return r;
  return count;
}

// THE formula
inline double geno_ld_r2(const fmh_geno_ld_counts& c) {
  const int64_t n = c.n;
  const int64_t cov = n * (int64_t)c.cross - (int64_t)c.sum_a * (int64_t)c.sum_b;
  const int64_t va = n * (int64_t)c.sq_a - (int64_t)c.sum_a * (int64_t)c.sum_a;
  const int64_t vb = n * (int64_t)c.sq_b - (int64_t)c.sum_b * (int64_t)c.sum_b;
  if (va == 0 || vb == 0) return std::numeric_limits<double>::quiet_NaN();
  return ((double)cov * (double)cov) / ((double)va * (double)vb);
}

// the counts of two dosage rows of n samples (0, 1, 2; 3 = not called)
inline fmh_geno_ld_counts geno_ld_counts_host(const uint8_t* a, const uint8_t* b, size_t n) {
  fmh_geno_ld_counts c{};
  for (size_t s = 0; s < n; ++s) {
    if (a[s] > 2 || b[s] > 2) continue;
    const uint32_t ga = a[s], gb = b[s];
    c.n += 1; c.sum_a += ga; c.sum_b += gb; c.sq_a += ga * ga; c.sq_b += gb * gb; c.cross += ga * gb;
  }
  return c;
}

// Rules 1 and 2: the participants (ascending rows of the range), the candidates among them (as participant numbers, ascending), per candidate
// its partner range [lo, hi) in participant numbers - both ends are monotone, two pointers - and the order of the visit (ascending (p, row)).
struct ClumpPlan {
  std::vector<uint32_t> rows;   // [K] participant -> row of the range
  std::vector<uint32_t> x;      // [K] its position
  std::vector<uint32_t> cand;   // [n_cand] candidate -> participant
  std::vector<uint32_t> lo, hi; // [n_cand]
  std::vector<uint32_t> order;  // [n_cand] candidates in the order of the visit
};
inline ClumpPlan clump_plan(const uint8_t* keep_or_null, const uint32_t* x_or_null /* per row of the range */, const double* p, size_t row_count,
                            const fmh_clump_params& P) {
  ClumpPlan plan;
  for (size_t r = 0; r < row_count; ++r) {
    if (keep_or_null && !keep_or_null[r]) continue;
    if (p[r] != p[r] || !(p[r] <= P.p2)) continue;
    if (p[r] <= P.p1) plan.cand.push_back((uint32_t)plan.rows.size());
    plan.rows.push_back((uint32_t)r);
    plan.x.push_back(x_or_null ? x_or_null[r] : (uint32_t)r);
  }
  const size_t K = plan.rows.size(), n_cand = plan.cand.size();
  plan.lo.resize(n_cand); plan.hi.resize(n_cand); plan.order.resize(n_cand);
  size_t lo = 0, hi = 0;
  for (size_t c = 0; c < n_cand; ++c) {
    const uint64_t xi = plan.x[plan.cand[c]];
    while (lo < K && (uint64_t)plan.x[lo] + P.window < xi) ++lo;
    while (hi < K && (uint64_t)plan.x[hi] <= xi + P.window) ++hi;
    plan.lo[c] = (uint32_t)lo; plan.hi[c] = (uint32_t)hi; plan.order[c] = (uint32_t)c;
  }
  std::sort(plan.order.begin(), plan.order.end(), [&](uint32_t a, uint32_t b) {
    const double pa = p[plan.rows[plan.cand[a]]], pb = p[plan.rows[plan.cand[b]]];
    return pa < pb || (pa == pb && a < b);
  });
  return plan;
}

// Rule 3.  qualifies(c, j): r2(candidate c, participant j) >= r2, asked only for j inside [lo, hi) of c, j != the candidate, not yet owned.
// owner[j] = the participant number of j's index, kClumpNone for none; `indexes` = the index participants in the order they were chosen.
template <class Q> inline void clump_greedy(const ClumpPlan& plan, Q qualifies, std::vector<uint32_t>& owner, std::vector<uint32_t>& indexes) {
  owner.assign(plan.rows.size(), kClumpNone);
  indexes.clear();
  for (uint32_t c : plan.order) {
    const uint32_t i = plan.cand[c];
    if (owner[i] != kClumpNone) continue;
    owner[i] = i;
    indexes.push_back(i);
    for (uint32_t j = plan.lo[c]; j < plan.hi[c]; ++j)
      if (j != i && owner[j] == kClumpNone && qualifies(c, j)) owner[j] = i;
  }
}

// the outputs of an empty answer: no clump anywhere
inline void clump_fill_none(size_t row_count, uint32_t* index_of, double* r2_or_null, uint64_t* n_clumps_or_null) {
  for (size_t r = 0; r < row_count; ++r) {
    index_of[r] = kClumpNone;
    if (r2_or_null) r2_or_null[r] = std::numeric_limits<double>::quiet_NaN();
  }
  if (n_clumps_or_null) *n_clumps_or_null = 0;
}

// owner (participants) -> h_index_of (rows of the range); the rows' r2 are written by the caller
inline void clump_write_owners(const ClumpPlan& plan, const std::vector<uint32_t>& owner, uint32_t* index_of) {
  for (size_t j = 0; j < owner.size(); ++j)
    if (owner[j] != kClumpNone) index_of[plan.rows[j]] = plan.rows[owner[j]];
}

inline void geno_ld_pairs_host(const uint8_t* dosage, size_t n, const uint32_t* rows_a, const uint32_t* rows_b, size_t P, fmh_geno_ld_counts* out) {
  for (size_t i = 0; i < P; ++i) out[i] = geno_ld_counts_host(dosage + (size_t)rows_a[i] * n, dosage + (size_t)rows_b[i] * n, n);
}

// the twin: every given row is kept, rows are 0 .. K - 1
inline void clump_host(const uint8_t* dosage, const uint32_t* x_or_null, const double* p, size_t K, size_t n, const fmh_clump_params& P, uint32_t* index_of,
                       double* r2_or_null, uint64_t* n_clumps_or_null) {
  clump_fill_none(K, index_of, r2_or_null, n_clumps_or_null);
  const ClumpPlan plan = clump_plan(nullptr, x_or_null, p, K, P);
  std::vector<uint32_t> owner, indexes;
  auto r2_of = [&](uint32_t i, uint32_t j) {
    return geno_ld_r2(geno_ld_counts_host(dosage + (size_t)plan.rows[i] * n, dosage + (size_t)plan.rows[j] * n, n));
  };
  clump_greedy(plan, [&](uint32_t c, uint32_t j) { return r2_of(plan.cand[c], j) >= P.r2; }, owner, indexes);
  clump_write_owners(plan, owner, index_of);
  if (r2_or_null)
    for (size_t j = 0; j < owner.size(); ++j)
      if (owner[j] != kClumpNone) r2_or_null[plan.rows[j]] = r2_of(owner[j], (uint32_t)j);
  if (n_clumps_or_null) *n_clumps_or_null = indexes.size();
}

}  // namespace fmh_host
