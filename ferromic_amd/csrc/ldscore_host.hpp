// ldscore_host.hpp — the host side of the LD scores (ldscore.hip): the pair term (ld_score_term: r^2 by THE formula of clump_host.hpp, the
// bias correction, the 2^-40 fixed point), the partner ranges of the kept rows by two pointers (ld_score_ranges), the host twin
// fmh_ld_scores_host - plain loops over pairs of a dosage table: NO bit planes, NO tiles, NO symmetry - fmh_ld_score_values, and the LD
// score regression fmh_ldsc_regress with its block jackknife.  The definition is include/ferromic_hip.h's (LD scores and LD score
// regression).  Plain C++: no HIP, no library state, so that a stand-alone program can run it under a sanitizer.  Build with
// -ffp-contract=off.  A refusal is returned as its message (nullptr = none).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "../../include/ferromic_hip.h"
#include "clump_host.hpp"

namespace fmh_host {

constexpr uint32_t kLdScoreMaxPartners = 1u << 22;  // |q| < 2^41 per term: |Q| < 2^63

inline const char* ld_score_check_params(const fmh_ldscore_params& p) {
  if (p.flags & ~FMH_LDSCORE_ADJUST) return "flags other than 0 or FMH_LDSCORE_ADJUST";
  return nullptr;
}

// the pair term: false = skipped
inline bool ld_score_term(const fmh_geno_ld_counts& c, bool adjust, int64_t* q) {
  const double r2 = geno_ld_r2(c);
  if (r2 != r2) return false;
  double t = r2;
  if (adjust) {
    if (c.n < 3) return false;
    t = r2 - (1.0 - r2) / (double)(c.n - 2);
  }
  *q = (int64_t)llrint(ldexp(t, 40));
  return true;
}

// per row k of K rows with non-decreasing x: the rows j with |x_j - x_k| <= window are [lo[k], hi[k]); both ends are monotone
inline void ld_score_ranges(const std::vector<uint32_t>& x, uint32_t window, std::vector<uint32_t>& lo, std::vector<uint32_t>& hi) {
  const size_t K = x.size();
  lo.resize(K); hi.resize(K);
  size_t l = 0, h = 0;
  for (size_t k = 0; k < K; ++k) {
    const uint64_t xk = x[k];
    while (l < K && (uint64_t)x[l] + window < xk) ++l;
    while (h < K && (uint64_t)x[h] <= xk + window) ++h;
    lo[k] = (uint32_t)l; hi[k] = (uint32_t)h;
  }
}

// the first row with more than kLdScoreMaxPartners partners, or K
inline size_t ld_score_crowded_row(const std::vector<uint32_t>& lo, const std::vector<uint32_t>& hi) {
  for (size_t k = 0; k < lo.size(); ++k)
    if (hi[k] - lo[k] > kLdScoreMaxPartners) return k;
  return lo.size();
}

// the twin: every given row is kept, rows are 0 .. K - 1; every ordered pair of the window is computed on its own
inline void ld_scores_host(const uint8_t* dosage, const uint32_t* x_or_null, size_t K, size_t n, const fmh_ldscore_params& P, int64_t* q_out,
                           uint32_t* partners_or_null, uint32_t* counted) {
  const bool adjust = P.flags & FMH_LDSCORE_ADJUST;
  for (size_t i = 0; i < K; ++i) {
    const int64_t xi = x_or_null ? (int64_t)x_or_null[i] : (int64_t)i;
    int64_t Q = 0;
    uint32_t partners = 0, used = 0;
    for (size_t j = 0; j < K; ++j) {
      const int64_t xj = x_or_null ? (int64_t)x_or_null[j] : (int64_t)j;
      const int64_t gap = xj > xi ? xj - xi : xi - xj;
      if (gap > (int64_t)P.window) continue;
      ++partners;
      int64_t q = 0;
      if (!ld_score_term(geno_ld_counts_host(dosage + i * n, dosage + j * n, n), adjust, &q)) continue;
      ++used;
      Q += q;
    }
    q_out[i] = Q;
    counted[i] = used;
    if (partners_or_null) partners_or_null[i] = partners;
  }
}

inline void ld_score_values(const int64_t* q, const uint32_t* counted, size_t K, double* score) {
  for (size_t k = 0; k < K; ++k) score[k] = counted[k] ? (double)q[k] * 0x1p-40 : std::numeric_limits<double>::quiet_NaN();
}

// ---- LD score regression ----------------------------------------------------------------------------------------------------------------------
struct LdscSums { double w = 0.0, x = 0.0, xx = 0.0, y = 0.0, xy = 0.0; };
inline void ldsc_add(LdscSums& s, const LdscSums& b) { s.w += b.w; s.x += b.x; s.xx += b.xx; s.y += b.y; s.xy += b.xy; }
inline void ldsc_solve(const LdscSums& s, bool fixed, double* a, double* h) {
  if (fixed) { *h = (s.xy - *a * s.x) / s.xx; return; }
  const double det = s.w * s.xx - s.x * s.x;
  *h = (s.w * s.xy - s.x * s.y) / det;
  *a = (s.xx * s.y - s.x * s.xy) / det;
}
inline double ldsc_se(const std::vector<double>& pseudo) {
  const size_t B = pseudo.size();
  double mean = 0.0, ss = 0.0;
  for (double v : pseudo) mean += v;
  mean /= (double)B;
  for (double v : pseudo) ss += (v - mean) * (v - mean);
  return sqrt(ss / (double)(B - 1) / (double)B);
}

inline const char* ldsc_regress(const double* chi2, const double* score, const double* w_score_or_null, size_t K, double N, double M, uint64_t blocks,
                                const double* fixed_or_null, fmh_ldsc_out* out) {
  if (!std::isfinite(N) || !std::isfinite(M) || !(N > 0.0) || !(M > 0.0)) return "N and M must be finite and above 0";
  if (fixed_or_null && !std::isfinite(*fixed_or_null)) return "the fixed intercept is not finite";
  if (blocks < 2) return "at least 2 blocks are required";
  const bool fixed = fixed_or_null != nullptr;
  std::vector<double> y, l, lw;
  for (size_t k = 0; k < K; ++k) {
    const double w = w_score_or_null ? w_score_or_null[k] : score[k];
    if (!std::isfinite(chi2[k]) || !std::isfinite(score[k]) || !std::isfinite(w)) continue;
    y.push_back(chi2[k]); l.push_back(score[k]); lw.push_back(w);
  }
  const size_t U = y.size(), B = (size_t)std::min<uint64_t>(blocks, U), P = fixed ? 1 : 2;
  if (B < 2 || U < 2 * P * B) return "fewer than 2 used sites per fitted parameter and block";
  for (size_t i = 0; i < U; ++i)
    if (y[i] < 0.0) return "a chi2 is negative";

  double sum_y = 0.0, sum_l = 0.0;
  for (size_t i = 0; i < U; ++i) { sum_y += y[i]; sum_l += l[i]; }
  const double mean_y = sum_y / (double)U, mean_l = sum_l / (double)U;
  double a = fixed ? *fixed_or_null : 1.0;
  double h = M * (mean_y - 1.0) / (N * mean_l);
  std::vector<double> x(U), w(U);
  for (size_t i = 0; i < U; ++i) x[i] = N * l[i] / M;
  for (int fit = 0; fit < 3; ++fit) {
    const double hc = h < 0.0 ? 0.0 : h > 1.0 ? 1.0 : h;
    LdscSums s;
    for (size_t i = 0; i < U; ++i) {
      const double c = a + ((hc * N) * std::max(l[i], 1.0)) / M;
      w[i] = 1.0 / (std::max(lw[i], 1.0) * (2.0 * (c * c)));
      const double wx = w[i] * x[i];
      s.w += w[i]; s.x += wx; s.xx += wx * x[i]; s.y += w[i] * y[i]; s.xy += wx * y[i];
    }
    ldsc_solve(s, fixed, &a, &h);
  }
  // the jackknife of the last fit, its weights held
  std::vector<LdscSums> block(B);
  for (size_t b = 0; b < B; ++b)
    for (size_t i = b * U / B; i < (b + 1) * U / B; ++i) {
      const double wx = w[i] * x[i];
      block[b].w += w[i]; block[b].x += wx; block[b].xx += wx * x[i]; block[b].y += w[i] * y[i]; block[b].xy += wx * y[i];
    }
  std::vector<double> pseudo_a(B), pseudo_h(B);
  for (size_t b = 0; b < B; ++b) {
    LdscSums s;
    for (size_t o = 0; o < B; ++o)
      if (o != b) ldsc_add(s, block[o]);
    double ab = a, hb = 0.0;
    ldsc_solve(s, fixed, &ab, &hb);
    pseudo_a[b] = (double)B * a - (double)(B - 1) * ab;
    pseudo_h[b] = (double)B * h - (double)(B - 1) * hb;
  }
  std::vector<double> sorted(y);
  std::sort(sorted.begin(), sorted.end());
  const double median = U % 2 ? sorted[U / 2] : (sorted[U / 2 - 1] + sorted[U / 2]) / 2.0;
  out->h2 = h; out->h2_se = ldsc_se(pseudo_h);
  out->intercept = a; out->intercept_se = fixed ? std::numeric_limits<double>::quiet_NaN() : ldsc_se(pseudo_a);
  out->ratio = (a - 1.0) / (mean_y - 1.0);
  out->mean_chi2 = mean_y;
  out->lambda_gc = median / 0.4549364231195724;
  out->n_used = U; out->blocks = B;
  return nullptr;
}

}  // namespace fmh_host
