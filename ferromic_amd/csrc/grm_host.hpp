// grm_host.hpp — the host arithmetic of the genomic relationship matrix (grm.hip): per-row values from the exact counts (grm_values), the
// matrix from the products (grm_finish), the twin that sums the products from a dosage table (grm_host) and the sign rule of an
// eigenvector (grm_fix_sign).  The definition is include/ferromic_hip.h's (genomic relationship matrix); every f64 is formed from the
// integers in the operation order written there, so that numpy reproduces the bits.  Plain C++: no HIP, no library state, so that a
// stand-alone program can run it under a sanitizer.  Build with -ffp-contract=off.  A refusal is returned as its message (nullptr = none).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <limits>
#include <vector>

#include "../../include/ferromic_hip.h"

namespace fmh_host {

inline const char* grm_check_params(const fmh_grm_params& p) {
  if (p.method != FMH_GRM_STANDARDIZED && p.method != FMH_GRM_CENTERED) return "method is neither FMH_GRM_STANDARDIZED nor FMH_GRM_CENTERED";
  if (p.denominator != FMH_GRM_SITES && p.denominator != FMH_GRM_PAIRS) return "denominator is neither FMH_GRM_SITES nor FMH_GRM_PAIRS";
  if (p.denominator == FMH_GRM_PAIRS && p.method != FMH_GRM_STANDARDIZED) return "denominator FMH_GRM_PAIRS takes method FMH_GRM_STANDARDIZED only";
  return nullptr;
}

inline bool grm_usable(uint32_t c, uint32_t a) { return c >= 1 && a > 0 && (uint64_t)a < 2 * (uint64_t)c; }

// rows in, per row: usable, p (NaN where c == 0), z[3] (zeros on a row that is not usable); *scale = sum over the usable rows, ascending,
// of 2 p (1 - p); *n_usable their number.  Every output may be null.
inline void grm_values(const uint32_t* c, const uint32_t* a, size_t rows, uint32_t method, uint8_t* usable, double* p_out, double* z, double* scale,
                       uint64_t* n_usable) {
  double sum = 0.0;
  uint64_t count = 0;
  for (size_t k = 0; k < rows; ++k) {
    const bool use = grm_usable(c[k], a[k]);
    const double p = c[k] == 0 ? std::numeric_limits<double>::quiet_NaN() : (double)a[k] / (double)(2 * (uint64_t)c[k]);
    double z0 = 0.0, z1 = 0.0, z2 = 0.0;
    if (use) {
      const double mean = 2.0 * p, var = mean * (1.0 - p);
      z0 = 0.0 - mean; z1 = 1.0 - mean; z2 = 2.0 - mean;
      if (method == FMH_GRM_STANDARDIZED) {
        const double sd = std::sqrt(var);
        z0 = z0 / sd; z1 = z1 / sd; z2 = z2 / sd;
      }
      sum = sum + var;
      ++count;
    }
    if (usable) usable[k] = use ? 1 : 0;
    if (p_out) p_out[k] = p;
    if (z) { z[3 * k] = z0; z[3 * k + 1] = z1; z[3 * k + 2] = z2; }
  }
  if (scale) *scale = sum;
  if (n_usable) *n_usable = count;
}

// A from S (and N for FMH_GRM_PAIRS)
inline void grm_finish(const double* S, const uint64_t* N, size_t n, const fmh_grm_params& P, uint64_t n_usable, double scale, double* A) {
  const double denom = P.method == FMH_GRM_STANDARDIZED ? (double)n_usable : scale;
  for (size_t e = 0; e < n * n; ++e) {
    if (P.denominator == FMH_GRM_PAIRS) A[e] = N[e] == 0 ? std::numeric_limits<double>::quiet_NaN() : S[e] / (double)N[e];
    else A[e] = S[e] / denom;
  }
}

// S[n][n] WRITTEN from dosage[K][n] (0, 1, 2; above 2 = not called): the counts, the values, then every entry summed over ascending k
inline void grm_host(const uint8_t* dosage, size_t K, size_t n, uint32_t method, double* S, uint64_t* N_or_null, uint64_t* n_usable, double* scale) {
  std::vector<uint32_t> c(K, 0), a(K, 0);
  for (size_t k = 0; k < K; ++k)
    for (size_t s = 0; s < n; ++s)
      if (dosage[k * n + s] <= 2) { ++c[k]; a[k] += dosage[k * n + s]; }
  std::vector<double> z(3 * K + 1);
  std::vector<uint8_t> usable(K + 1);
  grm_values(c.data(), a.data(), K, method, usable.data(), nullptr, z.data(), scale, n_usable);
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) {
      double sum = 0.0;
      uint64_t both = 0;
      for (size_t k = 0; k < K; ++k) {
        const uint8_t gi = dosage[k * n + i], gj = dosage[k * n + j];
        if (!usable[k] || gi > 2 || gj > 2) continue;
        sum = sum + z[3 * k + gi] * z[3 * k + gj];
        ++both;
      }
      S[i * n + j] = sum;
      if (N_or_null) N_or_null[i * n + j] = both;
    }
}

// the sign rule: the component of the largest magnitude is positive, on a tie the one of the lowest index
inline void grm_fix_sign(double* v, size_t n, size_t stride) {
  size_t at = 0;
  for (size_t i = 1; i < n; ++i)
    if (std::fabs(v[i * stride]) > std::fabs(v[at * stride])) at = i;
  if (n && v[at * stride] < 0.0)
    for (size_t i = 0; i < n; ++i) v[i * stride] = -v[i * stride];
}

}  // namespace fmh_host
