// assoc_host.hpp — the host arithmetic fmh_assoc_prepare (assoc.hip) and fmh_logistic_null (logistic_host.hpp) share: sequential sums,
// centring, the twice-over modified Gram-Schmidt, the covariate basis with its drop rule, the fixed-point exponent, and the Student-t tail
// of fmh_assoc_stats, which the mixed-model scan (lmm_host.hpp) shares with the covariate basis.  The operation order
// is include/ferromic_hip.h's (association scan, host preparation, steps 1, 2 and 4); every unit that includes this is built with
// -ffp-contract=off.  Plain C++: no HIP, no library state, so that a stand-alone program can run it under a sanitizer.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace fmh_host {

inline double seq_dot(const double* a, const double* b, size_t n, size_t stride_a, size_t stride_b) {
  double s = 0.0;
  for (size_t i = 0; i < n; ++i) s += a[i * stride_a] * b[i * stride_b];
  return s;
}

// column-major work copy: centred in place
inline void centre(double* x, size_t n) {
  double s = 0.0;
  for (size_t i = 0; i < n; ++i) s += x[i];
  const double mean = s / (double)n;
  for (size_t i = 0; i < n; ++i) x[i] -= mean;
}

// x minus its projections on the `c` orthonormal columns of q, one after the other, the whole pass twice
inline void project_off(double* x, const std::vector<double>& q, size_t c, size_t n) {
  for (int pass = 0; pass < 2; ++pass)
    for (size_t j = 0; j < c; ++j) {
      const double* qj = q.data() + j * n;
      const double d = seq_dot(qj, x, n, 1, 1);
      for (size_t i = 0; i < n; ++i) x[i] -= d * qj[i];
    }
}

// the largest e with max |v| * 2^e <= 2^30; 0 for a column of zeros
inline int fixed_point_exponent(const double* x, size_t n) {
  double mx = 0.0;
  for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(x[i]));
  if (mx == 0.0) return 0;
  int ex = 0;
  const double f = std::frexp(mx, &ex);  // mx = f * 2^ex, f in [0.5, 1)
  return f == 0.5 ? 31 - ex : 30 - ex;
}

// One column x[n] against the kept columns q: orthogonalised in place, then dropped (returns false) or normalised and appended to q.  The
// covariate basis centres the column first; the whitened basis of the logistic null model does not.
inline bool orthonormal_append(double* x, std::vector<double>& q, size_t* c, size_t n) {
  const double r0 = std::sqrt(seq_dot(x, x, n, 1, 1));
  project_off(x, q, *c, n);
  const double r = std::sqrt(seq_dot(x, x, n, 1, 1));
  if (r0 == 0.0 || r <= r0 * 0x1p-26) return false;
  for (size_t i = 0; i < n; ++i) x[i] /= r;
  q.insert(q.end(), x, x + n);
  ++*c;
  return true;
}

// covariates [n][cin] row-major: centre, orthogonalise against the kept columns (modified Gram-Schmidt, twice), drop or normalise.
// q receives the kept columns column-major; returns their number.
inline size_t covariate_basis(const double* covariates, size_t n, size_t cin, std::vector<double>& q, uint8_t* dropped_or_null) {
  std::vector<double> x(n);
  size_t c = 0;
  for (size_t j = 0; j < cin; ++j) {
    for (size_t i = 0; i < n; ++i) x[i] = covariates[i * cin + j];
    centre(x.data(), n);
    const bool kept = orthonormal_append(x.data(), q, &c, n);
    if (dropped_or_null) dropped_or_null[j] = kept ? 0 : 1;
  }
  return c;
}

// V[i * pitch] = (int32) rint(col[i] * 2^e) with e = fixed_point_exponent; the exponent and the exact total
inline void quantise_column(const double* col, size_t n, int32_t* values, size_t pitch, int32_t* exponent, long long* total) {
  const int e = fixed_point_exponent(col, n);
  long long t = 0;
  for (size_t i = 0; i < n; ++i) {
    const int32_t v = (int32_t)std::rint(std::ldexp(col[i], e));
    values[i * pitch] = v;
    t += v;
  }
  *exponent = e;
  *total = t;
}

// ---- the two-sided tail of Student's t: fmh_assoc_stats' p, which the mixed-model statistics (lmm_host.hpp) report with the same bits ----
// the continued fraction of the incomplete beta function (modified Lentz), to a relative change below 1e-15
inline double beta_cf(double a, double b, double x) {
  const double tiny = 1e-300;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (std::fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= 10000; ++m) {
    const double dm = (double)m, m2 = 2.0 * dm;
    double aa = dm * (b - dm) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (std::fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h = h * (d * c);
    aa = -(a + dm) * (qab + dm) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (std::fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (std::fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h = h * del;
    if (std::fabs(del - 1.0) < 1e-15) break;
  }
  return h;
}

// two-sided tail of Student's t: I_x(df / 2, 1 / 2) at x = df / (df + t^2)
inline double student_t_two_sided(double t, double df) {
  const double t2 = t * t;
  if (t2 == 0.0) return 1.0;
  const double x = df / (df + t2), xc = t2 / (df + t2);  // xc = 1 - x without the cancellation
  if (x == 0.0) return 0.0;
  const double a = df / 2.0, b = 0.5;
  const double front = std::exp(std::lgamma(a + b) - std::lgamma(a) - std::lgamma(b) + a * std::log(x) + b * std::log(xc));
  if (x < (a + 1.0) / (a + b + 2.0)) return front * beta_cf(a, b, x) / a;
  return 1.0 - front * beta_cf(b, a, xc) / b;
}


}  // namespace fmh_host
