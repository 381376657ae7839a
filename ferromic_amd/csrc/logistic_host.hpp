// logistic_host.hpp — the arithmetic of the logistic association scan that runs on the host, or on both sides: the null model
// (fmh_logistic_null), the per-(row, phenotype) score and variance (logistic_score_one: ONE function for the kernel of logistic_kernels.hpp
// and for fmh_logistic_score_host, as hwe_exact_p is for the exact test) and the statistics from them (fmh_logistic_stats).  The definition,
// down to the operation order, is include/ferromic_hip.h's (logistic association scan); every unit that includes this is built with
// -ffp-contract=off.  Plain C++ apart from the __host__ __device__ marks: no HIP call and no library state, so that the stand-alone host
// check (host_pack_check.cpp, `make asan`) runs it under AddressSanitizer and UBSan.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "assoc_host.hpp"

#if defined(__HIPCC__)
#define FMH_LOGISTIC_HD __host__ __device__
#else
#define FMH_LOGISTIC_HD
#endif

namespace fmh_host {

constexpr size_t kLogisticMaxSamples = (size_t)1 << 21;  // S + 2 H of a w column stays within 2^53
constexpr size_t kLogisticMaxColumns = 64;               // fmh_assoc_sums' value columns
constexpr int kLogisticMaxSteps = 25;
constexpr double kLogisticTolerance = 1e-8;              // on the largest |delta_j| of a Newton step

// fmh_logistic_null's reason codes (FMH_LOGISTIC_* of the header)
enum : int32_t {
  kLogisticFitted = 0,
  kLogisticOneClass = 1,      // no case or no control
  kLogisticNotConverged = 2,  // kLogisticMaxSteps steps without max |delta| < kLogisticTolerance
  kLogisticPivot = 3,         // a Cholesky pivot that is not > 0
  kLogisticZeroWeight = 4,    // some w_i is not > 0
  kLogisticBasisLost = 5,     // a column of the whitened design dropped
};

struct LogisticNullOut {
  int32_t* values;     // n * P * (c_in + 3) entries; batches of [n][Pb * (c + 3)] written
  int32_t* exponent;   // P * (c_in + 3) entries; [P][c + 3] written
  long long* total;    // the same
  uint8_t* fitted;     // [P]
  int32_t* reason;     // [P]
  int32_t* iterations; // [P]
  uint64_t* n_cases;   // [P]
  size_t* n_basis;
  uint8_t* dropped_or_null;  // [c_in]
};

// eta, mu and w of every sample from the coefficients; false when some w is not > 0
inline bool logistic_weights(const std::vector<double>& X, size_t n, size_t d, const double* beta, double* mu, double* w) {
  for (size_t i = 0; i < n; ++i) {
    double eta = 0.0;
    for (size_t j = 0; j < d; ++j) eta += X[j * n + i] * beta[j];
    mu[i] = 1.0 / (1.0 + std::exp(-eta));
    w[i] = mu[i] * (1.0 - mu[i]);
    if (!(w[i] > 0.0)) return false;
  }
  return true;
}

// The null fit of one phenotype y (0 / 1) on the design X (column-major [d][n]); mu and w of the final coefficients.
inline int32_t logistic_fit(const std::vector<double>& X, size_t n, size_t d, const double* y, uint64_t n_cases, double* mu, double* w, int32_t* steps) {
  *steps = 0;
  if (n_cases == 0 || n_cases == n) return kLogisticOneClass;
  std::vector<double> beta(d, 0.0), grad(d), A(d * d), L(d * d), z(d), delta(d);
  beta[0] = std::log((double)n_cases / (double)(n - n_cases)) / X[0];  // the intercept-only fit: X[0] = 1 / sqrt(n)
  for (int step = 1; step <= kLogisticMaxSteps; ++step) {
    if (!logistic_weights(X, n, d, beta.data(), mu, w)) return kLogisticZeroWeight;
    for (size_t j = 0; j < d; ++j) {
      const double* xj = X.data() + j * n;
      double g = 0.0;
      for (size_t i = 0; i < n; ++i) g += xj[i] * (y[i] - mu[i]);
      grad[j] = g;
      for (size_t k = 0; k <= j; ++k) {
        const double* xk = X.data() + k * n;
        double a = 0.0;
        for (size_t i = 0; i < n; ++i) a += (xj[i] * w[i]) * xk[i];
        A[j * d + k] = a;
      }
    }
    // Cholesky A = L L^T, row by row
    for (size_t j = 0; j < d; ++j)
      for (size_t k = 0; k <= j; ++k) {
        double s = A[j * d + k];
        for (size_t m = 0; m < k; ++m) s -= L[j * d + m] * L[k * d + m];
        if (k == j) {
          if (!(s > 0.0)) return kLogisticPivot;
          L[j * d + j] = std::sqrt(s);
        } else {
          L[j * d + k] = s / L[k * d + k];
        }
      }
    for (size_t j = 0; j < d; ++j) {  // L z = grad
      double s = grad[j];
      for (size_t m = 0; m < j; ++m) s -= L[j * d + m] * z[m];
      z[j] = s / L[j * d + j];
    }
    for (size_t j = d; j-- > 0;) {  // L^T delta = z
      double s = z[j];
      for (size_t m = j + 1; m < d; ++m) s -= L[m * d + j] * delta[m];
      delta[j] = s / L[j * d + j];
    }
    double worst = 0.0;
    bool finite = true;
    for (size_t j = 0; j < d; ++j) {
      beta[j] += delta[j];
      const double a = std::fabs(delta[j]);
      if (!(a <= 1.7976931348623157e308)) finite = false;  // NaN or infinite
      if (a > worst) worst = a;
    }
    *steps = step;
    if (finite && worst < kLogisticTolerance) {
      if (!logistic_weights(X, n, d, beta.data(), mu, w)) return kLogisticZeroWeight;
      return kLogisticFitted;
    }
  }
  return kLogisticNotConverged;
}

// nullptr, or the message of the refusal (FMH_ERR_INVALID); only dropped_or_null may have been written by then.
inline const char* logistic_null(const double* phenotypes, const double* covariates_or_null, size_t n, size_t P, size_t cin, const LogisticNullOut& out) {
  if (!phenotypes || !out.values || !out.exponent || !out.total || !out.fitted || !out.reason || !out.iterations || !out.n_cases || !out.n_basis)
    return "NULL argument";
  if (cin != 0 && !covariates_or_null) return "covariates are counted but the pointer is NULL";
  if (P < 1) return "at least one phenotype is required";
  if (n == 0 || n > kLogisticMaxSamples) return "1 to 2^21 samples are taken";
  for (size_t i = 0; i < n * cin; ++i)
    if (!std::isfinite(covariates_or_null[i])) return "a covariate is not finite";
  for (size_t i = 0; i < n * P; ++i)
    if (!(phenotypes[i] == 0.0 || phenotypes[i] == 1.0)) return "a phenotype entry is neither 0 nor 1";

  std::vector<double> X(n, 1.0 / std::sqrt((double)n));  // the design, column-major: the constant, then the kept covariates
  std::vector<double> q;
  const size_t c = covariate_basis(covariates_or_null, n, cin, q, out.dropped_or_null);
  if (c + 3 > kLogisticMaxColumns) return "the kept covariates + 3 exceed 64 value columns";
  if (n < c + 3) return "fewer samples than kept covariates + 3";
  X.insert(X.end(), q.begin(), q.end());
  const size_t d = c + 1, W = c + 3, batch = kLogisticMaxColumns / W;
  *out.n_basis = c;

  std::vector<double> y(n), mu(n), w(n), z(n), col(n), u;
  for (size_t p = 0; p < P; ++p) {
    uint64_t cases = 0;
    for (size_t i = 0; i < n; ++i) {
      y[i] = phenotypes[i * P + p];
      cases += y[i] == 1.0 ? 1 : 0;
    }
    int32_t steps = 0;
    int32_t reason = logistic_fit(X, n, d, y.data(), cases, mu.data(), w.data(), &steps);
    // the whitened basis: z_j = sqrt(w) x_j, orthonormalised in column order
    u.clear();
    size_t kept = 0;
    for (size_t j = 0; j < d && reason == kLogisticFitted; ++j) {
      for (size_t i = 0; i < n; ++i) z[i] = std::sqrt(w[i]) * X[j * n + i];
      if (!orthonormal_append(z.data(), u, &kept, n)) reason = kLogisticBasisLost;
    }
    // this phenotype's W columns within its batch: [n][Pb * W] at values + n * W * (first phenotype of the batch)
    const size_t first = p / batch * batch, Pb = (P - first < batch ? P - first : batch), pitch = Pb * W;
    int32_t* v = out.values + n * W * first + (p - first) * W;
    int32_t* e = out.exponent + p * W;
    long long* t = out.total + p * W;
    if (reason == kLogisticFitted) {
      for (size_t j = 0; j < d; ++j) {
        for (size_t i = 0; i < n; ++i) col[i] = std::sqrt(w[i]) * u[j * n + i];
        quantise_column(col.data(), n, v + j, pitch, e + j, t + j);
      }
      for (size_t i = 0; i < n; ++i) col[i] = y[i] - mu[i];
      quantise_column(col.data(), n, v + d, pitch, e + d, t + d);
      quantise_column(w.data(), n, v + d + 1, pitch, e + d + 1, t + d + 1);
    } else {
      for (size_t k = 0; k < W; ++k) {
        for (size_t i = 0; i < n; ++i) v[i * pitch + k] = 0;
        e[k] = 0;
        t[k] = 0;
      }
    }
    out.fitted[p] = reason == kLogisticFitted ? 1 : 0;
    out.reason[p] = reason;
    out.iterations[p] = steps;
    out.n_cases[p] = cases;
  }
  return nullptr;
}

// ---- score and variance of one (row, phenotype): the device kernel and the host twin call this one function -------------------------------
// S, C: the row's sums [K]; h: the hom-alt sum of the phenotype's w column; T, e: [K]; o = p * (c + 3).
FMH_LOGISTIC_HD inline void logistic_score_one(const long long* S, const long long* C, long long h, uint32_t hom_ref, uint32_t het, uint32_t hom_alt,
                                               const long long* T, const int32_t* e, size_t c, size_t o, double* score, double* variance) {
  const uint64_t N = (uint64_t)hom_ref + het + hom_alt, n_alt = (uint64_t)het + 2 * (uint64_t)hom_alt;
  if (N == 0 || n_alt == 0 || n_alt == 2 * N) {
    *score = *variance = __builtin_nan("");
    return;
  }
  const double mu = (double)n_alt / (double)N;
  const size_t kr = o + c + 1, kw = o + c + 2;
  const double U = ldexp((double)S[kr] + mu * (double)(T[kr] - C[kr]), -e[kr]);
  double Vr = ldexp((double)(S[kw] + 2 * h) + (mu * mu) * (double)(T[kw] - C[kw]), -e[kw]);
  for (size_t j = 0; j <= c; ++j) {
    const size_t k = o + j;
    const double a = ldexp((double)S[k] + mu * (double)(T[k] - C[k]), -e[k]);
    Vr = Vr - a * a;
  }
  *score = U;
  *variance = Vr;
}

// chi2, z, p, beta, se of one (U, Vr); NaN where Vr is not > 0 or an input is NaN
inline void logistic_stats_one(double U, double Vr, double* chi2, double* z, double* p, double* beta, double* se) {
  const double nan = __builtin_nan("");
  if (!(Vr > 0.0) || U != U) {
    *chi2 = *z = *p = *beta = *se = nan;
    return;
  }
  *chi2 = U * U / Vr;
  *z = U / std::sqrt(Vr);
  *p = std::erfc(std::sqrt(*chi2 / 2.0));
  *beta = U / Vr;
  *se = 1.0 / std::sqrt(Vr);
}

}  // namespace fmh_host
