// lmm_host.hpp — host arithmetic of the mixed-model association scan (lmm.hip; definition in include/ferromic_hip.h, scheme in DESIGN.md
// section 3.25): the twin of the device projections over a dosage table, the null fit of the variance ratio delta per phenotype in the
// eigenbasis of the relationship matrix, and the per-site statistics from the projections.  The covariate basis, the sequential sums and the
// Student-t tail are assoc_host.hpp's.  The operation order is the header's; every unit that includes this is built with -ffp-contract=off.
// Plain C++: no HIP, no library state, so that a stand-alone program (lmm_host_check.cpp) can run it under a sanitizer.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <limits>
#include <vector>

#include "assoc_host.hpp"

namespace fmh_host {

constexpr size_t kLmmMaxComponents = 32768, kLmmMaxQuad = 16, kLmmMaxLinear = 64;
constexpr int kLmmGridPoints = 101, kLmmGoldenSteps = 40;  // log10 delta = -5, -4.9, .. 5, then the golden section around the best

// mu of a row from its exact counts: the device and the oracle use these bits
inline double lmm_mu(uint32_t called, uint32_t allele_count) { return called == 0 ? 0.0 : (double)allele_count / (double)called; }

// ---- the twin: dosage [rows][n] (0, 1, 2; above 2 = not called), every sum over ascending index in plain f64 -----------------------------
inline void lmm_projections_host(const uint8_t* dosage, size_t rows, size_t n, const double* basis, size_t K, const double* weights, size_t P,
                                 const double* linear, size_t L, double* quad, double* lin, uint32_t* called_or_null, uint32_t* allele_count_or_null) {
  std::vector<double> T(K), x(n);
  for (size_t r = 0; r < rows; ++r) {
    const uint8_t* d = dosage + r * n;
    uint32_t c = 0, a = 0;
    for (size_t i = 0; i < n; ++i)
      if (d[i] <= 2) { ++c; a += d[i]; }
    const double mu = lmm_mu(c, a);
    for (size_t i = 0; i < n; ++i) x[i] = d[i] <= 2 ? (double)d[i] : mu;
    for (size_t k = 0; k < K; ++k) T[k] = 0.0;
    for (size_t i = 0; i < n; ++i)  // per k the sum still runs over ascending i
      for (size_t k = 0; k < K; ++k) T[k] += basis[i * K + k] * x[i];
    for (size_t p = 0; p < P; ++p) {
      double s = 0.0;
      for (size_t k = 0; k < K; ++k) s += weights[p * K + k] * (T[k] * T[k]);
      quad[r * P + p] = s;
    }
    for (size_t j = 0; j < L; ++j) {
      double s = 0.0;
      for (size_t k = 0; k < K; ++k) s += linear[j * K + k] * T[k];
      lin[r * L + j] = s;
    }
    if (called_or_null) called_or_null[r] = c;
    if (allele_count_or_null) allele_count_or_null[r] = a;
  }
}

// ---- the null fit ------------------------------------------------------------------------------------------------------------------------------
// Cholesky of the symmetric q x q matrix a (row-major), lower factor in place; false where a pivot is not positive
inline bool lmm_cholesky(double* a, size_t q) {
  for (size_t j = 0; j < q; ++j) {
    double d = a[j * q + j];
    for (size_t k = 0; k < j; ++k) d -= a[j * q + k] * a[j * q + k];
    if (!(d > 0.0)) return false;
    const double l = std::sqrt(d);
    a[j * q + j] = l;
    for (size_t i = j + 1; i < q; ++i) {
      double s = a[i * q + j];
      for (size_t k = 0; k < j; ++k) s -= a[i * q + k] * a[j * q + k];
      a[i * q + j] = s / l;
    }
  }
  return true;
}
// b <- (L L^T)^-1 b
inline void lmm_cholesky_solve(const double* l, size_t q, double* b) {
  for (size_t i = 0; i < q; ++i) {
    double s = b[i];
    for (size_t k = 0; k < i; ++k) s -= l[i * q + k] * b[k];
    b[i] = s / l[i * q + i];
  }
  for (size_t i = q; i-- > 0;) {
    double s = b[i];
    for (size_t k = i + 1; k < q; ++k) s -= l[k * q + i] * b[k];
    b[i] = s / l[i * q + i];
  }
}

// one phenotype in the eigenbasis: lam [n] (clipped at 0), xr [n][q] and yr [n] rotated
struct LmmRotated {
  size_t n = 0, q = 0;
  const double *lam = nullptr, *xr = nullptr, *yr = nullptr;
};
// what one evaluation at delta leaves behind
struct LmmEval {
  std::vector<double> w, chol, xwy, b;  // [n], [q][q] lower factor of XWX, [q] X~^T W y~, [q] the solution
  double R = 0.0, ll = 0.0;
};
// l(delta); -inf where XWX is not positive definite or R is not positive
inline double lmm_log_likelihood(const LmmRotated& z, double delta, LmmEval& e) {
  const size_t n = z.n, q = z.q;
  const double neg_inf = -std::numeric_limits<double>::infinity();
  e.w.resize(n); e.chol.assign(q * q, 0.0); e.xwy.assign(q, 0.0); e.b.resize(q);
  double log_v = 0.0;
  for (size_t k = 0; k < n; ++k) {
    const double s = z.lam[k] + delta;
    e.w[k] = 1.0 / s;
    log_v += std::log(s);
  }
  for (size_t a = 0; a < q; ++a) {
    for (size_t b = 0; b <= a; ++b) {
      double s = 0.0;
      for (size_t k = 0; k < n; ++k) s += e.w[k] * z.xr[k * q + a] * z.xr[k * q + b];
      e.chol[a * q + b] = e.chol[b * q + a] = s;
    }
    double s = 0.0;
    for (size_t k = 0; k < n; ++k) s += e.w[k] * z.xr[k * q + a] * z.yr[k];
    e.xwy[a] = s;
  }
  e.R = std::numeric_limits<double>::quiet_NaN();
  e.ll = neg_inf;
  if (!lmm_cholesky(e.chol.data(), q)) return neg_inf;
  double log_det = 0.0;
  for (size_t a = 0; a < q; ++a) log_det += std::log(e.chol[a * q + a]);
  log_det = 2.0 * log_det;
  e.b = e.xwy;
  lmm_cholesky_solve(e.chol.data(), q, e.b.data());
  double R = 0.0;
  for (size_t k = 0; k < n; ++k) {
    double fit = 0.0;
    for (size_t a = 0; a < q; ++a) fit += z.xr[k * q + a] * e.b[a];
    const double res = z.yr[k] - fit;
    R += e.w[k] * (res * res);
  }
  e.R = R;
  if (!(R > 0.0)) return neg_inf;
  const double dof = (double)(n - q);
  e.ll = -0.5 * (dof * std::log(2.0 * 3.14159265358979323846 * R / dof) + log_v + log_det + dof);
  return e.ll;
}

// log10 delta of grid point i
inline double lmm_grid_point(int i) { return -5.0 + 0.1 * (double)i; }

// the search: 101 grid points, the argmax (the lowest index on a tie), 40 golden-section steps on [best - 0.1, best + 0.1] clipped to
// [-5, 5]; returns log10 delta of the best point evaluated (an earlier point wins a tie)
inline double lmm_search(const LmmRotated& z, LmmEval& e, double* grid_ll_or_null) {
  double best_x = lmm_grid_point(0), best_ll = -std::numeric_limits<double>::infinity();
  bool any = false;
  for (int i = 0; i < kLmmGridPoints; ++i) {
    const double x = lmm_grid_point(i), ll = lmm_log_likelihood(z, std::pow(10.0, x), e);
    if (grid_ll_or_null) grid_ll_or_null[i] = ll;
    if (!any || ll > best_ll) { best_x = x; best_ll = ll; any = true; }
  }
  const double gr = (std::sqrt(5.0) - 1.0) / 2.0;
  double lo = std::max(best_x - 0.1, -5.0), hi = std::min(best_x + 0.1, 5.0);
  double c = hi - gr * (hi - lo), d = lo + gr * (hi - lo);
  double fc = lmm_log_likelihood(z, std::pow(10.0, c), e), fd = lmm_log_likelihood(z, std::pow(10.0, d), e);
  if (fc > best_ll) { best_x = c; best_ll = fc; }
  if (fd > best_ll) { best_x = d; best_ll = fd; }
  for (int step = 0; step < kLmmGoldenSteps; ++step) {
    if (fc > fd) {
      hi = d; d = c; fd = fc;
      c = hi - gr * (hi - lo);
      fc = lmm_log_likelihood(z, std::pow(10.0, c), e);
      if (fc > best_ll) { best_x = c; best_ll = fc; }
    } else {
      lo = c; c = d; fc = fd;
      d = lo + gr * (hi - lo);
      fd = lmm_log_likelihood(z, std::pow(10.0, d), e);
      if (fd > best_ll) { best_x = d; best_ll = fd; }
    }
  }
  return best_x;
}

// the outputs of the null fit; every pointer set.  q = the columns of the design matrix, known after the covariate basis: the arrays are sized
// by the caller for q = c_in + 1 and filled densely for the q that results
struct LmmNullOut {
  double *delta, *sigma_g2, *sigma_e2, *h2, *log_likelihood;  // [P]
  uint8_t *at_boundary, *reason;                              // [P]; reason: 0 fitted, 1 no variance left after the design matrix
  double *weights, *linear;                                   // [P][n], [P][q + 1][n]
  double *M, *v, *R;                                          // [P][q][q], [P][q], [P]
  double* grid_ll_or_null;                                    // [P][101] l at the grid points (tests), or null
};

// lam [n], U [n][n] (column k the eigenvector of lam[k]), Y [n][P], cov [n][cin] or null.  Returns a refusal's words or null.
// *q_out and dropped (may be null) are set before the P (q + 1) <= 64 refusal can fire.  fixed_delta [P] (or null): the search is skipped.
inline const char* lmm_null(const double* lam_in, const double* U, const double* Y, const double* cov, size_t n, size_t P, size_t cin, size_t* q_out,
                            uint8_t* dropped_or_null, const double* fixed_delta_or_null, const LmmNullOut& o) {
  std::vector<double> basis;  // Q, column-major
  const size_t c = covariate_basis(cov, n, cin, basis, dropped_or_null), q = c + 1;
  *q_out = q;
  if (n < q + 2) return "n - q - 1 residual degrees of freedom: at least 1 is required";
  if (P > kLmmMaxQuad || P * (q + 1) > kLmmMaxLinear) return "P phenotypes with q design columns: P <= 16 and P (q + 1) <= 64 are required (batch the phenotypes)";
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> lam(n), X(n * q), xr(n * q), y(n), yr(n), res(n);
  for (size_t k = 0; k < n; ++k) lam[k] = lam_in[k] > 0.0 ? lam_in[k] : 0.0;
  const double ones = 1.0 / std::sqrt((double)n);
  for (size_t i = 0; i < n; ++i) {
    X[i * q] = ones;
    for (size_t j = 0; j < c; ++j) X[i * q + 1 + j] = basis[j * n + i];
  }
  for (size_t k = 0; k < n; ++k)
    for (size_t j = 0; j < q; ++j) xr[k * q + j] = seq_dot(U + k, X.data() + j, n, n, q);
  LmmEval e;
  for (size_t p = 0; p < P; ++p) {
    for (size_t i = 0; i < n; ++i) y[i] = res[i] = Y[i * P + p];
    // what the design matrix leaves of the phenotype, by the covariates' own drop rule
    const double r0 = std::sqrt(seq_dot(y.data(), y.data(), n, 1, 1));
    centre(res.data(), n);
    project_off(res.data(), basis, c, n);
    const double r1 = std::sqrt(seq_dot(res.data(), res.data(), n, 1, 1));
    double* weights = o.weights + p * n;
    double* linear = o.linear + p * (q + 1) * n;
    if (r0 == 0.0 || r1 <= r0 * 0x1p-26) {
      o.delta[p] = o.sigma_g2[p] = o.sigma_e2[p] = o.h2[p] = o.log_likelihood[p] = o.R[p] = nan;
      o.at_boundary[p] = 0;
      o.reason[p] = 1;
      for (size_t k = 0; k < n; ++k) weights[k] = 0.0;
      for (size_t k = 0; k < (q + 1) * n; ++k) linear[k] = 0.0;
      for (size_t k = 0; k < q * q; ++k) o.M[p * q * q + k] = nan;
      for (size_t k = 0; k < q; ++k) o.v[p * q + k] = nan;
      if (o.grid_ll_or_null)
        for (int i = 0; i < kLmmGridPoints; ++i) o.grid_ll_or_null[p * kLmmGridPoints + i] = nan;
      continue;
    }
    for (size_t k = 0; k < n; ++k) yr[k] = seq_dot(U + k, y.data(), n, n, 1);
    const LmmRotated z{n, q, lam.data(), xr.data(), yr.data()};
    double x = 0.0, delta;
    if (fixed_delta_or_null) {
      delta = fixed_delta_or_null[p];
      if (o.grid_ll_or_null)
        for (int i = 0; i < kLmmGridPoints; ++i) o.grid_ll_or_null[p * kLmmGridPoints + i] = nan;
    } else {
      x = lmm_search(z, e, o.grid_ll_or_null ? o.grid_ll_or_null + p * kLmmGridPoints : nullptr);
      delta = std::pow(10.0, x);
    }
    const double ll = lmm_log_likelihood(z, delta, e);
    o.delta[p] = delta;
    o.sigma_g2[p] = e.R / (double)(n - q);
    o.sigma_e2[p] = delta * o.sigma_g2[p];
    o.h2[p] = 1.0 / (1.0 + delta);
    o.log_likelihood[p] = ll;
    o.at_boundary[p] = (!fixed_delta_or_null && (x == -5.0 || x == 5.0)) ? 1 : 0;
    o.reason[p] = 0;
    o.R[p] = e.R;
    for (size_t k = 0; k < n; ++k) weights[k] = e.w[k];
    for (size_t j = 0; j < q; ++j)
      for (size_t k = 0; k < n; ++k) linear[j * n + k] = e.w[k] * xr[k * q + j];
    for (size_t k = 0; k < n; ++k) linear[q * n + k] = e.w[k] * yr[k];
    // M = XWX^-1 column by column through the factor; v = M (X~^T W y~)
    double* M = o.M + p * q * q;
    std::vector<double> col(q);
    for (size_t j = 0; j < q; ++j) {
      for (size_t i = 0; i < q; ++i) col[i] = i == j ? 1.0 : 0.0;
      lmm_cholesky_solve(e.chol.data(), q, col.data());
      for (size_t i = 0; i < q; ++i) M[i * q + j] = col[i];
    }
    for (size_t i = 0; i < q; ++i) o.v[p * q + i] = seq_dot(M + i * q, e.xwy.data(), q, 1, 1);
  }
  return nullptr;
}

// ---- the statistics of `rows` rows: quad [rows][P], lin [rows][P (q + 1)], the exact counts c and a ------------------------------------------
inline void lmm_stats(const double* quad, const double* lin, const uint32_t* called, const uint32_t* allele_count, size_t rows, const double* M,
                      const double* v, const double* R, uint64_t n, size_t q, size_t P, double* beta, double* se, double* t, double* p_out) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const uint64_t df = n - q - 1;
  const size_t L = P * (q + 1);
  auto put = [&](double* out, size_t i, double x) { if (out) out[i] = x; };
  for (size_t r = 0; r < rows; ++r) {
    const uint64_t c = called[r], a = allele_count[r];
    const bool polymorphic = c != 0 && a != 0 && a != 2 * c;
    for (size_t p = 0; p < P; ++p) {
      const size_t o = r * P + p;
      const double* av = lin + r * L + p * (q + 1);
      const double *Mp = M + p * q * q, *vp = v + p * q;
      double D = nan, num = nan;
      if (polymorphic) {
        double aMa = 0.0, av_v = 0.0;
        for (size_t i = 0; i < q; ++i) aMa += seq_dot(Mp + i * q, av, q, 1, 1) * av[i];
        for (size_t i = 0; i < q; ++i) av_v += av[i] * vp[i];
        D = quad[o] - aMa;
        num = av[q] - av_v;
      }
      if (!(D > 0.0)) {
        put(beta, o, nan); put(se, o, nan); put(t, o, nan); put(p_out, o, nan);
        continue;
      }
      const double b = num / D;
      double rss = R[p] - num * num / D;
      if (rss < 0.0) rss = 0.0;
      const double s = std::sqrt(rss / (double)df / D);
      put(beta, o, b);
      put(se, o, s);
      if (s == 0.0) {
        put(t, o, nan); put(p_out, o, nan);
        continue;
      }
      const double tv = b / s;
      put(t, o, tv);
      put(p_out, o, student_t_two_sided(tv, (double)df));
    }
  }
}

}  // namespace fmh_host
