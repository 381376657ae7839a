// admix_host.hpp — host arithmetic of the admixture model (admix.hip, admix_host_check.cpp; definition in include/ferromic_hip.h, scheme in
// DESIGN.md section 3.27): the usable rule, the host twin of one EM step, the default start and the SQUAREM extrapolation.  No device, no
// library call: plain f64, every sum over ascending index; the units that include this are built with -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fmh_host {

constexpr size_t kAdmixMaxK = 16;
constexpr double kAdmixEps = 1e-5;  // ADMIXTURE's bound on Q and F
constexpr uint32_t kAdmixUpdateQ = 1u, kAdmixUpdateF = 2u;

inline bool admix_usable(uint32_t c, uint32_t a) { return c > 0 && a > 0 && (uint64_t)a < 2ull * c; }

inline double admix_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// q° -> q': clamp every component, then divide by the sum over ascending k
inline void admix_renormalise(double* q, size_t K) {
  double sum = 0.0;
  for (size_t k = 0; k < K; ++k) {
    q[k] = admix_clamp(q[k], kAdmixEps, 1.0 - kAdmixEps);
    sum += q[k];
  }
  for (size_t k = 0; k < K; ++k) q[k] = q[k] / sum;
}

// The tracks of a dosage table [rows][n] (0, 1, 2; above 2 = not called): usable, c, a per row, m_i per sample; returns m.
inline size_t admix_tracks(const uint8_t* dosage, size_t rows, size_t n, uint8_t* usable, uint32_t* called, uint32_t* allele_count, uint64_t* sample_sites) {
  size_t m = 0;
  if (sample_sites)
    for (size_t i = 0; i < n; ++i) sample_sites[i] = 0;
  for (size_t r = 0; r < rows; ++r) {
    uint32_t c = 0, a = 0;
    for (size_t i = 0; i < n; ++i) {
      const uint8_t g = dosage[r * n + i];
      if (g <= 2) { ++c; a += g; }
    }
    const bool ok = admix_usable(c, a);
    if (usable) usable[r] = ok ? 1 : 0;
    if (called) called[r] = c;
    if (allele_count) allele_count[r] = a;
    if (!ok) continue;
    ++m;
    if (sample_sites)
      for (size_t i = 0; i < n; ++i)
        if (dosage[r * n + i] <= 2) ++sample_sites[i];
  }
  return m;
}

// One EM step over the usable rows of a dosage table.  q [n][K]; f, f_out [m][K] over the usable rows in row order; q_out [n][K].
// flags: kAdmixUpdateQ | kAdmixUpdateF; a half that is not updated is copied.  loglik (may be null) is l of the INPUT.
inline void admix_step_host(const uint8_t* dosage, size_t rows, size_t n, size_t K, const double* q, const double* f, double* q_out, double* f_out,
                            double* loglik, uint32_t flags) {
  std::vector<double> E(n * K, 0.0), A(K), B(K), g1(K);
  std::vector<uint64_t> sites(n, 0);
  double ll = 0.0;
  size_t j = 0;
  for (size_t r = 0; r < rows; ++r) {
    uint32_t c = 0, a = 0;
    for (size_t i = 0; i < n; ++i) {
      const uint8_t g = dosage[r * n + i];
      if (g <= 2) { ++c; a += g; }
    }
    if (!admix_usable(c, a)) continue;
    const double* fj = f + j * K;
    for (size_t k = 0; k < K; ++k) { g1[k] = 1.0 - fj[k]; A[k] = 0.0; B[k] = 0.0; }
    for (size_t i = 0; i < n; ++i) {
      const uint8_t g = dosage[r * n + i];
      if (g > 2) continue;
      ++sites[i];
      const double* qi = q + i * K;
      double h0 = 0.0, h1 = 0.0;
      for (size_t k = 0; k < K; ++k) { h0 += qi[k] * fj[k]; h1 += qi[k] * g1[k]; }
      const double u = (double)g / h0, v = (double)(2 - g) / h1;
      for (size_t k = 0; k < K; ++k) {
        A[k] += u * qi[k];
        B[k] += v * qi[k];
        E[i * K + k] += u * fj[k] + v * g1[k];
      }
      if (loglik) ll += (double)g * std::log(h0) + (double)(2 - g) * std::log(h1);
    }
    for (size_t k = 0; k < K; ++k) {
      if (flags & kAdmixUpdateF) {
        const double fa = fj[k] * A[k], gb = g1[k] * B[k];
        f_out[j * K + k] = admix_clamp(fa / (fa + gb), kAdmixEps, 1.0 - kAdmixEps);
      } else {
        f_out[j * K + k] = fj[k];
      }
    }
    ++j;
  }
  for (size_t i = 0; i < n; ++i) {
    for (size_t k = 0; k < K; ++k) q_out[i * K + k] = q[i * K + k];
    if (!(flags & kAdmixUpdateQ) || sites[i] == 0) continue;
    for (size_t k = 0; k < K; ++k) q_out[i * K + k] = q[i * K + k] * E[i * K + k] / (2.0 * (double)sites[i]);
    admix_renormalise(q_out + i * K, K);
  }
  if (loglik) *loglik = ll;
}

// splitmix64's finaliser after adding the golden-ratio increment
inline uint64_t admix_mix(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline double admix_unit(uint64_t seed_mixed, uint64_t t) { return (double)(admix_mix(seed_mixed + t) >> 11) * 0x1p-53; }

// The default start: q [n][K], f [m][K] from c, a of the m usable rows.
inline void admix_start(const uint32_t* called, const uint32_t* allele_count, size_t m, size_t n, size_t K, uint64_t seed, double* q, double* f) {
  const uint64_t s = admix_mix(seed);
  for (size_t i = 0; i < n; ++i) {
    double sum = 0.0;
    for (size_t k = 0; k < K; ++k) {
      q[i * K + k] = 1.0 + admix_unit(s, (uint64_t)(i * K + k));
      sum += q[i * K + k];
    }
    for (size_t k = 0; k < K; ++k) q[i * K + k] = q[i * K + k] / sum;
  }
  for (size_t j = 0; j < m; ++j) {
    const double p = (double)allele_count[j] / (2.0 * (double)called[j]);
    for (size_t k = 0; k < K; ++k)
      f[j * K + k] = admix_clamp(p + 0.2 * (admix_unit(s, ((uint64_t)1 << 40) + (uint64_t)(j * K + k)) - 0.5), 0.01, 0.99);
  }
}

// SQUAREM-S3: r = t1 - t0, v = (t2 - t1) - r, alpha = max(1, sqrt(sum r^2 / sum v^2)) with the sums over Q then F in ascending index;
// ta = t0 + 2 alpha r + alpha^2 v, F clamped, Q clamped and renormalised.  sum v^2 == 0: ta = t2 and alpha = 0 (no extrapolation).
inline double admix_accelerate(const double* q0, const double* f0, const double* q1, const double* f1, const double* q2, const double* f2, size_t n, size_t m,
                               size_t K, double* qa, double* fa) {
  double sr = 0.0, sv = 0.0;
  for (size_t e = 0; e < n * K; ++e) {
    const double r = q1[e] - q0[e], v = (q2[e] - q1[e]) - r;
    sr += r * r;
    sv += v * v;
  }
  for (size_t e = 0; e < m * K; ++e) {
    const double r = f1[e] - f0[e], v = (f2[e] - f1[e]) - r;
    sr += r * r;
    sv += v * v;
  }
  if (sv == 0.0) {
    for (size_t e = 0; e < n * K; ++e) qa[e] = q2[e];
    for (size_t e = 0; e < m * K; ++e) fa[e] = f2[e];
    return 0.0;
  }
  double alpha = std::sqrt(sr / sv);
  if (!(alpha > 1.0)) alpha = 1.0;
  const double a2 = 2.0 * alpha, aa = alpha * alpha;
  for (size_t e = 0; e < n * K; ++e) {
    const double r = q1[e] - q0[e], v = (q2[e] - q1[e]) - r;
    qa[e] = (q0[e] + a2 * r) + aa * v;
  }
  for (size_t i = 0; i < n; ++i) admix_renormalise(qa + i * K, K);
  for (size_t e = 0; e < m * K; ++e) {
    const double r = f1[e] - f0[e], v = (f2[e] - f1[e]) - r;
    fa[e] = admix_clamp((f0[e] + a2 * r) + aa * v, kAdmixEps, 1.0 - kAdmixEps);
  }
  return alpha;
}

}  // namespace fmh_host
