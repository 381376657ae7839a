// lmm_host_check.cpp — sanitizer check of the host arithmetic of the mixed-model scan (lmm_host.hpp: lmm_projections_host, lmm_null,
// lmm_stats; assoc_host.hpp's covariate basis underneath) on a seeded case held in exact-size heap blocks, so that a read or write one
// element past a table, a coefficient row or an output is an ASan report.  The case comes from a splitmix64 stream that tests/lmm_ref.py
// restates: a dosage table with missing calls and monomorphic rows, an orthonormal basis (a Householder reflection), eigenvalues with zeros
// among them, two phenotypes (the second is constant when `flat` is 1) and three covariates of which the third repeats the first.  The null
// fit runs twice: with the search, whose log10 delta is printed, and at delta = 0.5 and 2 for the checksum - the bits of the weights, the
// linear rows, M, v, R, the projections of the twin and beta, se and t, none of which goes through log or pow.  tests/test_lmm_cpu.py compares
// the lines of a plain build, of this build and of the oracle.
// Built by `make asan` with -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off.
//   lmm_host_check.asan seed rows n flat
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lmm_host.hpp"

static uint64_t g_state = 0;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double unit() { return (double)(rnd() >> 11) * 0x1p-53 - 0.5; }  // [-0.5, 0.5)

static uint64_t bits_of(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof b);
  return v != v ? 0x7FF8000000000000ull : b;  // every NaN alike
}

int main(int argc, char** argv) {
  if (argc != 5) { fprintf(stderr, "usage: %s seed rows n flat\n", argv[0]); return 2; }
  g_state = strtoull(argv[1], nullptr, 10);
  const size_t rows = strtoull(argv[2], nullptr, 10), n = strtoull(argv[3], nullptr, 10);
  const bool flat = strtoul(argv[4], nullptr, 10) != 0;
  const size_t P = 2, cin = 3;
  if (n < 8) { fprintf(stderr, "refused: n below 8\n"); return 2; }

  std::vector<uint8_t> dosage(rows * n);
  for (size_t k = 0; k < rows; ++k) {
    const uint64_t t = rnd() % 17, gaps = rnd() % 32;
    for (size_t s = 0; s < n; ++s) {
      uint8_t g = (uint8_t)((rnd() % 16 < t) + (rnd() % 16 < t));
      if (gaps == 0 || (gaps < 4 && rnd() % 4 == 0)) g = 3;
      dosage[k * n + s] = g;
    }
  }
  // U = I - 2 h h^T / (h^T h); lambda: a quarter zero
  std::vector<double> h(n), U(n * n), lambda(n), Y(n * P), cov(n * cin);
  double hh = 0.0;
  for (size_t i = 0; i < n; ++i) { h[i] = unit(); hh += h[i] * h[i]; }
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 0; k < n; ++k) U[i * n + k] = (i == k ? 1.0 : 0.0) - 2.0 * h[i] * h[k] / hh;
  for (size_t k = 0; k < n; ++k) lambda[k] = rnd() % 4 == 0 ? 0.0 : 4.0 * (unit() + 0.5);
  for (size_t i = 0; i < n; ++i) {
    Y[i * P] = 3.0 + unit();
    Y[i * P + 1] = flat ? 1.5 : unit();
    cov[i * cin] = unit();
    cov[i * cin + 1] = 10.0 * unit();
    cov[i * cin + 2] = cov[i * cin];
  }

  const size_t qmax = cin + 1;
  std::vector<double> delta(P), sg(P), se2(P), h2(P), ll(P), weights(P * n), linear(P * (qmax + 1) * n), M(P * qmax * qmax), v(P * qmax), R(P);
  std::vector<uint8_t> boundary(P), reason(P), dropped(cin);
  const fmh_host::LmmNullOut out{delta.data(), sg.data(), se2.data(), h2.data(), ll.data(), boundary.data(), reason.data(), weights.data(),
                                 linear.data(), M.data(), v.data(), R.data(), nullptr};
  size_t q = 0;
  if (const char* refused = fmh_host::lmm_null(lambda.data(), U.data(), Y.data(), cov.data(), n, P, cin, &q, dropped.data(), nullptr, out)) {
    fprintf(stderr, "refused: %s\n", refused);
    return 2;
  }
  const double searched[2] = {delta[0], delta[1]};
  const unsigned flags = boundary[0] + 2u * boundary[1] + 4u * reason[0] + 8u * reason[1];

  const double fixed[2] = {0.5, 2.0};
  if (const char* refused = fmh_host::lmm_null(lambda.data(), U.data(), Y.data(), cov.data(), n, P, cin, &q, dropped.data(), fixed, out)) {
    fprintf(stderr, "refused: %s\n", refused);
    return 2;
  }
  const size_t L = P * (q + 1);
  // exact-size copies: the library's own layout for the q that resulted
  std::vector<double> lin_rows(linear.begin(), linear.begin() + (std::ptrdiff_t)(L * n)), Mq(M.begin(), M.begin() + (std::ptrdiff_t)(P * q * q)),
      vq(v.begin(), v.begin() + (std::ptrdiff_t)(P * q));
  std::vector<double> quad(rows * P), lin(rows * L), beta(rows * P), se(rows * P), t(rows * P), p(rows * P);
  std::vector<uint32_t> called(rows), allele_count(rows);
  fmh_host::lmm_projections_host(dosage.data(), rows, n, U.data(), n, weights.data(), P, lin_rows.data(), L, quad.data(), lin.data(), called.data(),
                                 allele_count.data());
  fmh_host::lmm_stats(quad.data(), lin.data(), called.data(), allele_count.data(), rows, Mq.data(), vq.data(), R.data(), n, q, P, beta.data(), se.data(),
                      t.data(), p.data());

  uint64_t sum = q * 1000003ull + dropped[0] + 2u * dropped[1] + 4u * dropped[2];
  size_t finite = 0;
  for (size_t e = 0; e < P * n; ++e) sum += bits_of(weights[e]) * (2 * e + 1);
  for (size_t e = 0; e < L * n; ++e) sum += bits_of(lin_rows[e]) * (2 * e + 3);
  for (size_t e = 0; e < P * q * q; ++e) sum += bits_of(Mq[e]) * (2 * e + 5);
  for (size_t e = 0; e < P * q; ++e) sum += bits_of(vq[e]) * (2 * e + 7);
  for (size_t e = 0; e < P; ++e) sum += bits_of(R[e]) * (2 * e + 9);
  for (size_t e = 0; e < rows; ++e) sum += (uint64_t)called[e] * (0x9E3779B97F4A7C15ull + e) + (uint64_t)allele_count[e] * (0xBF58476D1CE4E5B9ull + e);
  for (size_t e = 0; e < rows * P; ++e) {
    sum += bits_of(quad[e]) * (2 * e + 11) + bits_of(beta[e]) * (2 * e + 13) + bits_of(se[e]) * (2 * e + 15) + bits_of(t[e]) * (2 * e + 17);
    if (p[e] == p[e]) ++finite;
  }
  for (size_t e = 0; e < rows * L; ++e) sum += bits_of(lin[e]) * (2 * e + 19);
  printf("lmm_host_check: %zu rows x %zu samples, q %zu, %zu finite, flags %u, checksum %016llx\n", rows, n, q, finite, flags, (unsigned long long)sum);
  printf("delta %.17g %.17g\n", searched[0], searched[1]);
  return 0;
}
