// grm_host_check.cpp — sanitizer check of the host arithmetic of the relationship matrix (grm_host.hpp: grm_values, grm_host, grm_finish,
// grm_fix_sign) on a seeded cohort held in exact-size heap blocks, so that a read or write one element past the dosage table, the counts or
// an output is an ASan report.  The cohort comes from a splitmix64 stream that tests/grm_ref.py restates; the program prints an order-free
// checksum of the usable flags, the value bits, the product bits, the pair counts and the matrix bits, which tests/test_grm_cpu.py compares
// with the oracle's (tests/grm_ref.py: checksum).
// Built by `make asan` with -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off.
//   grm_host_check.asan seed K n method denominator
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "grm_host.hpp"

static uint64_t g_state = 0;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static uint64_t bits_of(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof b);
  return v != v ? 0x7FF8000000000000ull : b;  // every NaN alike
}

int main(int argc, char** argv) {
  if (argc != 6) { fprintf(stderr, "usage: %s seed K n method denominator\n", argv[0]); return 2; }
  g_state = strtoull(argv[1], nullptr, 10);
  const size_t K = strtoull(argv[2], nullptr, 10), n = strtoull(argv[3], nullptr, 10);
  fmh_grm_params P{};
  P.method = (uint32_t)strtoul(argv[4], nullptr, 10);
  P.denominator = (uint32_t)strtoul(argv[5], nullptr, 10);
  if (const char* refused = fmh_host::grm_check_params(P)) { fprintf(stderr, "refused: %s\n", refused); return 2; }
  if (n == 0) { fprintf(stderr, "refused: n is 0\n"); return 2; }

  // the cohort: per row an allele frequency of t / 16 (t = 0 .. 16: monomorphic rows at both ends), two draws per genotype; a tenth of the rows
  // lose a quarter of their calls, one row in 32 all of them
  std::vector<uint8_t> dosage(K * n);
  for (size_t k = 0; k < K; ++k) {
    const uint64_t t = rnd() % 17, gaps = rnd() % 32;
    for (size_t s = 0; s < n; ++s) {
      uint8_t g = (uint8_t)((rnd() % 16 < t) + (rnd() % 16 < t));
      if (gaps == 0 || (gaps < 4 && rnd() % 4 == 0)) g = 3;
      dosage[k * n + s] = g;
    }
  }

  std::vector<double> S(n * n), A(n * n);
  std::vector<uint64_t> N(n * n);
  uint64_t n_usable = 0;
  double scale = 0.0;
  fmh_host::grm_host(dosage.data(), K, n, P.method, S.data(), N.data(), &n_usable, &scale);
  fmh_host::grm_finish(S.data(), N.data(), n, P, n_usable, scale, A.data());
  std::vector<uint32_t> c(K, 0), a(K, 0);
  for (size_t k = 0; k < K; ++k)
    for (size_t s = 0; s < n; ++s)
      if (dosage[k * n + s] <= 2) { ++c[k]; a[k] += dosage[k * n + s]; }
  std::vector<uint8_t> usable(K);
  std::vector<double> p(K), z(3 * K);
  fmh_host::grm_values(c.data(), a.data(), K, P.method, usable.data(), p.data(), z.data(), nullptr, nullptr);
  std::vector<double> diag(n);
  for (size_t i = 0; i < n; ++i) diag[i] = -A[i * n + i];
  fmh_host::grm_fix_sign(diag.data(), n, 1);

  uint64_t h = n_usable * 1000003 + bits_of(scale);
  for (size_t k = 0; k < K; ++k)
    h += (uint64_t)(usable[k] + 1) * (0x9E3779B97F4A7C15ull * (k + 1)) + bits_of(p[k]) * (2 * k + 1) + bits_of(z[3 * k]) * 3 + bits_of(z[3 * k + 1]) * 5 +
         bits_of(z[3 * k + 2]) * 7;
  for (size_t e = 0; e < n * n; ++e) h += bits_of(S[e]) * (2 * e + 1) + N[e] * (0xBF58476D1CE4E5B9ull + e) + bits_of(A[e]) * (2 * e + 3);
  for (size_t i = 0; i < n; ++i) h += bits_of(diag[i]) * (4 * i + 1);
  printf("grm_host_check: %zu rows x %zu samples, %llu usable, checksum %016llx\n", K, n, (unsigned long long)n_usable, (unsigned long long)h);
  return 0;
}
