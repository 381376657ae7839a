// ldscore_host_check.cpp — sanitizer check of the host side of the LD scores (ldscore_host.hpp: ld_scores_host, ld_score_values,
// ldsc_regress) on the seeded founder-mosaic cohort of clump_host_check.cpp, held in exact-size heap blocks, so that a read or write one
// element past the dosage table, the positions or an output is an ASan report.  The cohort comes from a splitmix64 stream that
// tests/clump_ref.py restates (splitmix_cohort; its p values, drawn last, are not needed here); the chi^2 column of the regression comes
// from a second stream seeded with seed + 1.  The program prints an order-free checksum of Q, partners, counted and the score bits and the bits of the regression's four
// estimates, which tests/test_ldscore_cpu.py compares with the oracle's (tests/ldscore_ref.py).
// Built by `make asan` with -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off.
//   ldscore_host_check.asan seed K n window flags
//   ldscore_host_check.asan ranges K window every     the partner ranges of K rows at positions k / every, and the row the 2^22 rule refuses
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ldscore_host.hpp"

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
  if (argc == 5 && strcmp(argv[1], "ranges") == 0) {
    const size_t K = strtoull(argv[2], nullptr, 10), every = strtoull(argv[4], nullptr, 10);
    const uint32_t window = (uint32_t)strtoul(argv[3], nullptr, 10);
    if (every == 0) { fprintf(stderr, "refused: every is 0\n"); return 2; }
    std::vector<uint32_t> x(K), lo, hi;
    for (size_t k = 0; k < K; ++k) x[k] = (uint32_t)(k / every);
    fmh_host::ld_score_ranges(x, window, lo, hi);
    uint64_t most = 0, total = 0;
    for (size_t k = 0; k < K; ++k) { most = std::max<uint64_t>(most, hi[k] - lo[k]); total += hi[k] - lo[k]; }
    const size_t crowded = fmh_host::ld_score_crowded_row(lo, hi);
    printf("ldscore_host_check: ranges of %zu rows, window %u: %llu partners in all, at most %llu, first refused row %lld\n", K, window, (unsigned long long)total,
           (unsigned long long)most, crowded == K ? -1ll : (long long)crowded);
    return 0;
  }
  if (argc != 6) { fprintf(stderr, "usage: %s seed K n window flags\n", argv[0]); return 2; }
  const uint64_t seed = strtoull(argv[1], nullptr, 10);
  g_state = seed;
  const size_t K = strtoull(argv[2], nullptr, 10), n = strtoull(argv[3], nullptr, 10);
  fmh_ldscore_params P{};
  P.window = (uint32_t)strtoul(argv[4], nullptr, 10);
  P.flags = (uint32_t)strtoul(argv[5], nullptr, 10);
  if (const char* refused = fmh_host::ld_score_check_params(P)) { fprintf(stderr, "refused: %s\n", refused); return 2; }
  if (n == 0) { fprintf(stderr, "refused: n is 0\n"); return 2; }

  constexpr size_t F = 4;
  std::vector<uint8_t> founder(F * K);
  for (size_t f = 0; f < F; ++f)
    for (size_t k = 0; k < K; ++k) founder[f * K + k] = (uint8_t)(rnd() % 2);
  std::vector<uint8_t> dosage(K * n, 0);
  for (size_t i = 0; i < n; ++i)
    for (size_t h = 0; h < 2; ++h)
      for (size_t k = 0; k < K;) {
        const size_t len = 10 + rnd() % 40, src = rnd() % F;
        for (size_t j = 0; j < len && k < K; ++j, ++k) {
          const uint64_t r = rnd() % 100;
          dosage[k * n + i] += (uint8_t)(r < 2 ? 1 - founder[src * K + k] : founder[src * K + k]);
        }
      }
  for (size_t i = 0; i < K * n; ++i)
    if (rnd() % 100 < 3) dosage[i] = 3;
  std::vector<uint32_t> x(K);
  for (size_t k = 0; k < K; ++k) x[k] = (k ? x[k - 1] : 0) + (uint32_t)(rnd() % 4);

  std::vector<int64_t> q(K);
  std::vector<uint32_t> partners(K), counted(K);
  std::vector<double> score(K);
  fmh_host::ld_scores_host(dosage.data(), x.data(), K, n, P, q.data(), partners.data(), counted.data());
  fmh_host::ld_score_values(q.data(), counted.data(), K, score.data());
  uint64_t h = 0, terms = 0;
  for (size_t k = 0; k < K; ++k) {
    h += (uint64_t)q[k] * (0x9E3779B97F4A7C15ull * (k + 1)) + (uint64_t)counted[k] * (2 * k + 1) + (uint64_t)partners[k] * (4 * k + 3) + bits_of(score[k]) * (6 * k + 5);
    terms += counted[k];
  }
  printf("ldscore_host_check: %zu rows x %zu samples, %llu terms, checksum %016llx\n", K, n, (unsigned long long)terms, (unsigned long long)h);

  // the regression over a drawn chi^2 column, four blocks
  std::vector<double> chi2(K);
  g_state = seed + 1;
  for (size_t k = 0; k < K; ++k) chi2[k] = (double)(rnd() % 4096) / 1024.0;
  fmh_ldsc_out out{};
  const char* refused = fmh_host::ldsc_regress(chi2.data(), score.data(), nullptr, K, (double)n, (double)K, 4, nullptr, &out);
  if (refused) printf("ldscore_host_check: regression refused: %s\n", refused);
  else
    printf("ldscore_host_check: regression %016llx %016llx %016llx %016llx used %llu\n", (unsigned long long)bits_of(out.h2), (unsigned long long)bits_of(out.h2_se),
           (unsigned long long)bits_of(out.intercept), (unsigned long long)bits_of(out.intercept_se), (unsigned long long)out.n_used);
  return 0;
}
