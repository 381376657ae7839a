// admix_host_check.cpp — sanitizer check of the host arithmetic of the admixture model (admix_host.hpp: admix_tracks, admix_start,
// admix_step_host, admix_accelerate) on a seeded cohort held in exact-size heap blocks, so that a read or write one element past the dosage
// table, a state array or a track is an ASan report.  The cohort comes from a splitmix64 stream that tests/admix_ref.py restates.  The program
// runs the default start, three EM steps (the last with only Q updated) and one extrapolation, and prints a checksum of the tracks and of the
// bits of every state on the way - none of which goes through log - and the log-likelihood of the start in text.  tests/test_admix_cpu.py
// compares the lines of a plain build, of this build and of the library's own entry points.
// Built by `make asan` with -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off.
//   admix_host_check.asan seed rows n K
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "admix_host.hpp"

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
  if (argc != 5) { fprintf(stderr, "usage: %s seed rows n K\n", argv[0]); return 2; }
  g_state = strtoull(argv[1], nullptr, 10);
  const size_t rows = strtoull(argv[2], nullptr, 10), n = strtoull(argv[3], nullptr, 10), K = strtoull(argv[4], nullptr, 10);
  if (n == 0 || K < 1 || K > fmh_host::kAdmixMaxK) { fprintf(stderr, "refused: n is 0 or K outside 1 .. 16\n"); return 2; }

  // the cohort: per row an allele frequency of t / 16 (t = 0 .. 16: monomorphic rows at both ends), two draws per genotype; a tenth of the rows
  // lose a quarter of their calls, one row in 32 all of them
  std::vector<uint8_t> dosage(rows * n);
  for (size_t k = 0; k < rows; ++k) {
    const uint64_t t = rnd() % 17, gaps = rnd() % 32;
    for (size_t s = 0; s < n; ++s) {
      uint8_t g = (uint8_t)((rnd() % 16 < t) + (rnd() % 16 < t));
      if (gaps == 0 || (gaps < 4 && rnd() % 4 == 0)) g = 3;
      dosage[k * n + s] = g;
    }
  }

  std::vector<uint8_t> usable(rows);
  std::vector<uint32_t> called(rows), allele_count(rows);
  std::vector<uint64_t> sites(n);
  const size_t m = fmh_host::admix_tracks(dosage.data(), rows, n, usable.data(), called.data(), allele_count.data(), sites.data());
  std::vector<uint32_t> cu, au;
  for (size_t r = 0; r < rows; ++r)
    if (usable[r]) { cu.push_back(called[r]); au.push_back(allele_count[r]); }
  cu.shrink_to_fit();
  au.shrink_to_fit();

  std::vector<double> q[5], f[5];
  for (int s = 0; s < 5; ++s) { q[s].assign(n * K, 0.0); f[s].assign(m * K, 0.0); }
  fmh_host::admix_start(cu.data(), au.data(), m, n, K, g_state, q[0].data(), f[0].data());
  double ll = 0.0;
  fmh_host::admix_step_host(dosage.data(), rows, n, K, q[0].data(), f[0].data(), q[1].data(), f[1].data(), &ll, fmh_host::kAdmixUpdateQ | fmh_host::kAdmixUpdateF);
  fmh_host::admix_step_host(dosage.data(), rows, n, K, q[1].data(), f[1].data(), q[2].data(), f[2].data(), nullptr, fmh_host::kAdmixUpdateQ | fmh_host::kAdmixUpdateF);
  const double alpha = fmh_host::admix_accelerate(q[0].data(), f[0].data(), q[1].data(), f[1].data(), q[2].data(), f[2].data(), n, m, K, q[3].data(), f[3].data());
  fmh_host::admix_step_host(dosage.data(), rows, n, K, q[3].data(), f[3].data(), q[4].data(), f[4].data(), nullptr, fmh_host::kAdmixUpdateQ);

  uint64_t h = m * 1000003ull + bits_of(alpha);
  for (size_t r = 0; r < rows; ++r)
    h += (uint64_t)(usable[r] + 1) * (0x9E3779B97F4A7C15ull * (r + 1)) + (uint64_t)called[r] * (2 * r + 1) + (uint64_t)allele_count[r] * (2 * r + 3);
  for (size_t i = 0; i < n; ++i) h += sites[i] * (0xBF58476D1CE4E5B9ull + i);
  for (int s = 0; s < 5; ++s) {
    for (size_t e = 0; e < n * K; ++e) h += bits_of(q[s][e]) * (2 * e + 5 + 2 * (uint64_t)s);
    for (size_t e = 0; e < m * K; ++e) h += bits_of(f[s][e]) * (2 * e + 7 + 2 * (uint64_t)s);
  }
  printf("admix_host_check: %zu rows x %zu samples, K %zu, %zu usable, checksum %016llx\n", rows, n, K, m, (unsigned long long)h);
  printf("loglik %.17g alpha %.17g\n", ll, alpha);
  return 0;
}
