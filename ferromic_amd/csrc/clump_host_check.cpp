// clump_host_check.cpp — sanitizer check of the host twins of LD clumping (clump_host.hpp: clump_host, geno_ld_pairs_host, geno_ld_r2) on a
// seeded founder-mosaic cohort held in exact-size heap blocks, so that a read or write one element past the dosage table, the positions, the
// p values or an output is an ASan report.  The cohort comes from a splitmix64 stream that tests/clump_ref.py restates; the program prints an
// order-free checksum of the assignment, the r^2 bits and the counts of the (index, member) pairs, which tests/test_clump_cpu.py compares
// with the oracle's (tests/clump_ref.py: checksum).
// Built by `make asan` with -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off.
//   clump_host_check.asan seed K n p1 p2 r2 window
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "clump_host.hpp"

static uint64_t g_state = 0;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main(int argc, char** argv) {
  if (argc != 8) { fprintf(stderr, "usage: %s seed K n p1 p2 r2 window\n", argv[0]); return 2; }
  g_state = strtoull(argv[1], nullptr, 10);
  const size_t K = strtoull(argv[2], nullptr, 10), n = strtoull(argv[3], nullptr, 10);
  fmh_clump_params P{};
  P.p1 = strtod(argv[4], nullptr); P.p2 = strtod(argv[5], nullptr); P.r2 = strtod(argv[6], nullptr);
  P.window = (uint32_t)strtoul(argv[7], nullptr, 10);
  if (const char* refused = fmh_host::clump_check_params(P)) { fprintf(stderr, "refused: %s\n", refused); return 2; }
  if (n == 0) { fprintf(stderr, "refused: n is 0\n"); return 2; }

  // the cohort: four founder haplotype tracks; each of a sample's two haplotypes copies a founder over stretches of 10..49 rows (2 % of the
  // copied alleles flipped); 3 % of the genotypes not called
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
  std::vector<double> p(K);
  for (size_t k = 0; k < K; ++k) {
    const uint64_t r = rnd() % 1000;
    p[k] = r < 20 ? std::numeric_limits<double>::quiet_NaN() : r < 40 ? 0.0 : (double)(rnd() % 4096) / 40960.0;  // ties, zeros and NaN
  }

  std::vector<uint32_t> index_of(K);
  std::vector<double> r2(K);
  uint64_t n_clumps = 0;
  fmh_host::clump_host(dosage.data(), x.data(), p.data(), K, n, P, index_of.data(), r2.data(), &n_clumps);
  std::vector<uint32_t> a, b;
  for (size_t k = 0; k < K; ++k)
    if (index_of[k] != fmh_host::kClumpNone) { a.push_back(index_of[k]); b.push_back((uint32_t)k); }
  std::vector<fmh_geno_ld_counts> counts(a.size());
  fmh_host::geno_ld_pairs_host(dosage.data(), n, a.data(), b.data(), a.size(), counts.data());

  uint64_t h = n_clumps;
  for (size_t k = 0; k < K; ++k) {
    uint64_t bits;
    memcpy(&bits, &r2[k], sizeof bits);
    if (r2[k] != r2[k]) bits = 0x7FF8000000000000ull;  // every NaN alike
    h += ((uint64_t)index_of[k] + 1) * (0x9E3779B97F4A7C15ull * (k + 1)) + bits * (2 * k + 1);
  }
  for (size_t i = 0; i < counts.size(); ++i) {
    uint64_t e = 0;
    for (uint64_t v : {(uint64_t)b[i], (uint64_t)counts[i].n, (uint64_t)counts[i].sum_a, (uint64_t)counts[i].sum_b, (uint64_t)counts[i].sq_a, (uint64_t)counts[i].sq_b,
                       (uint64_t)counts[i].cross})
      e = e * 1000003 + v + 1;
    h += e * e;
    if (fmh_host::geno_ld_r2(counts[i]) != r2[b[i]] && r2[b[i]] == r2[b[i]]) { fprintf(stderr, "row %u: the counts' r2 differs from the twin's\n", b[i]); return 1; }
  }
  printf("clump_host_check: %zu rows x %zu samples, %llu clumps, %zu owned, checksum %016llx\n", K, n, (unsigned long long)n_clumps, a.size(), (unsigned long long)h);
  return 0;
}
