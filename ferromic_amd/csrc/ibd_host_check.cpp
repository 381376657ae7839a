// ibd_host_check.cpp — sanitizer check of the host twin of the IBD segments (ibd_host.hpp: ibd_scan_host, ibd_segment_less) on a seeded
// cohort with planted sharing, held in exact-size heap blocks, so that a read or write one element past the dosage table, the positions, a
// table or the segment buffer is an ASan report.  The cohort comes from a splitmix64 stream that tests/test_ibd_cpu.py restates, the scan
// runs twice (once to count, once into a buffer of exactly that many segments) and the program prints an order-free checksum of the tables
// and segments, which the test compares with the oracle's (tests/ibd_ref.py: checksum).  Before that, silently, the kept rows and the
// break bitmap the device entry point builds (segment_host_check.hpp): break(k) at bit k of ceil(K / 64) words, and at bit k + 64.
// Built by `make asan` with -fsanitize=address,undefined -fno-sanitize-recover=all.
//   ibd_host_check.asan seed K n mode min_sites min_length max_gap max_bp_per_site max_missing
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ibd_host.hpp"
#include "segment_host_check.hpp"

static uint64_t g_state = 0;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main(int argc, char** argv) {
  if (argc != 10) { fprintf(stderr, "usage: %s seed K n mode min_sites min_length max_gap max_bp_per_site max_missing\n", argv[0]); return 2; }
  for (size_t offset : {(size_t)0, (size_t)64})
    if (!fmh_host::check_kept_rows_and_breaks(offset, [&](size_t K) { return (K + offset + 63) / 64; })) return 1;
  g_state = strtoull(argv[1], nullptr, 10);
  const size_t K = strtoull(argv[2], nullptr, 10), n = strtoull(argv[3], nullptr, 10);
  fmh_ibd_params p{};
  p.mode = (uint32_t)strtoul(argv[4], nullptr, 10);
  p.min_sites = (uint32_t)strtoul(argv[5], nullptr, 10);
  p.min_length = (uint32_t)strtoul(argv[6], nullptr, 10);
  p.max_gap = (uint32_t)strtoul(argv[7], nullptr, 10);
  p.max_bp_per_site = (uint32_t)strtoul(argv[8], nullptr, 10);
  p.max_missing = (uint32_t)strtoul(argv[9], nullptr, 10);
  if (const char* refused = fmh_host::ibd_check_params(p)) { fprintf(stderr, "refused: %s\n", refused); return 2; }
  if (n == 0) { fprintf(stderr, "refused: n is 0\n"); return 2; }

  // the cohort: three founder tracks of dosages; per sample stretches of 5..64 rows that copy a founder (5 % of the rows redrawn) or are
  // drawn afresh; 2 % of the genotypes not called
  constexpr size_t F = 3;
  std::vector<uint8_t> founder(F * K);
  for (size_t f = 0; f < F; ++f)
    for (size_t k = 0; k < K; ++k) founder[f * K + k] = (uint8_t)(rnd() % 3);
  std::vector<uint8_t> dosage(K * n);
  for (size_t i = 0; i < n; ++i) {
    for (size_t k = 0; k < K;) {
      const size_t len = 5 + rnd() % 60;
      const size_t src = rnd() % (F + 1);
      for (size_t j = 0; j < len && k < K; ++j, ++k) {
        const uint64_t r = rnd() % 1000;
        dosage[k * n + i] = r < 20 ? 3 : (src < F && r >= 70) ? founder[src * K + k] : (uint8_t)(r % 3);
      }
    }
  }
  std::vector<uint32_t> x(K);
  for (size_t k = 0; k < K; ++k) {
    const uint64_t jump = rnd() % 50 == 0 ? 3000000 : rnd() % 2000;
    x[k] = k ? x[k - 1] + (uint32_t)jump : (uint32_t)(rnd() % 1000);
  }

  std::vector<unsigned long long> t0(n * n), t1(n * n), t2(n * n), t3(n * n);
  const fmh_ibd_out out{t0.data(), t1.data(), t2.data(), t3.data()};
  const fmh_ibd_out none{nullptr, nullptr, nullptr, nullptr};
  uint64_t count = 0, again = 0;
  fmh_host::ibd_scan_host(dosage.data(), x.data(), K, n, p, none, nullptr, 0, &count);  // counted only
  std::vector<fmh_ibd_segment> segments((size_t)count);
  fmh_host::ibd_scan_host(dosage.data(), x.data(), K, n, p, out, segments.data(), segments.size(), &again);
  if (again != count) { fprintf(stderr, "the two calls count %llu and %llu runs\n", (unsigned long long)count, (unsigned long long)again); return 1; }
  std::sort(segments.begin(), segments.end(), fmh_host::ibd_segment_less);

  uint64_t h = 0;
  for (const std::vector<unsigned long long>* t : {&t0, &t1, &t2, &t3}) {
    for (size_t i = 0; i < n * n; ++i) h += ((*t)[i] + 1) * (0x9E3779B97F4A7C15ull * (i + 1));
    h = h * 31 + 7;
  }
  for (const fmh_ibd_segment& s : segments) {
    uint64_t e = 0;
    for (uint64_t v : {(uint64_t)s.a, (uint64_t)s.b, (uint64_t)s.n_sites, (uint64_t)s.n_missing, s.first_row, s.last_row}) e = e * 1000003 + v + 1;
    h += e * e;
  }
  printf("ibd_host_check: %zu kept rows x %zu samples, mode %u, %llu runs, checksum %016llx\n", K, n, p.mode, (unsigned long long)count,
         (unsigned long long)h);
  return 0;
}
