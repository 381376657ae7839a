// roh_host_check.cpp — sanitizer check of the host twin of the runs of homozygosity (roh_host.hpp: roh_need, roh_scan_host,
// roh_segment_less) on a seeded planted cohort held in exact-size heap blocks, so that a read or write one element past the state table,
// the positions, a table or the segment buffer is an ASan report.  The cohort comes from a splitmix64 stream that tests/test_roh_cpu.py
// restates, the scan runs twice (once to count, once into a buffer of exactly that many segments) and the program prints an order-free
// checksum of the tables and segments, which the test compares with the oracle's (tests/roh_ref.py: checksum).  Before that, silently,
// the kept rows and the break bitmap the device entry point builds (segment_host_check.hpp), in the scan kernel's layout as well: 64 zero
// bits in front and zero words behind, for the smallest and the largest window.
// Built by `make asan` with -fsanitize=address,undefined -fno-sanitize-recover=all.
//   roh_host_check.asan seed K n window window_het window_missing threshold min_sites min_length max_gap max_bp_per_site max_het max_missing [edge ...]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "roh_host.hpp"
#include "segment_host_check.hpp"

static uint64_t g_state = 0;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main(int argc, char** argv) {
  if (argc < 14) { fprintf(stderr, "usage: %s seed K n window window_het window_missing threshold min_sites min_length max_gap max_bp_per_site max_het max_missing [edge ...]\n", argv[0]); return 2; }
  using namespace fmh_host;
  for (size_t offset : {(size_t)0, kRohBreakOffset})
    if (!check_kept_rows_and_breaks(offset, [&](size_t K) { return (K + offset + 63) / 64; })) return 1;
  for (size_t window : {(size_t)1, (size_t)kRohMaxWindow})
    if (!check_kept_rows_and_breaks(kRohBreakOffset, [&](size_t K) { return roh_break_words(K, window); })) return 1;
  g_state = strtoull(argv[1], nullptr, 10);
  const size_t K = strtoull(argv[2], nullptr, 10), n = strtoull(argv[3], nullptr, 10);
  fmh_roh_params p{};
  p.window = (uint32_t)strtoul(argv[4], nullptr, 10);
  p.window_het = (uint32_t)strtoul(argv[5], nullptr, 10);
  p.window_missing = (uint32_t)strtoul(argv[6], nullptr, 10);
  const double threshold = strtod(argv[7], nullptr);
  p.min_sites = (uint32_t)strtoul(argv[8], nullptr, 10);
  p.min_length = (uint32_t)strtoul(argv[9], nullptr, 10);
  p.max_gap = (uint32_t)strtoul(argv[10], nullptr, 10);
  p.max_bp_per_site = (uint32_t)strtoul(argv[11], nullptr, 10);
  p.max_het = (uint32_t)strtoul(argv[12], nullptr, 10);
  p.max_missing = (uint32_t)strtoul(argv[13], nullptr, 10);
  const int n_edges = argc - 14;
  if (n_edges > 7) { fprintf(stderr, "at most 7 edges\n"); return 2; }
  p.n_bins = n_edges ? (uint32_t)n_edges + 1 : 0;
  for (int e = 0; e < n_edges; ++e) p.bin_edges[e] = (uint32_t)strtoul(argv[14 + e], nullptr, 10);
  if (const char* refused = fmh_host::roh_check_params(p)) { fprintf(stderr, "refused: %s\n", refused); return 2; }
  if (const char* refused = fmh_host::roh_need(threshold, p.window, p.need)) { fprintf(stderr, "refused: %s\n", refused); return 2; }

  // the planted cohort: per sample alternating stretches, het 2 % and missing 2 % inside, het 40 % and missing 2 % outside
  std::vector<uint8_t> state(K * n);
  for (size_t i = 0; i < n; ++i) {
    bool inside = rnd() & 1;
    for (size_t k = 0; k < K; inside = !inside) {
      const size_t len = 10 + rnd() % 90;
      for (size_t j = 0; j < len && k < K; ++j, ++k) {
        const uint64_t r = rnd() % 1000;
        state[k * n + i] = inside ? (r < 20 ? 1 : r < 40 ? 2 : 0) : (r < 400 ? 1 : r < 420 ? 2 : 0);
      }
    }
  }
  std::vector<uint32_t> x(K);
  for (size_t k = 0; k < K; ++k) {
    const uint64_t jump = rnd() % 50 == 0 ? 3000000 : rnd() % 2000;
    x[k] = k ? x[k - 1] + (uint32_t)jump : (uint32_t)(rnd() % 1000);
  }

  const size_t nb = p.n_bins;
  std::vector<unsigned long long> t0(n), t1(n), t2(n), t3(n), b0(n * nb), b1(n * nb);
  const fmh_roh_out out{t0.data(), t1.data(), t2.data(), t3.data(), nb ? b0.data() : nullptr, nb ? b1.data() : nullptr};
  const fmh_roh_out none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  uint64_t count = 0, again = 0;
  fmh_host::roh_scan_host(state.data(), x.data(), K, n, p, none, nullptr, 0, &count);  // counted only
  std::vector<fmh_roh_segment> segments((size_t)count);
  fmh_host::roh_scan_host(state.data(), x.data(), K, n, p, out, segments.data(), segments.size(), &again);
  if (again != count) { fprintf(stderr, "the two calls count %llu and %llu runs\n", (unsigned long long)count, (unsigned long long)again); return 1; }
  std::sort(segments.begin(), segments.end(), fmh_host::roh_segment_less);

  uint64_t h = 0;
  for (const std::vector<unsigned long long>* t : {&t0, &t1, &t2, &t3}) {
    for (size_t i = 0; i < n; ++i) h += ((*t)[i] + 1) * (0x9E3779B97F4A7C15ull * (i + 1));
    h = h * 31 + 7;
  }
  for (const fmh_roh_segment& s : segments) {
    uint64_t e = 0;
    for (uint64_t v : {(uint64_t)s.sample, (uint64_t)s.n_sites, (uint64_t)s.n_het, (uint64_t)s.n_missing, s.first_row, s.last_row}) e = e * 1000003 + v + 1;
    h += e * e;
  }
  unsigned long long bins = 0;
  for (size_t i = 0; i < n * nb; ++i) bins += b0[i] * 3 + b1[i];
  printf("roh_host_check: %zu kept rows x %zu samples, %llu runs, bins %llu, checksum %016llx\n", K, n, (unsigned long long)count, bins,
         (unsigned long long)h);
  return 0;
}
