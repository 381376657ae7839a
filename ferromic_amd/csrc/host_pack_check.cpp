// host_pack_check.cpp — sanitizer check of the host-side packer (host_pack.hpp, what fmh_matrix_create runs on every upload):
// random u8 matrices of ragged widths, with and without a missing bitset, alleles inside and above the plane range, packed by
// pack_rows_host in row ranges (as upload.hip's threads do) and compared bit for bit with a column-by-column restatement.
// Then the host arithmetic of the logistic association scan (logistic_host.hpp: the null model, the score function's host side, the
// statistics) on exact-size heap blocks: ragged sample counts, dropped covariates, several phenotype batches, a one-class and a separated
// phenotype, rows without variation.
// Built by `make asan` with -fsanitize=address,undefined -fno-sanitize-recover=all; exits 0 and prints one line per part when every case agrees.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "host_pack.hpp"
#include "logistic_host.hpp"

// fmh_logistic_null, logistic_score_one and logistic_stats_one over small random cohorts; 0 when every invariant holds
static int logistic_check(std::mt19937_64& rng, int cases) {
  using namespace fmh_host;
  size_t fitted_total = 0, scored = 0;
  for (int t = 0; t < cases; ++t) {
    const size_t n = 8 + rng() % 90, cin = rng() % 7, P = 1 + rng() % 12;
    std::vector<double> y(n * P), x(n * cin);
    for (auto& v : x) v = (double)(rng() % 2001) / 100.0 - 10.0;
    if (cin >= 3)
      for (size_t i = 0; i < n; ++i) x[i * cin + 2] = 2.0 * x[i * cin] + 1.0;  // collinear: dropped
    for (auto& v : y) v = rng() % 3 == 0 ? 1.0 : 0.0;
    for (size_t i = 0; i < n; ++i) y[i * P] = 0.0;                              // no case
    if (P > 1 && cin)
      for (size_t i = 0; i < n; ++i) y[i * P + 1] = x[i * cin] > 0.0 ? 1.0 : 0.0;  // separated by the first covariate
    const size_t Win = cin + 3;
    std::vector<int32_t> values(n * P * Win, 0x5A5A5A5A), exponent(P * Win), reason(P), iterations(P);
    std::vector<long long> total(P * Win);
    std::vector<uint8_t> fitted(P), dropped(cin ? cin : 1);
    std::vector<uint64_t> n_cases(P);
    size_t c = 0;
    const LogisticNullOut out{values.data(), exponent.data(), total.data(), fitted.data(), reason.data(), iterations.data(), n_cases.data(), &c, dropped.data()};
    const char* refused = logistic_null(y.data(), cin ? x.data() : nullptr, n, P, cin, out);
    if (n < cin + 3 && refused) continue;  // too few samples for the kept covariates: a refusal, nothing to look at
    if (refused) { fprintf(stderr, "logistic case %d: refused: %s\n", t, refused); return 1; }
    if (cin >= 3 && !dropped[2]) { fprintf(stderr, "logistic case %d: the collinear covariate was kept\n", t); return 1; }
    if (fitted[0] || reason[0] != kLogisticOneClass) { fprintf(stderr, "logistic case %d: the phenotype without a case was fitted\n", t); return 1; }
    if (P > 1 && cin && !dropped[0] && fitted[1]) { fprintf(stderr, "logistic case %d: the separated phenotype was fitted\n", t); return 1; }
    const size_t W = c + 3, B = kLogisticMaxColumns / W;
    for (size_t first = 0; first < P; first += B) {
      const size_t Pb = P - first < B ? P - first : B, K = Pb * W;
      const int32_t* v = values.data() + n * W * first;
      for (size_t k = 0; k < K; ++k) {  // the totals are the column sums, every entry within +-2^30
        long long s = 0;
        for (size_t i = 0; i < n; ++i) {
          if (v[i * K + k] > (1 << 30) || v[i * K + k] < -(1 << 30)) { fprintf(stderr, "logistic case %d: a value beyond 2^30\n", t); return 1; }
          s += v[i * K + k];
        }
        if (s != total[first * W + k]) { fprintf(stderr, "logistic case %d: total of column %zu\n", t, k); return 1; }
      }
      // one row of random genotypes through the score function and the statistics
      std::vector<long long> S(K, 0), C(K, 0), H(Pb, 0);
      uint32_t cls[3] = {0, 0, 0};
      const unsigned kind = (unsigned)(rng() % 4);  // 0: random, 1: all ref, 2: all alt, 3: nothing called
      for (size_t i = 0; i < n; ++i) {
        const bool called = kind != 3 && rng() % 10 != 0;
        const unsigned g = kind == 1 ? 0 : kind == 2 ? 2 : (unsigned)(rng() % 3);
        if (!called) continue;
        ++cls[g];
        for (size_t k = 0; k < K; ++k) { S[k] += (long long)g * v[i * K + k]; C[k] += v[i * K + k]; }
        if (g == 2)
          for (size_t p = 0; p < Pb; ++p) H[p] += v[i * K + p * W + c + 2];
      }
      for (size_t p = 0; p < Pb; ++p) {
        double U, Vr, st[5];
        logistic_score_one(S.data(), C.data(), H[p], cls[0], cls[1], cls[2], total.data() + first * W, exponent.data() + first * W, c, p * W, &U, &Vr);
        logistic_stats_one(U, Vr, st, st + 1, st + 2, st + 3, st + 4);
        if (kind != 0 && (U == U || Vr == Vr)) { fprintf(stderr, "logistic case %d: a row without variation carries a score\n", t); return 1; }
        if (fitted[first + p] && Vr > 0.0 && !(st[2] >= 0.0 && st[2] <= 1.0)) { fprintf(stderr, "logistic case %d: p = %g\n", t, st[2]); return 1; }
        fitted_total += fitted[first + p];
        ++scored;
      }
    }
  }
  printf("logistic_host_check: %d cases, %zu (row, phenotype) scores, %zu of fitted phenotypes ok\n", cases, scored, fitted_total);
  return fitted_total ? 0 : 1;
}

int main(int argc, char** argv) {
  const int cases = argc > 1 ? atoi(argv[1]) : 400;
  std::mt19937_64 rng(20251004);
  size_t checked = 0;
  for (int c = 0; c < cases; ++c) {
    const size_t rows = 1 + rng() % 40, columns = 1 + rng() % 300;
    const int nplanes = 1 + (int)(rng() % 3);
    const bool with_missing = rng() % 2 == 0;
    const unsigned max_allele = (1u << nplanes) - 1;
    const bool overflow_wanted = rng() % 5 == 0;
    const size_t pitch = ((columns + 7) / 8 + 15) / 16 * 16, total = rows * columns;
    // exact-size heap blocks: a read or write one byte past the matrix, the bitset or a plane is an ASan report
    std::vector<uint8_t> data(total);
    for (auto& v : data) v = (uint8_t)(rng() % (max_allele + 1));
    std::vector<uint64_t> missing((total + 63) / 64, 0);
    if (with_missing)
      for (size_t i = 0; i < total; ++i)
        if (rng() % 7 == 0) missing[i >> 6] |= 1ull << (i & 63);
    bool expect_overflow = false;
    if (overflow_wanted) {
      const size_t at = rng() % total;
      data[at] = (uint8_t)(max_allele + 1 + rng() % 3);
      expect_overflow = !(with_missing && ((missing[at >> 6] >> (at & 63)) & 1));  // a missing entry's value is never looked at
    }
    const int planes_total = nplanes + (with_missing ? 1 : 0);
    std::vector<uint8_t> dst((size_t)planes_total * rows * pitch, 0xAB);
    bool overflow = false;
    const size_t cut = rng() % (rows + 1);  // two row ranges, like two packer threads
    overflow |= fmh_host::pack_rows_host(data.data(), with_missing ? missing.data() : nullptr, columns, total, 0, cut, nplanes, with_missing, dst.data(), 0, rows, pitch);
    overflow |= fmh_host::pack_rows_host(data.data(), with_missing ? missing.data() : nullptr, columns, total, cut, rows, nplanes, with_missing, dst.data(), 0, rows, pitch);
    if (overflow != expect_overflow) { fprintf(stderr, "case %d: overflow flag %d, expected %d\n", c, (int)overflow, (int)expect_overflow); return 1; }
    for (size_t r = 0; r < rows; ++r)
      for (size_t b = 0; b < pitch * 8; ++b) {
        const bool inside = b < columns;
        const size_t idx = r * columns + b;
        const bool miss = inside && with_missing && ((missing[idx >> 6] >> (idx & 63)) & 1);
        for (int k = 0; k < planes_total; ++k) {
          const int got = (dst[((size_t)k * rows + r) * pitch + (b >> 3)] >> (b & 7)) & 1;
          int want = 0;
          if (inside) want = k < nplanes ? ((data[idx] >> k) & 1) : (miss ? 0 : 1);
          // value bits of a missing entry are whatever the row holds (the sweeps AND them with the called plane; unpack masks them)
          if (inside && k < nplanes && miss) continue;
          if (got != want) { fprintf(stderr, "case %d: row %zu column %zu plane %d: %d, expected %d\n", c, r, b, k, got, want); return 1; }
          ++checked;
        }
      }
  }
  printf("host_pack_check: %d cases, %zu bits ok\n", cases, checked);
  return logistic_check(rng, cases < 60 ? cases : 60);
}
