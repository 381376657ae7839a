// assoc.hip — single-variant association scan: fmh_assoc_sums (per site the exact i64 sums of the genotype dosage, and of the called flag,
// against K fixed-point value columns, an int8 contraction on the matrix cores straight from the bit planes), fmh_assoc_prepare (host: the
// centred, orthonormalised covariate basis and the residualised phenotypes as i32 fixed point) and fmh_assoc_stats (host: beta, se, t and p
// per site and phenotype from the sums and the QC tracks).  Kernels in assoc_kernels.hpp; definition in include/ferromic_hip.h, scheme in
// DESIGN.md section 3.18.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "abi_internal.hpp"
#include "assoc_host.hpp"
#include "assoc_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;
using namespace fmh_host;  // assoc_host.hpp: the arithmetic shared with the logistic null model

namespace {

constexpr size_t kAssocDefaultItemRows = 4096;
constexpr size_t kAssocMaxSamples = (size_t)1 << 22;  // a digit accumulator holds 2 * n * 128 <= 2^30
constexpr int32_t kAssocMaxValue = (int32_t)1 << 30;  // four signed base-256 digits

}  // namespace

extern "C" int fmh_assoc_sums(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                              const int32_t* h_values, size_t n_columns, long long* d_dosage_sum, long long* d_called_sum_or_null, void* stream) {
  // ---- every refusal, before any launch ----
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!h_values) return fail(FMH_ERR_INVALID, "NULL values");
  if (!d_dosage_sum) return fail(FMH_ERR_INVALID, "d_dosage_sum is NULL");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  if (n_samples > kAssocMaxSamples) return fail(FMH_ERR_INVALID, "n_samples %zu exceeds 2^22: a digit accumulator would leave 32 bits", n_samples);
  if (n_columns < 1 || n_columns > kAssocMaxColumns) return fail(FMH_ERR_INVALID, "%zu value columns: 1 to %u are taken", n_columns, kAssocMaxColumns);
  for (size_t i = 0; i < n_samples * n_columns; ++i)
    if (h_values[i] > kAssocMaxValue || h_values[i] < -kAssocMaxValue)
      return fail(FMH_ERR_INVALID, "value %d (sample entry %zu, column %zu) is beyond +-2^30", h_values[i], i / n_columns, i % n_columns);
  FMH_TRY(check_samples(h_samples_or_null, n_samples, m->samples));
  FMH_TRY(check_rows(row_begin, row_count, m->variants));
  if (m->ploidy != 2) return fail(FMH_ERR_UNSUPPORTED, "the association scan takes diploid genotypes (ploidy 2), got ploidy %zu", m->ploidy);
  FMH_TRY(check_packed(m, "the association scan reads"));
  if (row_count == 0) return FMH_OK;

  const size_t n = n_samples, K = n_columns;
  const uint32_t last = h_samples_or_null ? h_samples_or_null[n - 1] : (uint32_t)(n - 1);
  const uint32_t covered = last + 1;
  const uint32_t nvec = last / 64 + 1;  // 64 samples per 16 bytes of a row; within the row: sample `last` exists
  const uint32_t groups = (nvec + 3) / 4, vgroups = (uint32_t)((K + 15) / 16);
  const size_t n_vectors = (size_t)groups * vgroups * kAssocChunkVecs;

  const size_t item_rows = item_rows_of(options().assoc_item_rows, kAssocDefaultItemRows);
  const size_t n_items = (row_count + item_rows - 1) / item_rows;
  FMH_TRY(check_item_count(n_items, "FMH_ASSOC_ITEM_ROWS"));

  // a matrix that is biallelic with nothing missing calls every genotype: C is the column totals, no second contraction
  const bool complete = !m->pc && !m->p1 && !m->p2;
  const bool contract_called = d_called_sum_or_null && !complete;
  std::vector<long long> totals;
  if (d_called_sum_or_null && complete) {
    totals.assign(K, 0);
    for (size_t i = 0; i < n; ++i)
      for (size_t k = 0; k < K; ++k) totals[k] += h_values[i * K + k];
  }
  std::vector<int32_t> rank;
  if (h_samples_or_null) {
    rank.assign(covered, -1);
    for (size_t i = 0; i < n; ++i) rank[h_samples_or_null[i]] = (int32_t)i;
  }

  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;
  int32_t *d_values = nullptr, *d_rank = nullptr;
  long long* d_totals = nullptr;
  uint4* d_digits = nullptr;
  FMH_TRY(call.upload(h_values, n * K, &d_values));
  FMH_TRY(call.scratch.get(&d_digits, n_vectors));
  if (!rank.empty()) FMH_TRY(call.upload(rank.data(), rank.size(), &d_rank));
  if (!totals.empty()) FMH_TRY(call.upload(totals.data(), K, &d_totals));

  AssocArgs a{};
  set_plane_rows(a, m);
  a.nvec = nvec;
  a.groups = groups;
  a.columns = (uint32_t)K;
  a.vgroups = vgroups;
  a.digits = d_digits;
  a.row_begin = row_begin;
  a.row_count = row_count;
  a.item_rows = (uint32_t)item_rows;
  a.n_items = (uint32_t)n_items;
  a.dosage_sum = d_dosage_sum;
  a.called_sum = contract_called ? d_called_sum_or_null : nullptr;

  FMH_TRY(call.start());
  hipLaunchKernelGGL(assoc_digits_kernel, dim3((unsigned)((n_vectors + 255) / 256)), dim3(256), 0, st, d_values, d_rank, (uint32_t)n, covered, (uint32_t)K,
                     vgroups, n_vectors, d_digits);
  HIP_TRY(hipGetLastError());
  {
    void (*kernel)(const AssocArgs) = contract_called ? assoc_sums_kernel<true> : assoc_sums_kernel<false>;
    size_t grid = 0;
    FMH_TRY(persistent_grid(reinterpret_cast<const void*>(kernel), kAssocThreads, 0, n_items, call.ws->cus, &grid, kAssocChunkVecs * sizeof(uint4)));
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kAssocThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  if (d_totals) {
    const size_t count = row_count * K;
    hipLaunchKernelGGL(assoc_fill_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, d_totals, (uint32_t)K, count, d_called_sum_or_null);
    HIP_TRY(hipGetLastError());
  }
  return call.finish();
}

// ---- host only (no device).  The operation order is the header's; the unit is built with -ffp-contract=off ----------------------------------
extern "C" int fmh_assoc_prepare(const double* h_phenotypes, const double* h_covariates_or_null, size_t n, size_t n_phenotypes, size_t n_covariates,
                                 int32_t* h_values, int32_t* h_exponent, long long* h_total, double* h_yy, size_t* h_n_basis,
                                 uint8_t* h_dropped_or_null) {
  if (!h_phenotypes || !h_values || !h_exponent || !h_total || !h_yy || !h_n_basis) return fail(FMH_ERR_INVALID, "NULL argument");
  if (n_covariates != 0 && !h_covariates_or_null) return fail(FMH_ERR_INVALID, "%zu covariates but the pointer is NULL", n_covariates);
  if (n_phenotypes < 1) return fail(FMH_ERR_INVALID, "at least one phenotype is required");
  if (n == 0 || n > kAssocMaxSamples) return fail(FMH_ERR_INVALID, "n = %zu: 1 to 2^22 samples are taken", n);
  const size_t P = n_phenotypes, cin = n_covariates;
  for (size_t i = 0; i < n * P; ++i)
    if (!std::isfinite(h_phenotypes[i])) return fail(FMH_ERR_INVALID, "phenotype %zu of sample entry %zu is not finite", i % P, i / P);
  for (size_t i = 0; i < n * cin; ++i)
    if (!std::isfinite(h_covariates_or_null[i])) return fail(FMH_ERR_INVALID, "covariate %zu of sample entry %zu is not finite", i % cin, i / cin);

  // covariates: centre, orthogonalise against the kept columns (modified Gram-Schmidt, twice), drop or normalise
  std::vector<double> q;  // kept columns, column-major
  std::vector<double> x(n);
  const size_t c = covariate_basis(h_covariates_or_null, n, cin, q, h_dropped_or_null);
  if (n < c + 3) return fail(FMH_ERR_INVALID, "n - c - 2 = %lld residual degrees of freedom: at least 1 is required", (long long)n - (long long)c - 2);
  if (c + P > kAssocMaxColumns) return fail(FMH_ERR_INVALID, "%zu kept covariates + %zu phenotypes exceed %u value columns", c, P, kAssocMaxColumns);
  const size_t K = c + P;
  *h_n_basis = c;

  auto quantise = [&](const double* col, size_t k) { quantise_column(col, n, h_values + k, K, h_exponent + k, h_total + k); };
  for (size_t j = 0; j < c; ++j) quantise(q.data() + j * n, j);
  for (size_t p = 0; p < P; ++p) {
    for (size_t i = 0; i < n; ++i) x[i] = h_phenotypes[i * P + p];
    centre(x.data(), n);
    project_off(x.data(), q, c, n);
    quantise(x.data(), c + p);
    double yy = 0.0;
    for (size_t i = 0; i < n; ++i) {
      const double v = std::ldexp((double)h_values[i * K + c + p], -h_exponent[c + p]);
      yy += v * v;
    }
    h_yy[p] = yy;
  }
  return FMH_OK;
}

extern "C" int fmh_assoc_stats(const long long* h_dosage_sum, const long long* h_called_sum, const uint32_t* h_hom_ref, const uint32_t* h_het,
                               const uint32_t* h_hom_alt, size_t n_rows, const long long* h_total, const int32_t* h_exponent, const double* h_yy,
                               uint64_t n_samples, size_t n_basis, size_t n_phenotypes, double* h_beta, double* h_se, double* h_t, double* h_p) {
  if (n_phenotypes < 1) return fail(FMH_ERR_INVALID, "at least one phenotype is required");
  if (n_basis + n_phenotypes > kAssocMaxColumns) return fail(FMH_ERR_INVALID, "%zu + %zu value columns exceed %u", n_basis, n_phenotypes, kAssocMaxColumns);
  if (n_samples > kAssocMaxSamples || n_samples < n_basis + 3)
    return fail(FMH_ERR_INVALID, "n = %llu with %zu basis columns: n <= 2^22 and n - c - 2 >= 1 are required", (unsigned long long)n_samples, n_basis);
  if (n_rows == 0) return FMH_OK;
  if (!h_dosage_sum || !h_called_sum || !h_hom_ref || !h_het || !h_hom_alt || !h_total || !h_exponent || !h_yy) return fail(FMH_ERR_INVALID, "NULL argument");
  const size_t c = n_basis, P = n_phenotypes, K = c + P;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const uint64_t df = n_samples - c - 2;
  auto put = [&](double* out, size_t i, double v) { if (out) out[i] = v; };
  for (size_t r = 0; r < n_rows; ++r) {
    const long long *S = h_dosage_sum + r * K, *C = h_called_sum + r * K;
    const uint64_t het = h_het[r], alt = h_hom_alt[r], N = (uint64_t)h_hom_ref[r] + het + alt, n_alt = het + 2 * alt;
    double D = nan, mu = 0.0;
    if (N != 0) {
      mu = (double)n_alt / (double)N;
      D = (double)(het + 4 * alt) - (double)(n_alt * n_alt) / (double)N;
      for (size_t k = 0; k < c; ++k) {
        const double a = std::ldexp((double)S[k] + mu * (double)(h_total[k] - C[k]), -h_exponent[k]);
        D = D - a * a;
      }
    }
    for (size_t p = 0; p < P; ++p) {
      const size_t o = r * P + p, k = c + p;
      if (!(D > 0.0)) {  // N == 0 too
        put(h_beta, o, nan); put(h_se, o, nan); put(h_t, o, nan); put(h_p, o, nan);
        continue;
      }
      const double a = std::ldexp((double)S[k] + mu * (double)(h_total[k] - C[k]), -h_exponent[k]);
      const double beta = a / D;
      double rss = h_yy[p] - a * a / D;
      if (rss < 0.0) rss = 0.0;
      const double se = std::sqrt(rss / (double)df / D);
      put(h_beta, o, beta);
      put(h_se, o, se);
      if (se == 0.0) {
        put(h_t, o, nan); put(h_p, o, nan);
        continue;
      }
      const double t = beta / se;
      put(h_t, o, t);
      put(h_p, o, student_t_two_sided(t, (double)df));
    }
  }
  return FMH_OK;
}
