// logistic.hip — logistic association scan (score test): fmh_assoc_homalt_sums (per site the exact i64 sums of the value columns over the
// hom-alt genotypes, the int8 contraction of assoc.hip with another operand), fmh_logistic_null (host: the null model per phenotype and its
// value columns as i32 fixed point), fmh_logistic_score / fmh_logistic_score_host (score and variance per site and phenotype from the exact
// sums, one function on both sides) and fmh_logistic_stats (host: chi2, z, p, beta, se).  Kernels in logistic_kernels.hpp, host arithmetic in
// logistic_host.hpp; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.19.
#include <hip/hip_runtime.h>

#include <vector>

#include "abi_internal.hpp"
#include "logistic_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;
using namespace fmh_host;

namespace {

constexpr size_t kHomaltDefaultItemRows = 4096;       // FMH_ASSOC_ITEM_ROWS unset, as fmh_assoc_sums
constexpr int32_t kHomaltMaxValue = (int32_t)1 << 30;  // four signed base-256 digits

// the refusals fmh_logistic_score and its host twin share; *K = Pb * (c + 3)
int check_score_shape(size_t n_basis, size_t n_phenotypes, size_t* K) {
  if (n_phenotypes < 1) return fail(FMH_ERR_INVALID, "at least one phenotype is required");
  if (n_basis + 3 > kLogisticMaxColumns || n_phenotypes > kLogisticMaxColumns / (n_basis + 3))
    return fail(FMH_ERR_INVALID, "%zu phenotypes x (%zu basis columns + 3) exceed %zu value columns", n_phenotypes, n_basis, kLogisticMaxColumns);
  *K = n_phenotypes * (n_basis + 3);
  return FMH_OK;
}

}  // namespace

extern "C" int fmh_assoc_homalt_sums(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                                     const int32_t* h_values, size_t n_columns, long long* d_homalt_sum, void* stream) {
  // ---- every refusal, before any launch: fmh_assoc_sums' and in its order ----
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!h_values) return fail(FMH_ERR_INVALID, "NULL values");
  if (!d_homalt_sum) return fail(FMH_ERR_INVALID, "d_homalt_sum is NULL");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  if (n_samples > kLogisticMaxSamples) return fail(FMH_ERR_INVALID, "n_samples %zu exceeds 2^21: S + 2 H would leave 53 bits", n_samples);
  if (n_columns < 1 || n_columns > kAssocMaxColumns) return fail(FMH_ERR_INVALID, "%zu value columns: 1 to %u are taken", n_columns, kAssocMaxColumns);
  for (size_t i = 0; i < n_samples * n_columns; ++i)
    if (h_values[i] > kHomaltMaxValue || h_values[i] < -kHomaltMaxValue)
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

  const size_t item_rows = item_rows_of(options().assoc_item_rows, kHomaltDefaultItemRows);
  const size_t n_items = (row_count + item_rows - 1) / item_rows;
  FMH_TRY(check_item_count(n_items, "FMH_ASSOC_ITEM_ROWS"));

  std::vector<int32_t> rank;
  if (h_samples_or_null) {
    rank.assign(covered, -1);
    for (size_t i = 0; i < n; ++i) rank[h_samples_or_null[i]] = (int32_t)i;
  }

  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;
  int32_t *d_values = nullptr, *d_rank = nullptr;
  uint4* d_digits = nullptr;
  FMH_TRY(call.upload(h_values, n * K, &d_values));
  FMH_TRY(call.scratch.get(&d_digits, n_vectors));
  if (!rank.empty()) FMH_TRY(call.upload(rank.data(), rank.size(), &d_rank));

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
  a.dosage_sum = d_homalt_sum;
  a.called_sum = nullptr;

  FMH_TRY(call.start());
  hipLaunchKernelGGL(assoc_digits_kernel, dim3((unsigned)((n_vectors + 255) / 256)), dim3(256), 0, st, d_values, d_rank, (uint32_t)n, covered, (uint32_t)K,
                     vgroups, n_vectors, d_digits);
  HIP_TRY(hipGetLastError());
  size_t grid = 0;
  FMH_TRY(persistent_grid(reinterpret_cast<const void*>(assoc_homalt_kernel), kAssocThreads, 0, n_items, call.ws->cus, &grid, kAssocChunkVecs * sizeof(uint4)));
  hipLaunchKernelGGL(assoc_homalt_kernel, dim3((unsigned)grid), dim3(kAssocThreads), 0, st, a);
  HIP_TRY(hipGetLastError());
  return call.finish();
}

extern "C" int fmh_logistic_score(const long long* d_dosage_sum, const long long* d_called_sum, const long long* d_homalt_sum, const uint32_t* d_hom_ref,
                                  const uint32_t* d_het, const uint32_t* d_hom_alt, size_t n_rows, const long long* h_total, const int32_t* h_exponent,
                                  size_t n_basis, size_t n_phenotypes, double* d_score, double* d_variance, int device, void* stream) {
  size_t K = 0;
  FMH_TRY(check_score_shape(n_basis, n_phenotypes, &K));
  if (n_rows == 0) return FMH_OK;
  if (!d_dosage_sum || !d_called_sum || !d_homalt_sum || !d_hom_ref || !d_het || !d_hom_alt || !h_total || !h_exponent || !d_score || !d_variance)
    return fail(FMH_ERR_INVALID, "NULL argument");
  const size_t threads = n_rows * n_phenotypes;
  if (n_rows > ((size_t)1 << 56) || (threads + 255) / 256 > 0x7FFFFFFFu) return fail(FMH_ERR_UNSUPPORTED, "more than 2^39 (row, phenotype) pairs in one call");
  StatCall call;
  FMH_TRY(call.begin(device, stream));
  long long* d_total = nullptr;
  int32_t* d_exponent = nullptr;
  FMH_TRY(call.upload(h_total, K, &d_total));
  FMH_TRY(call.upload(h_exponent, K, &d_exponent));
  const LogisticScoreArgs a{d_dosage_sum, d_called_sum, d_homalt_sum, d_hom_ref, d_het, d_hom_alt, d_total, d_exponent, n_rows, (uint32_t)n_basis,
                            (uint32_t)n_phenotypes, d_score, d_variance};
  FMH_TRY(call.start());
  hipLaunchKernelGGL(logistic_score_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, call.st, a);
  HIP_TRY(hipGetLastError());
  return call.finish();
}

// ---- host only (no device).  The operation order is the header's; the unit is built with -ffp-contract=off ----------------------------------
extern "C" int fmh_logistic_score_host(const long long* h_dosage_sum, const long long* h_called_sum, const long long* h_homalt_sum,
                                       const uint32_t* h_hom_ref, const uint32_t* h_het, const uint32_t* h_hom_alt, size_t n_rows,
                                       const long long* h_total, const int32_t* h_exponent, size_t n_basis, size_t n_phenotypes, double* h_score,
                                       double* h_variance) {
  size_t K = 0;
  FMH_TRY(check_score_shape(n_basis, n_phenotypes, &K));
  if (n_rows == 0) return FMH_OK;
  if (!h_dosage_sum || !h_called_sum || !h_homalt_sum || !h_hom_ref || !h_het || !h_hom_alt || !h_total || !h_exponent || !h_score || !h_variance)
    return fail(FMH_ERR_INVALID, "NULL argument");
  const size_t Pb = n_phenotypes, W = n_basis + 3;
  for (size_t r = 0; r < n_rows; ++r)
    for (size_t p = 0; p < Pb; ++p)
      logistic_score_one(h_dosage_sum + r * K, h_called_sum + r * K, h_homalt_sum[r * Pb + p], h_hom_ref[r], h_het[r], h_hom_alt[r], h_total, h_exponent,
                         n_basis, p * W, h_score + r * Pb + p, h_variance + r * Pb + p);
  return FMH_OK;
}

extern "C" int fmh_logistic_null(const double* h_phenotypes, const double* h_covariates_or_null, size_t n, size_t n_phenotypes, size_t n_covariates,
                                 int32_t* h_values, int32_t* h_exponent, long long* h_total, uint8_t* h_fitted, int32_t* h_reason, int32_t* h_iterations,
                                 uint64_t* h_n_cases, size_t* h_n_basis, uint8_t* h_dropped_or_null) {
  const LogisticNullOut out{h_values, h_exponent, h_total, h_fitted, h_reason, h_iterations, h_n_cases, h_n_basis, h_dropped_or_null};
  const char* refused = logistic_null(h_phenotypes, h_covariates_or_null, n, n_phenotypes, n_covariates, out);
  if (refused) return fail(FMH_ERR_INVALID, "fmh_logistic_null (n = %zu, %zu phenotypes, %zu covariates): %s", n, n_phenotypes, n_covariates, refused);
  return FMH_OK;
}

extern "C" int fmh_logistic_stats(const double* h_score, const double* h_variance, size_t count, double* h_chi2, double* h_z, double* h_p, double* h_beta,
                                  double* h_se) {
  if (count == 0) return FMH_OK;
  if (!h_score || !h_variance) return fail(FMH_ERR_INVALID, "NULL argument");
  for (size_t i = 0; i < count; ++i) {
    double chi2, z, p, beta, se;
    logistic_stats_one(h_score[i], h_variance[i], &chi2, &z, &p, &beta, &se);
    if (h_chi2) h_chi2[i] = chi2;
    if (h_z) h_z[i] = z;
    if (h_p) h_p[i] = p;
    if (h_beta) h_beta[i] = beta;
    if (h_se) h_se[i] = se;
  }
  return FMH_OK;
}
