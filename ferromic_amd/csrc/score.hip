// score.hip — polygenic scores: fmh_score_sums (per sample the exact i64 sums of the genotype dosage, and of the called flag, against K
// fixed-point weight columns - the contraction of assoc.hip transposed: over rows, per sample, on the int8 matrix cores straight from the bit
// planes), fmh_score_exponents / fmh_score_values (host: the weights, and their products with the row's mean dosage, as i32 fixed point) and
// fmh_score_stats (host: the score per sample and column from the sums).  Kernels in score_kernels.hpp; definition in
// include/ferromic_hip.h, scheme in DESIGN.md section 3.20.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "abi_internal.hpp"
#include "score_host.hpp"
#include "score_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;
using namespace fmh_host;

namespace {

constexpr int32_t kScoreMaxValue = (int32_t)1 << 30;  // four signed base-256 digits

}  // namespace

extern "C" int fmh_score_sums(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                              const int32_t* h_dosage_values, const int32_t* h_called_values_or_null, size_t n_columns, long long* d_dosage_sum,
                              long long* d_called_sum_or_null, void* stream) {
  // ---- every refusal, before any launch ----
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!h_dosage_values) return fail(FMH_ERR_INVALID, "NULL values");
  if (!d_dosage_sum) return fail(FMH_ERR_INVALID, "d_dosage_sum is NULL");
  if (!h_called_values_or_null != !d_called_sum_or_null)
    return fail(FMH_ERR_INVALID, "the called values and d_called_sum go together: %s is NULL", h_called_values_or_null ? "d_called_sum" : "h_called_values");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  if (n_columns < 1 || n_columns > kScoreMaxColumns) return fail(FMH_ERR_INVALID, "%zu value columns: 1 to %u are taken", n_columns, kScoreMaxColumns);
  if (row_count > kScoreMaxRows) return fail(FMH_ERR_INVALID, "row_count %zu exceeds 2^21: a sum would leave the integers of an f64 (split the rows)", row_count);
  for (const int32_t* values : {h_dosage_values, h_called_values_or_null})
    for (size_t i = 0; values && i < row_count * n_columns; ++i)
      if (values[i] > kScoreMaxValue || values[i] < -kScoreMaxValue)
        return fail(FMH_ERR_INVALID, "value %d (row entry %zu, column %zu) is beyond +-2^30", values[i], i / n_columns, i % n_columns);
  FMH_TRY(check_samples(h_samples_or_null, n_samples, m->samples));
  FMH_TRY(check_rows(row_begin, row_count, m->variants));
  if (m->ploidy != 2) return fail(FMH_ERR_UNSUPPORTED, "the polygenic score takes diploid genotypes (ploidy 2), got ploidy %zu", m->ploidy);
  FMH_TRY(check_packed(m, "the polygenic score reads"));

  const size_t n = n_samples, K = n_columns;
  const uint32_t last = h_samples_or_null ? h_samples_or_null[n - 1] : (uint32_t)(n - 1);
  const uint32_t nvec = last / 64 + 1;  // 64 samples per 16 bytes of a row; within the row: sample `last` exists
  const uint32_t groups = (nvec + 3) / 4, vgroups = (uint32_t)((K + 15) / 16);
  const size_t item_rows = score_item_rows(options().score_item_rows.load(std::memory_order_relaxed));
  const size_t n_blocks = (row_count + item_rows - 1) / item_rows, steps = (row_count + kScoreStepRows - 1) / kScoreStepRows;
  FMH_TRY(check_item_count(n_blocks * groups, "FMH_SCORE_ITEM_ROWS"));

  // a matrix that is biallelic with nothing missing calls every genotype: C is the column totals of U, no second contraction
  const bool complete = !m->pc && !m->p1 && !m->p2;
  const bool contract_called = d_called_sum_or_null && !complete;
  const long long budget = options().score_budget_bytes.load(std::memory_order_relaxed);
  const size_t need = score_call_bytes(row_count, (size_t)last + 1, K, item_rows, contract_called);
  if (row_count && (budget < 0 || need > (size_t)budget))
    return fail(FMH_ERR_UNSUPPORTED, "the score of %zu rows x %u covered samples x %zu columns needs %zu bytes of digits and slabs, above FMH_SCORE_BUDGET_BYTES = %lld (split the rows)",
                row_count, last + 1, K, need, budget);

  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;
  if (row_count == 0) {  // empty sums
    FMH_TRY(call.start());
    HIP_TRY(hipMemsetAsync(d_dosage_sum, 0, n * K * sizeof(long long), st));
    if (d_called_sum_or_null) HIP_TRY(hipMemsetAsync(d_called_sum_or_null, 0, n * K * sizeof(long long), st));
    return call.finish();
  }
  std::vector<long long> totals;
  if (d_called_sum_or_null && complete) {
    totals.assign(K, 0);
    for (size_t r = 0; r < row_count; ++r)
      for (size_t k = 0; k < K; ++k) totals[k] += h_called_values_or_null[r * K + k];
  }

  const size_t digit_threads = steps * vgroups * 64, digit_vectors = digit_threads * 4;
  const size_t block_pitch = (size_t)groups * kScoreGroupSamples * K;  // i64 of one row block's slab
  int32_t *d_v = nullptr, *d_u = nullptr;
  uint32_t* d_samples = nullptr;
  long long *d_totals = nullptr, *slab_s = nullptr, *slab_c = nullptr;
  uint4 *digits_v = nullptr, *digits_u = nullptr;
  FMH_TRY(call.upload(h_dosage_values, row_count * K, &d_v));
  FMH_TRY(call.scratch.get(&digits_v, digit_vectors));
  FMH_TRY(call.scratch.get(&slab_s, n_blocks * block_pitch));
  if (contract_called) {
    FMH_TRY(call.upload(h_called_values_or_null, row_count * K, &d_u));
    FMH_TRY(call.scratch.get(&digits_u, digit_vectors));
    FMH_TRY(call.scratch.get(&slab_c, n_blocks * block_pitch));
  }
  if (h_samples_or_null) FMH_TRY(call.upload(h_samples_or_null, n, &d_samples));
  if (!totals.empty()) FMH_TRY(call.upload(totals.data(), K, &d_totals));

  ScoreArgs a{};
  set_plane_rows(a, m);
  a.nvec = nvec;
  a.groups = groups;
  a.columns = (uint32_t)K;
  a.vgroups = vgroups;
  a.digits_v = digits_v;
  a.digits_u = digits_u;
  a.row_begin = row_begin;
  a.row_count = row_count;
  a.item_rows = (uint32_t)item_rows;
  a.n_blocks = (uint32_t)n_blocks;
  a.n_items = (uint32_t)(n_blocks * groups);
  a.slab_s = slab_s;
  a.slab_c = slab_c;

  FMH_TRY(call.start());
  const dim3 digit_grid((unsigned)((digit_threads + 255) / 256)), reduce_grid((unsigned)((n * K + 255) / 256));
  hipLaunchKernelGGL(score_digits_kernel, digit_grid, dim3(256), 0, st, d_v, row_count, (uint32_t)K, vgroups, digit_threads, digits_v);
  HIP_TRY(hipGetLastError());
  if (contract_called) {
    hipLaunchKernelGGL(score_digits_kernel, digit_grid, dim3(256), 0, st, d_u, row_count, (uint32_t)K, vgroups, digit_threads, digits_u);
    HIP_TRY(hipGetLastError());
  }
  {
    void (*kernel)(const ScoreArgs) = contract_called ? score_sums_kernel<true> : score_sums_kernel<false>;
    const size_t lds = ((contract_called ? 2 : 1) * (kScoreFieldVecs + kScoreStepVecs) + (contract_called ? 0 : 2)) * sizeof(uint4);
    size_t grid = 0;
    FMH_TRY(persistent_grid(reinterpret_cast<const void*>(kernel), kScoreThreads, 0, a.n_items, call.ws->cus, &grid, lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kScoreThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(score_reduce_kernel, reduce_grid, dim3(256), 0, st, slab_s, d_samples, n * K, (uint32_t)K, (uint32_t)n_blocks, block_pitch, d_dosage_sum);
  HIP_TRY(hipGetLastError());
  if (contract_called) {
    hipLaunchKernelGGL(score_reduce_kernel, reduce_grid, dim3(256), 0, st, slab_c, d_samples, n * K, (uint32_t)K, (uint32_t)n_blocks, block_pitch,
                       d_called_sum_or_null);
    HIP_TRY(hipGetLastError());
  } else if (d_totals) {
    hipLaunchKernelGGL(assoc_fill_kernel, reduce_grid, dim3(256), 0, st, d_totals, (uint32_t)K, n * K, d_called_sum_or_null);
    HIP_TRY(hipGetLastError());
  }
  return call.finish();
}

// ---- host only (no device).  The operation order is the header's; the unit is built with -ffp-contract=off ----------------------------------
extern "C" int fmh_score_exponents(const double* h_weights, size_t n_rows, size_t n_columns, int32_t* h_exponent) {
  if (!h_exponent) return fail(FMH_ERR_INVALID, "NULL argument");
  if (n_columns < 1 || n_columns > kScoreMaxColumns) return fail(FMH_ERR_INVALID, "%zu value columns: 1 to %u are taken", n_columns, kScoreMaxColumns);
  if (n_rows != 0 && !h_weights) return fail(FMH_ERR_INVALID, "NULL weights");
  const size_t K = n_columns;
  std::vector<double> mx(K, 0.0);
  for (size_t r = 0; r < n_rows; ++r)
    for (size_t k = 0; k < K; ++k) {
      const double w = h_weights[r * K + k];
      if (!std::isfinite(w)) return fail(FMH_ERR_INVALID, "weight %zu of row entry %zu is not finite", k, r);
      mx[k] = std::max(mx[k], std::fabs(w));
    }
  for (size_t k = 0; k < K; ++k) h_exponent[k] = score_exponent(mx[k]);
  return FMH_OK;
}

extern "C" int fmh_score_values(const double* h_weights, size_t n_rows, size_t n_columns, const int32_t* h_exponent, const uint32_t* h_hom_ref_or_null,
                                const uint32_t* h_het_or_null, const uint32_t* h_hom_alt_or_null, int32_t* h_dosage_values,
                                int32_t* h_called_values_or_null, long long* h_called_total_or_null, uint8_t* h_row_used) {
  if (n_columns < 1 || n_columns > kScoreMaxColumns) return fail(FMH_ERR_INVALID, "%zu value columns: 1 to %u are taken", n_columns, kScoreMaxColumns);
  if (!h_exponent) return fail(FMH_ERR_INVALID, "NULL exponents");
  const int given = (h_hom_ref_or_null != nullptr) + (h_het_or_null != nullptr) + (h_hom_alt_or_null != nullptr);
  if (given != 0 && given != 3) return fail(FMH_ERR_INVALID, "the three site tracks go together: %d of them given", given);
  const bool tracks = given == 3;
  if (!h_called_values_or_null != !h_called_total_or_null) return fail(FMH_ERR_INVALID, "the called values and their totals go together");
  if (h_called_values_or_null && !tracks) return fail(FMH_ERR_INVALID, "the called values need the site tracks (the row's mean dosage)");
  const size_t K = n_columns;
  if (h_called_total_or_null) std::fill(h_called_total_or_null, h_called_total_or_null + K, 0ll);
  if (n_rows == 0) return FMH_OK;
  if (!h_weights || !h_dosage_values || !h_row_used) return fail(FMH_ERR_INVALID, "NULL argument");
  for (size_t r = 0; r < n_rows; ++r) {
    const double* w = h_weights + r * K;
    bool any = false;
    for (size_t k = 0; k < K; ++k) {
      if (!std::isfinite(w[k])) return fail(FMH_ERR_INVALID, "weight %zu of row entry %zu is not finite", k, r);
      if (std::fabs(std::ldexp(w[k], h_exponent[k])) > 0x1p29)
        return fail(FMH_ERR_INVALID, "weight %zu of row entry %zu is beyond the column's exponent %d: 2 |w| 2^e <= 2^30 is required", k, r, h_exponent[k]);
      any = any || w[k] != 0.0;
    }
    uint64_t N = 1, n_alt = 0;
    if (tracks) {
      N = (uint64_t)h_hom_ref_or_null[r] + h_het_or_null[r] + h_hom_alt_or_null[r];
      n_alt = (uint64_t)h_het_or_null[r] + 2 * (uint64_t)h_hom_alt_or_null[r];
    }
    const bool used = any && N != 0;
    h_row_used[r] = used ? 1 : 0;
    const double mu = used && tracks ? (double)n_alt / (double)N : 0.0;
    for (size_t k = 0; k < K; ++k) {
      h_dosage_values[r * K + k] = used ? (int32_t)std::rint(std::ldexp(w[k], h_exponent[k])) : 0;
      if (h_called_values_or_null) {
        const double product = mu * w[k];
        const int32_t u = used ? (int32_t)std::rint(std::ldexp(product, h_exponent[k])) : 0;
        h_called_values_or_null[r * K + k] = u;
        h_called_total_or_null[k] += u;
      }
    }
  }
  return FMH_OK;
}

extern "C" int fmh_score_stats(const long long* h_dosage_sum, const long long* h_called_sum_or_null, const long long* h_called_total_or_null,
                               const int32_t* h_exponent, size_t n_samples, size_t n_columns, int mode, double* h_score) {
  if (n_columns < 1 || n_columns > kScoreMaxColumns) return fail(FMH_ERR_INVALID, "%zu value columns: 1 to %u are taken", n_columns, kScoreMaxColumns);
  if (mode != kScoreModeMean && mode != kScoreModeCenter && mode != kScoreModeZero)
    return fail(FMH_ERR_INVALID, "mode %d: FMH_SCORE_MEAN, FMH_SCORE_CENTER or FMH_SCORE_ZERO", mode);
  if (n_samples == 0) return FMH_OK;
  if (!h_dosage_sum || !h_exponent || !h_score) return fail(FMH_ERR_INVALID, "NULL argument");
  if (mode != kScoreModeZero && !h_called_sum_or_null) return fail(FMH_ERR_INVALID, "modes mean and center need the called sums");
  if (mode == kScoreModeMean && !h_called_total_or_null) return fail(FMH_ERR_INVALID, "mode mean needs the totals of the called values");
  const size_t K = n_columns;
  for (size_t i = 0; i < n_samples; ++i)
    for (size_t k = 0; k < K; ++k) {
      const size_t o = i * K + k;
      long long x = h_dosage_sum[o];
      if (mode == kScoreModeMean) x += h_called_total_or_null[k] - h_called_sum_or_null[o];
      if (mode == kScoreModeCenter) x -= h_called_sum_or_null[o];
      h_score[o] = std::ldexp((double)x, -h_exponent[k]);
    }
  return FMH_OK;
}
