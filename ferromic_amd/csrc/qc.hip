// qc.hip — genotype QC: fmh_genotype_counts (per site and per sample the numbers of hom-ref, het and hom-alt genotypes, exact integers from
// one pass over the bit planes, and the exact per-sample weighted called sum), fmh_hwe_exact / fmh_hwe_exact_host (the Hardy-Weinberg exact
// test on the device and its host twin, one shared function) and the host-only estimators fmh_genotype_site_stats,
// fmh_genotype_site_weights and fmh_genotype_sample_stats.  Kernels in qc_kernels.hpp; definition in include/ferromic_hip.h, scheme in
// DESIGN.md section 3.17.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "abi_internal.hpp"
#include "qc_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;

namespace {

constexpr size_t kQcDefaultItemRows = 4096;
constexpr uint64_t kQcMaxStatGenotypes = (uint64_t)1 << 31;  // the estimators' integer products stay below 2^63

}  // namespace

extern "C" int fmh_genotype_counts(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                                   const uint8_t* h_keep_or_null, const uint32_t* h_row_weight_or_null, const fmh_genotype_site_out* site_or_null,
                                   const fmh_genotype_sample_out* sample_or_null, uint64_t* h_kept_rows, void* stream) {
  // ---- every refusal, before any launch ----
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  if (m->ploidy != 2) return fail(FMH_ERR_UNSUPPORTED, "genotype QC takes diploid genotypes (ploidy 2), got ploidy %zu", m->ploidy);
  FMH_TRY(check_samples(h_samples_or_null, n_samples, m->samples));
  FMH_TRY(check_rows(row_begin, row_count, m->variants));
  const fmh_genotype_site_out site = site_or_null ? *site_or_null : fmh_genotype_site_out{nullptr, nullptr, nullptr};
  const fmh_genotype_sample_out sample = sample_or_null ? *sample_or_null : fmh_genotype_sample_out{nullptr, nullptr, nullptr, nullptr};
  const bool want_tracks = site.d_hom_ref || site.d_het || site.d_hom_alt;
  const bool want_tables = sample.d_hom_ref || sample.d_het || sample.d_hom_alt;
  if (!want_tracks && !want_tables && !sample.d_weighted_called) return fail(FMH_ERR_INVALID, "every output is NULL");
  if (h_row_weight_or_null && !sample.d_weighted_called) return fail(FMH_ERR_INVALID, "row weights are given but d_weighted_called is NULL");
  if (!h_row_weight_or_null && sample.d_weighted_called) return fail(FMH_ERR_INVALID, "d_weighted_called is given but the row weights are NULL");
  FMH_TRY(check_packed(m, "genotype QC reads"));

  const size_t n = n_samples;
  size_t kept = row_count;
  unsigned long long weight_total = 0;
  if (h_keep_or_null) kept = (size_t)std::count_if(h_keep_or_null, h_keep_or_null + row_count, [](uint8_t k) { return k != 0; });
  if (h_row_weight_or_null)
    for (size_t i = 0; i < row_count; ++i)
      if (!h_keep_or_null || h_keep_or_null[i]) weight_total += h_row_weight_or_null[i];
  if (h_kept_rows) *h_kept_rows = kept;
  const bool tables = want_tables && kept != 0, weighted = h_row_weight_or_null && kept != 0;
  if (row_count == 0 || !(want_tracks || tables || weighted)) return FMH_OK;

  // the sample list as a bit mask over the row's 32-bit words, and the listed samples before each word
  const uint32_t last = h_samples_or_null ? h_samples_or_null[n - 1] : (uint32_t)(n - 1);
  const uint32_t words = last / 16 + 1;  // within the row: sample `last` exists
  uint32_t word_lanes = kQcMinWordLanes;
  while (word_lanes < words && word_lanes < kQcThreads) word_lanes *= 2;
  const uint32_t n_chunks = (words + word_lanes - 1) / word_lanes;
  std::vector<uint32_t> selected((size_t)n_chunks * word_lanes, 0), rank_before(selected.size(), 0);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t s = h_samples_or_null ? h_samples_or_null[i] : (uint32_t)i;
    selected[s / 16] |= 1u << (2 * (s % 16));
  }
  for (size_t w = 1; w < selected.size(); ++w) rank_before[w] = rank_before[w - 1] + (uint32_t)__builtin_popcount(selected[w - 1]);

  const size_t item_rows = item_rows_of(options().qc_item_rows, kQcDefaultItemRows);
  const size_t row_blocks = (row_count + item_rows - 1) / item_rows;
  FMH_TRY(check_item_count(row_blocks * n_chunks, "FMH_QC_ITEM_ROWS"));

  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;
  uint32_t *d_selected = nullptr, *d_rank = nullptr, *d_weight = nullptr;
  uint8_t* d_keep = nullptr;
  FMH_TRY(call.upload(selected.data(), selected.size(), &d_selected));
  FMH_TRY(call.upload(rank_before.data(), rank_before.size(), &d_rank));
  if (h_keep_or_null && (tables || weighted)) FMH_TRY(call.upload(h_keep_or_null, row_count, &d_keep));
  if (weighted) FMH_TRY(call.upload(h_row_weight_or_null, row_count, &d_weight));

  QcArgs a{};
  set_plane_rows(a, m);
  a.words = words;
  a.word_lanes = word_lanes;
  a.n_chunks = n_chunks;
  a.selected = d_selected;
  a.rank_before = d_rank;
  a.row_begin = row_begin;
  a.row_count = row_count;
  a.item_rows = (uint32_t)item_rows;
  a.n_items = (uint32_t)(row_blocks * n_chunks);
  a.keep = d_keep;
  a.weight = d_weight;
  a.weight_total = weight_total;
  a.site_hom_ref = site.d_hom_ref; a.site_het = site.d_het; a.site_hom_alt = site.d_hom_alt;
  a.hom_ref = sample.d_hom_ref; a.het = sample.d_het; a.hom_alt = sample.d_hom_alt;
  a.weighted_called = sample.d_weighted_called;

  FMH_TRY(call.start());
  if (want_tracks || tables) {
    // a row cut into column chunks has one writer per chunk: the tracks are zeroed and added to; otherwise they are stored
    if (want_tracks && n_chunks > 1)
      for (uint32_t* track : {site.d_hom_ref, site.d_het, site.d_hom_alt})
        if (track) HIP_TRY(hipMemsetAsync(track, 0, row_count * sizeof(uint32_t), st));
    void (*kernel)(const QcArgs) = want_tracks ? (tables ? qc_count_kernel<true, true> : qc_count_kernel<true, false>) : qc_count_kernel<false, true>;
    const size_t lds_bytes = (size_t)qc_count_lds_dwords(word_lanes, tables) * sizeof(uint32_t);
    size_t grid = 0;
    FMH_TRY(persistent_grid(reinterpret_cast<const void*>(kernel), kQcThreads, lds_bytes, a.n_items, call.ws->cus, &grid));
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kQcThreads), lds_bytes, st, a);
    HIP_TRY(hipGetLastError());
  }
  if (weighted) {
    const size_t lds_bytes = (size_t)16 * word_lanes * sizeof(unsigned long long);
    size_t grid = 0;
    FMH_TRY(persistent_grid(reinterpret_cast<const void*>(qc_weighted_kernel), kQcThreads, lds_bytes, a.n_items, call.ws->cus, &grid));
    hipLaunchKernelGGL(qc_weighted_kernel, dim3((unsigned)grid), dim3(kQcThreads), lds_bytes, st, a);
    HIP_TRY(hipGetLastError());
  }
  return call.finish();
}

extern "C" int fmh_hwe_exact(const uint32_t* d_hom_ref, const uint32_t* d_het, const uint32_t* d_hom_alt, size_t n_sites, double* d_p, int device,
                             void* stream) {
  if (n_sites == 0) return FMH_OK;
  if (!d_hom_ref || !d_het || !d_hom_alt || !d_p) return fail(FMH_ERR_INVALID, "NULL argument");
  if ((n_sites + 255) / 256 > 0x7FFFFFFFu) return fail(FMH_ERR_UNSUPPORTED, "more than 2^39 sites in one call");
  StatCall call;
  FMH_TRY(call.begin(device, stream));
  FMH_TRY(call.start());
  hipLaunchKernelGGL(hwe_kernel, dim3((unsigned)((n_sites + 255) / 256)), dim3(256), 0, call.st, d_hom_ref, d_het, d_hom_alt, n_sites, d_p);
  HIP_TRY(hipGetLastError());
  return call.finish();
}

// ---- host only (no device).  The operation order is the header's; the unit is built with -ffp-contract=off ----------------------------------
extern "C" int fmh_hwe_exact_host(const uint32_t* h_hom_ref, const uint32_t* h_het, const uint32_t* h_hom_alt, size_t n_sites, double* h_p) {
  if (n_sites == 0) return FMH_OK;
  if (!h_hom_ref || !h_het || !h_hom_alt || !h_p) return fail(FMH_ERR_INVALID, "NULL argument");
  for (size_t i = 0; i < n_sites; ++i)
    if ((uint64_t)h_hom_ref[i] + h_het[i] + h_hom_alt[i] > kHweMaxGenotypes)
      return fail(FMH_ERR_UNSUPPORTED, "site %zu has more than 2^26 called genotypes", i);
  for (size_t i = 0; i < n_sites; ++i) h_p[i] = hwe_exact_p(h_hom_ref[i], h_het[i], h_hom_alt[i]);
  return FMH_OK;
}

namespace {

// N of every site below 2^31, so that het (2N - 1), n_alt n_ref and N (2N - 1) fit a u64
int check_site_counts(const uint32_t* h_hom_ref, const uint32_t* h_het, const uint32_t* h_hom_alt, size_t n_sites) {
  if (!h_hom_ref || !h_het || !h_hom_alt) return fail(FMH_ERR_INVALID, "NULL argument");
  for (size_t i = 0; i < n_sites; ++i)
    if ((uint64_t)h_hom_ref[i] + h_het[i] + h_hom_alt[i] >= kQcMaxStatGenotypes)
      return fail(FMH_ERR_UNSUPPORTED, "site %zu has 2^31 or more called genotypes", i);
  return FMH_OK;
}

}  // namespace

extern "C" int fmh_genotype_site_stats(const uint32_t* h_hom_ref, const uint32_t* h_het, const uint32_t* h_hom_alt, size_t n_sites, uint64_t n_samples,
                                       const fmh_genotype_site_stats_out* out) {
  if (n_sites == 0) return FMH_OK;
  if (!out) return fail(FMH_ERR_INVALID, "out is NULL");
  FMH_TRY(check_site_counts(h_hom_ref, h_het, h_hom_alt, n_sites));
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t i = 0; i < n_sites; ++i) {
    const uint64_t het = h_het[i], N = (uint64_t)h_hom_ref[i] + het + h_hom_alt[i];
    const uint64_t n_alt = 2 * (uint64_t)h_hom_alt[i] + het, n_ref = 2 * N - n_alt;
    const double p = N == 0 ? nan : (double)n_alt / (double)(2 * N);
    if (out->h_call_rate) out->h_call_rate[i] = n_samples == 0 ? nan : (double)N / (double)n_samples;
    if (out->h_alt_frequency) out->h_alt_frequency[i] = p;
    if (out->h_maf) out->h_maf[i] = N == 0 ? nan : std::min(p, 1.0 - p);
    if (out->h_f_is) out->h_f_is[i] = n_alt * n_ref == 0 ? nan : 1.0 - (double)(het * (2 * N - 1)) / (double)(n_alt * n_ref);
    if (out->h_expected_het) out->h_expected_het[i] = N == 0 ? nan : (double)(n_alt * n_ref) / (double)(2 * N - 1);
  }
  return FMH_OK;
}

extern "C" int fmh_genotype_site_weights(const uint32_t* h_hom_ref, const uint32_t* h_het, const uint32_t* h_hom_alt, size_t n_sites, uint32_t* h_weight) {
  if (n_sites == 0) return FMH_OK;
  if (!h_weight) return fail(FMH_ERR_INVALID, "NULL argument");
  FMH_TRY(check_site_counts(h_hom_ref, h_het, h_hom_alt, n_sites));
  for (size_t i = 0; i < n_sites; ++i) {
    const uint64_t het = h_het[i], N = (uint64_t)h_hom_ref[i] + het + h_hom_alt[i];
    const uint64_t n_alt = 2 * (uint64_t)h_hom_alt[i] + het, n_ref = 2 * N - n_alt;
    // e = n_alt n_ref / (N (2N - 1)) <= N / (2N - 1) <= 1: the weight is at most 2^31
    const double e = N == 0 ? 0.0 : (double)(n_alt * n_ref) / (double)(N * (2 * N - 1));
    h_weight[i] = (uint32_t)std::rint(e * 2147483648.0);
  }
  return FMH_OK;
}

extern "C" int fmh_genotype_sample_stats(const uint64_t* h_hom_ref, const uint64_t* h_het, const uint64_t* h_hom_alt,
                                         const uint64_t* h_weighted_called_or_null, size_t n, uint64_t kept_rows,
                                         const fmh_genotype_sample_stats_out* out) {
  if (n == 0) return FMH_OK;
  if (!h_hom_ref || !h_het || !h_hom_alt || !out) return fail(FMH_ERR_INVALID, "NULL argument");
  if (out->h_f && !h_weighted_called_or_null) return fail(FMH_ERR_INVALID, "h_f needs the weighted called sums");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t i = 0; i < n; ++i) {
    const uint64_t called = h_hom_ref[i] + h_het[i] + h_hom_alt[i];
    if (out->h_call_rate) out->h_call_rate[i] = kept_rows == 0 ? nan : (double)called / (double)kept_rows;
    if (out->h_het_rate) out->h_het_rate[i] = called == 0 ? nan : (double)h_het[i] / (double)called;
    if (out->h_f) out->h_f[i] = h_weighted_called_or_null[i] == 0 ? nan : 1.0 - (double)h_het[i] / ((double)h_weighted_called_or_null[i] / 2147483648.0);
  }
  return FMH_OK;
}
