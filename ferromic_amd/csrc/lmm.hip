// lmm.hip — mixed-model association scan: fmh_lmm_projections (per site the projections of the mean-imputed dosage on a basis - the
// eigenvectors of the relationship matrix - contracted with weight and coefficient rows, on the f64 matrix cores straight from the bit
// planes), its host twin fmh_lmm_projections_host, fmh_lmm_null (host: the variance ratio delta per phenotype by restricted likelihood in the
// eigenbasis) and fmh_lmm_stats (host: beta, se, t and p per site and phenotype from the projections).  Kernels in lmm_kernels.hpp, host
// arithmetic in lmm_host.hpp; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.25.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "abi_internal.hpp"
#include "lmm_host.hpp"
#include "lmm_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;

namespace {

constexpr size_t kLmmDefaultItemRows = 4096;

}  // namespace

extern "C" int fmh_lmm_projections(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                                   const double* d_basis, size_t n_components, const double* d_weights, size_t n_weights, const double* d_linear,
                                   size_t n_linear, double* d_quad, double* d_lin, uint32_t* h_called_or_null, uint32_t* h_allele_count_or_null,
                                   void* stream) {
  // ---- every refusal, before any launch ----
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!d_basis || !d_weights || !d_linear) return fail(FMH_ERR_INVALID, "NULL basis, weights or linear");
  if (!d_quad || !d_lin) return fail(FMH_ERR_INVALID, "d_quad or d_lin is NULL");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  FMH_TRY(check_samples(h_samples_or_null, n_samples, m->samples));
  FMH_TRY(check_rows(row_begin, row_count, m->variants));
  if (n_components < 1 || n_components > fmh_host::kLmmMaxComponents)
    return fail(FMH_ERR_INVALID, "%zu components: 1 to %zu are taken", n_components, fmh_host::kLmmMaxComponents);
  if (n_weights < 1 || n_weights > fmh_host::kLmmMaxQuad) return fail(FMH_ERR_INVALID, "%zu weight rows: 1 to %zu are taken", n_weights, fmh_host::kLmmMaxQuad);
  if (n_linear < 1 || n_linear > fmh_host::kLmmMaxLinear) return fail(FMH_ERR_INVALID, "%zu linear rows: 1 to %zu are taken", n_linear, fmh_host::kLmmMaxLinear);
  if (m->ploidy != 2) return fail(FMH_ERR_UNSUPPORTED, "the mixed-model scan takes diploid genotypes (ploidy 2), got ploidy %zu", m->ploidy);
  FMH_TRY(check_packed(m, "the mixed-model scan reads"));

  const size_t n = n_samples, K = n_components, P = n_weights, L = n_linear;
  const uint32_t last = h_samples_or_null ? h_samples_or_null[n - 1] : (uint32_t)(n - 1);
  const uint32_t covered = last + 1;
  const uint32_t groups = last / kLmmGroupSamples + 1;  // 64 samples per 16 bytes of a row; within the row: sample `last` exists
  const size_t cgroups = (K + kLmmGroupComps - 1) / kLmmGroupComps;
  const uint32_t lin_tiles = (uint32_t)((L + 15) / 16);
  const size_t image_doubles = cgroups * groups * kLmmStageDoubles;
  const size_t coef_doubles = cgroups * 16 * (lin_tiles + 1) * kLmmCoefTileDoubles;
  const size_t bytes = (image_doubles + coef_doubles + row_count) * sizeof(double) + 3 * row_count * sizeof(uint32_t) + (size_t)covered * sizeof(int32_t);
  const size_t budget = (size_t)options().pca_budget_bytes.load();
  if (bytes > budget)
    return fail(FMH_ERR_UNSUPPORTED, "projections on %zu components of %zu samples x %zu rows need %zu bytes of device memory, budget %zu (FMH_PCA_BUDGET_BYTES)", K,
                n, row_count, bytes, budget);
  if (cgroups * groups > 0xFFFFFFFFull) return fail(FMH_ERR_UNSUPPORTED, "a basis image of %zu stages: fewer than 2^32 are taken", cgroups * groups);
  if (row_count == 0) return FMH_OK;

  // ---- c, a of the rows: genotype QC's site tracks over the range; mu on the host ----
  std::vector<double> mu(row_count);
  {
    DeviceScratch scratch(m->device, (hipStream_t)stream);
    uint32_t* d_tracks = nullptr;
    FMH_TRY(use_device(m->device));
    FMH_TRY(scratch.get(&d_tracks, 3 * row_count));
    const fmh_genotype_site_out site{d_tracks, d_tracks + row_count, d_tracks + 2 * row_count};
    FMH_TRY(fmh_genotype_counts(m, h_samples_or_null, n, row_begin, row_count, nullptr, nullptr, &site, nullptr, nullptr, stream));
    scratch.settled = true;  // fmh_genotype_counts has synchronised the stream
    std::vector<uint32_t> tracks(3 * row_count);
    HIP_TRY(hipMemcpy(tracks.data(), d_tracks, tracks.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < row_count; ++r) {
      const uint32_t c = tracks[r] + tracks[row_count + r] + tracks[2 * row_count + r];
      const uint32_t a = tracks[row_count + r] + 2 * tracks[2 * row_count + r];
      mu[r] = fmh_host::lmm_mu(c, a);
      if (h_called_or_null) h_called_or_null[r] = c;
      if (h_allele_count_or_null) h_allele_count_or_null[r] = a;
    }
  }
  std::vector<int32_t> rank;
  if (h_samples_or_null) {
    rank.assign(covered, -1);
    for (size_t i = 0; i < n; ++i) rank[h_samples_or_null[i]] = (int32_t)i;
  }

  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;

  // rows per item: the option, else 4 096 or - where that would leave compute units without an item - fewer, in whole passes
  size_t item_rows = item_rows_of(options().lmm_item_rows, kLmmDefaultItemRows);
  if (options().lmm_item_rows.load(std::memory_order_relaxed) <= 0) {
    const size_t wanted = 2 * (size_t)std::max(call.ws->cus, 1);
    const size_t spread = round_up((row_count + wanted - 1) / wanted, kLmmPassRows);
    item_rows = std::min(item_rows, std::max<size_t>(spread, kLmmPassRows));
  }
  const size_t n_items = (row_count + item_rows - 1) / item_rows;
  FMH_TRY(check_item_count(n_items, "FMH_LMM_ITEM_ROWS"));

  int32_t* d_rank = nullptr;
  double *d_image = nullptr, *d_coef = nullptr, *d_mu = nullptr;
  if (!rank.empty()) FMH_TRY(call.upload(rank.data(), rank.size(), &d_rank));
  FMH_TRY(call.upload(mu.data(), row_count, &d_mu));
  FMH_TRY(call.scratch.get(&d_image, image_doubles));
  FMH_TRY(call.scratch.get(&d_coef, coef_doubles));

  LmmArgs a{};
  set_plane_rows(a, m);
  a.groups = groups;
  a.cgroups = (uint32_t)cgroups;
  a.lin_tiles = lin_tiles;
  a.P = (uint32_t)P;
  a.L = (uint32_t)L;
  a.basis_image = d_image;
  a.coef_image = d_coef;
  a.mu = d_mu;
  a.row_begin = row_begin;
  a.row_count = row_count;
  a.item_rows = (uint32_t)item_rows;
  a.n_items = (uint32_t)n_items;
  a.quad = d_quad;
  a.lin = d_lin;

  FMH_TRY(call.start());
  hipLaunchKernelGGL(lmm_basis_image_kernel, dim3((unsigned)((image_doubles + 255) / 256)), dim3(256), 0, st, d_basis, d_rank, (uint32_t)n, covered, (uint32_t)K,
                     groups, image_doubles, d_image);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(lmm_coef_image_kernel, dim3((unsigned)((coef_doubles + 255) / 256)), dim3(256), 0, st, d_linear, d_weights, (uint32_t)L, (uint32_t)P,
                     (uint32_t)K, lin_tiles, coef_doubles, d_coef);
  HIP_TRY(hipGetLastError());
  {
    void (*kernel)(const LmmArgs) = lin_tiles == 1 ? lmm_project_kernel<1> : lin_tiles == 2 ? lmm_project_kernel<2> : lin_tiles == 3 ? lmm_project_kernel<3>
                                                                                                                                       : lmm_project_kernel<4>;
    size_t grid = 0;
    FMH_TRY(persistent_grid(reinterpret_cast<const void*>(kernel), kLmmThreads, 0, n_items, call.ws->cus, &grid, 2 * kLmmStageDoubles * sizeof(double)));
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kLmmThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  return call.finish();
}

// ---- host only (no device).  The operation order is the header's; the unit is built with -ffp-contract=off ----------------------------------
extern "C" int fmh_lmm_projections_host(const uint8_t* h_dosage, size_t rows, size_t n, const double* h_basis, size_t n_components, const double* h_weights,
                                        size_t n_weights, const double* h_linear, size_t n_linear, double* h_quad, double* h_lin,
                                        uint32_t* h_called_or_null, uint32_t* h_allele_count_or_null) {
  if (!h_basis || !h_weights || !h_linear || !h_quad || !h_lin || (rows != 0 && !h_dosage)) return fail(FMH_ERR_INVALID, "NULL argument");
  if (n == 0) return fail(FMH_ERR_INVALID, "n is 0");
  if (n_components < 1 || n_components > fmh_host::kLmmMaxComponents || n_weights < 1 || n_weights > fmh_host::kLmmMaxQuad || n_linear < 1 ||
      n_linear > fmh_host::kLmmMaxLinear)
    return fail(FMH_ERR_INVALID, "%zu components, %zu weight rows, %zu linear rows: 1 to %zu, 1 to %zu and 1 to %zu are taken", n_components, n_weights,
                n_linear, fmh_host::kLmmMaxComponents, fmh_host::kLmmMaxQuad, fmh_host::kLmmMaxLinear);
  fmh_host::lmm_projections_host(h_dosage, rows, n, h_basis, n_components, h_weights, n_weights, h_linear, n_linear, h_quad, h_lin, h_called_or_null,
                                 h_allele_count_or_null);
  return FMH_OK;
}

extern "C" int fmh_lmm_null(const double* h_eigenvalues, const double* h_eigenvectors, const double* h_phenotypes, const double* h_covariates_or_null,
                            size_t n, size_t n_phenotypes, size_t n_covariates, const double* h_fixed_delta_or_null, size_t* h_q, uint8_t* h_dropped_or_null,
                            const fmh_lmm_null_out* out) {
  if (!h_eigenvalues || !h_eigenvectors || !h_phenotypes || !h_q || !out) return fail(FMH_ERR_INVALID, "NULL argument");
  if (!out->h_delta || !out->h_sigma_g2 || !out->h_sigma_e2 || !out->h_heritability || !out->h_log_likelihood || !out->h_at_boundary || !out->h_reason ||
      !out->h_weights || !out->h_linear || !out->h_m || !out->h_v || !out->h_r)
    return fail(FMH_ERR_INVALID, "a NULL array in out");
  if (n_covariates != 0 && !h_covariates_or_null) return fail(FMH_ERR_INVALID, "%zu covariates but the pointer is NULL", n_covariates);
  if (n_phenotypes < 1) return fail(FMH_ERR_INVALID, "at least one phenotype is required");
  if (n == 0 || n > fmh_host::kLmmMaxComponents) return fail(FMH_ERR_INVALID, "n = %zu: 1 to %zu samples are taken", n, fmh_host::kLmmMaxComponents);
  const size_t P = n_phenotypes, cin = n_covariates;
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(h_eigenvalues[i])) return fail(FMH_ERR_INVALID, "eigenvalue %zu is not finite", i);
  for (size_t i = 0; i < n * n; ++i)
    if (!std::isfinite(h_eigenvectors[i])) return fail(FMH_ERR_INVALID, "eigenvector %zu, sample entry %zu is not finite", i % n, i / n);
  for (size_t i = 0; i < n * P; ++i)
    if (!std::isfinite(h_phenotypes[i])) return fail(FMH_ERR_INVALID, "phenotype %zu of sample entry %zu is not finite", i % P, i / P);
  for (size_t i = 0; i < n * cin; ++i)
    if (!std::isfinite(h_covariates_or_null[i])) return fail(FMH_ERR_INVALID, "covariate %zu of sample entry %zu is not finite", i % cin, i / cin);
  if (h_fixed_delta_or_null)
    for (size_t p = 0; p < P; ++p)
      if (!std::isfinite(h_fixed_delta_or_null[p]) || !(h_fixed_delta_or_null[p] > 0.0)) return fail(FMH_ERR_INVALID, "delta of phenotype %zu is not a positive number", p);
  const fmh_host::LmmNullOut o{out->h_delta, out->h_sigma_g2, out->h_sigma_e2, out->h_heritability, out->h_log_likelihood, out->h_at_boundary, out->h_reason,
                               out->h_weights, out->h_linear, out->h_m, out->h_v, out->h_r, out->h_grid_log_likelihood_or_null};
  if (const char* refused = fmh_host::lmm_null(h_eigenvalues, h_eigenvectors, h_phenotypes, h_covariates_or_null, n, P, cin, h_q, h_dropped_or_null, h_fixed_delta_or_null, o))
    return fail(FMH_ERR_INVALID, "n = %zu, %zu phenotypes, %zu design columns: %s", n, P, *h_q, refused);
  return FMH_OK;
}

extern "C" int fmh_lmm_stats(const double* h_quad, const double* h_lin, const uint32_t* h_called, const uint32_t* h_allele_count, size_t n_rows,
                             const double* h_m, const double* h_v, const double* h_r, uint64_t n_samples, size_t q, size_t n_phenotypes, double* h_beta,
                             double* h_se, double* h_t, double* h_p) {
  if (n_phenotypes < 1 || n_phenotypes > fmh_host::kLmmMaxQuad) return fail(FMH_ERR_INVALID, "%zu phenotypes: 1 to %zu are taken", n_phenotypes, fmh_host::kLmmMaxQuad);
  if (q < 1 || n_phenotypes * (q + 1) > fmh_host::kLmmMaxLinear)
    return fail(FMH_ERR_INVALID, "%zu phenotypes with %zu design columns: q >= 1 and P (q + 1) <= %zu are required", n_phenotypes, q, fmh_host::kLmmMaxLinear);
  if (n_samples < q + 2) return fail(FMH_ERR_INVALID, "n = %llu with %zu design columns: n - q - 1 >= 1 is required", (unsigned long long)n_samples, q);
  if (n_rows == 0) return FMH_OK;
  if (!h_quad || !h_lin || !h_called || !h_allele_count || !h_m || !h_v || !h_r) return fail(FMH_ERR_INVALID, "NULL argument");
  fmh_host::lmm_stats(h_quad, h_lin, h_called, h_allele_count, n_rows, h_m, h_v, h_r, n_samples, q, n_phenotypes, h_beta, h_se, h_t, h_p);
  return FMH_OK;
}
