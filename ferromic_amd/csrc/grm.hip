// grm.hip — the genomic relationship matrix and its eigenpairs: fmh_grm (the per-row counts through fmh_genotype_counts, the values on the
// host, the 2-bit codes of the usable rows and the f64 matrix-core Gram of the values they choose, added into the caller's matrix; the
// pair counts through fmh_kinship_counts), the host-only fmh_grm_values / fmh_grm_finish / fmh_grm_host and fmh_grm_eigen over the solver of
// fmh_pca_eigen_scores.  Kernels in grm_kernels.hpp, host arithmetic in grm_host.hpp; definition in include/ferromic_hip.h, scheme in
// DESIGN.md section 3.24.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "abi_internal.hpp"
#include "grm_host.hpp"
#include "grm_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;

namespace {

// stage times of the calling thread's last timed fmh_grm: codes, Gram, slab reduce + accumulate (ms)
thread_local double g_grm_stage_ms[3] = {0.0, 0.0, 0.0};

}  // namespace

extern "C" int fmh_timing_read_grm(double* h_stage_ms) {
  if (!h_stage_ms) return fail(FMH_ERR_INVALID, "h_stage_ms is NULL");
  for (int i = 0; i < 3; ++i) h_stage_ms[i] = g_grm_stage_ms[i];
  return FMH_OK;
}

extern "C" int fmh_grm(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                       const uint8_t* h_keep_or_null, const fmh_grm_params* params, const fmh_grm_out* out, uint64_t* h_kept_rows, void* stream) {
  // ---- every refusal, before any launch ----
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!params) return fail(FMH_ERR_INVALID, "NULL params");
  if (!out) return fail(FMH_ERR_INVALID, "out is NULL");
  if (!out->d_products) return fail(FMH_ERR_INVALID, "d_products of out is NULL");
  const fmh_grm_params P = *params;
  if (const char* refused = fmh_host::grm_check_params(P)) return fail(FMH_ERR_INVALID, "%s", refused);
  if (P.denominator == FMH_GRM_PAIRS && !out->d_pair_sites) return fail(FMH_ERR_INVALID, "denominator FMH_GRM_PAIRS needs d_pair_sites");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  if (m->ploidy != 2) return fail(FMH_ERR_UNSUPPORTED, "the relationship matrix takes diploid genotypes (ploidy 2), got ploidy %zu", m->ploidy);
  FMH_TRY(check_samples(h_samples_or_null, n_samples, m->samples));
  FMH_TRY(check_rows(row_begin, row_count, m->variants));
  FMH_TRY(check_packed(m, "the relationship matrix reads"));
  if (row_count >= 0xFFFFFFFFull) return fail(FMH_ERR_UNSUPPORTED, "a range of %zu rows: fewer than 2^32 - 1 are taken (split the rows)", row_count);
  const size_t n = n_samples;
  if (n > ((size_t)1 << 24)) return fail(FMH_ERR_UNSUPPORTED, "a relationship matrix of %zu samples: more than 2^24 samples are not supported", n);

  // the kept rows, relative to row_begin
  std::vector<uint32_t> kept_rows;
  kept_rows.reserve(row_count);
  for (size_t i = 0; i < row_count; ++i)
    if (!h_keep_or_null || h_keep_or_null[i]) kept_rows.push_back((uint32_t)i);
  const size_t kept = kept_rows.size();

  // the budget, with every kept row taken as usable (how many are is known only after the counting kernel)
  Workspace* w = nullptr;
  FMH_TRY(use_device(m->device));
  FMH_TRY(workspace(m->device, &w));
  const size_t n_pad = round_up(n, kPcaTile), nt = n_pad / kPcaTile, tiles = nt * (nt + 1) / 2;
  const size_t tile_bytes = (size_t)kPcaTile * kPcaTile * sizeof(double);
  const long long forced = options().grm_splits.load();
  // K splits as fmh_pca_gram's: enough (tile, split) workgroups for two per CU, a split keeps at least 8 stages (2 048 rows)
  auto plan_splits = [&](size_t kwords) {
    const size_t stages = kwords / kPcaStageWords;
    size_t splits = 1;
    if (forced > 0) splits = std::min<size_t>((size_t)forced, stages);
    else if (tiles < 2 * (size_t)w->cus) splits = std::min<size_t>((2 * (size_t)w->cus + tiles - 1) / tiles, std::max<size_t>(stages / 8, 1));
    return std::min<size_t>(std::max<size_t>(splits, 1), 65535);  // gridDim.y
  };
  auto total_bytes = [&](size_t rows, size_t splits) {
    const size_t kwords = round_up((rows + 63) / 64, kPcaStageWords);
    return n * n * sizeof(double) + 2 * kwords * n_pad * 8 + kwords * 64 * sizeof(GrmSiteValues) + rows * 5 + 3 * row_count * sizeof(uint32_t) +
           (splits > 1 ? splits * tiles * tile_bytes : 0) + (out->d_pair_sites ? 4 * n * n * 8 : 0);
  };
  const size_t budget = (size_t)options().pca_budget_bytes.load();
  if (kept != 0) {
    const size_t kwords = round_up((kept + 63) / 64, kPcaStageWords);
    size_t splits = plan_splits(kwords);
    if (total_bytes(kept, splits) > budget) splits = 1;
    if (total_bytes(kept, splits) > budget)
      return fail(FMH_ERR_UNSUPPORTED, "a relationship matrix of %zu samples x %zu rows needs %zu bytes of device memory, budget %zu (FMH_PCA_BUDGET_BYTES)", n,
                  kept, total_bytes(kept, splits), budget);
  }

  if (h_kept_rows) *h_kept_rows = kept;
  if (out->h_usable_rows) *out->h_usable_rows = 0;
  if (out->h_scale) *out->h_scale = 0.0;
  if (kept == 0) return FMH_OK;

  // ---- c, a of the kept rows: genotype QC's site tracks over the range ----
  std::vector<uint32_t> called(kept), allele_count(kept);
  {
    DeviceScratch scratch(m->device, (hipStream_t)stream);
    uint32_t* d_tracks = nullptr;
    FMH_TRY(scratch.get(&d_tracks, 3 * row_count));
    const fmh_genotype_site_out site{d_tracks, d_tracks + row_count, d_tracks + 2 * row_count};
    FMH_TRY(fmh_genotype_counts(m, h_samples_or_null, n, row_begin, row_count, nullptr, nullptr, &site, nullptr, nullptr, stream));
    scratch.settled = true;  // fmh_genotype_counts has synchronised the stream
    std::vector<uint32_t> tracks(3 * row_count);
    HIP_TRY(hipMemcpy(tracks.data(), d_tracks, tracks.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < kept; ++k) {
      const size_t r = kept_rows[k];
      called[k] = tracks[r] + tracks[row_count + r] + tracks[2 * row_count + r];
      allele_count[k] = tracks[row_count + r] + 2 * tracks[2 * row_count + r];
    }
  }
  std::vector<uint8_t> usable(kept);
  std::vector<double> z(3 * kept);
  double scale = 0.0;
  uint64_t n_usable = 0;
  fmh_host::grm_values(called.data(), allele_count.data(), kept, P.method, usable.data(), nullptr, z.data(), &scale, &n_usable);
  if (out->h_called) std::copy(called.begin(), called.end(), out->h_called);
  if (out->h_allele_count) std::copy(allele_count.begin(), allele_count.end(), out->h_allele_count);
  if (out->h_usable) std::copy(usable.begin(), usable.end(), out->h_usable);
  if (out->h_usable_rows) *out->h_usable_rows = n_usable;
  if (out->h_scale) *out->h_scale = scale;
  if (n_usable == 0) return FMH_OK;

  // ---- the usable rows: their list, their values (zero on the padding rows), the samples' list positions ----
  const size_t K = (size_t)n_usable, words = (K + 63) / 64, kwords = round_up(words, kPcaStageWords);
  std::vector<uint32_t> rows(K);
  std::vector<GrmSiteValues> vals(kwords * 64, GrmSiteValues{0.0, 0.0, 0.0, 0.0});
  for (size_t k = 0, u = 0; k < kept; ++k) {
    if (!usable[k]) continue;
    rows[u] = kept_rows[k];
    vals[u] = GrmSiteValues{z[3 * k], z[3 * k + 1], z[3 * k + 2], 0.0};
    ++u;
  }
  const uint32_t last = h_samples_or_null ? h_samples_or_null[n - 1] : (uint32_t)(n - 1);
  const uint32_t nvec = last / 64 + 1, groups = (nvec + 3) / 4;  // 16-byte vectors through the last selected sample: within the row
  std::vector<uint32_t> rank((size_t)groups * kSegGroupSamples, kSegNone);
  for (size_t i = 0; i < n; ++i) rank[h_samples_or_null ? h_samples_or_null[i] : i] = (uint32_t)i;

  size_t splits = plan_splits(kwords);
  if (total_bytes(K, splits) > budget) splits = 1;
  const size_t words_per_split = round_up((kwords + splits - 1) / splits, kPcaStageWords);
  splits = (kwords + words_per_split - 1) / words_per_split;

  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;
  uint32_t *d_rows = nullptr, *d_rank = nullptr;
  GrmSiteValues* d_vals = nullptr;
  uint8_t* d_flags = nullptr;
  unsigned long long* d_code = nullptr;
  double *d_call = nullptr, *d_slabs = nullptr;
  FMH_TRY(call.upload(rows.data(), K, &d_rows));
  FMH_TRY(call.upload(rank.data(), rank.size(), &d_rank));
  FMH_TRY(call.upload(vals.data(), vals.size(), &d_vals));
  const bool has_flags = m->pc || m->p1 || m->p2;
  if (has_flags) FMH_TRY(call.scratch.get(&d_flags, K));
  FMH_TRY(call.scratch.get(&d_code, 2 * kwords * n_pad));
  FMH_TRY(call.scratch.get(&d_call, n * n));
  if (splits > 1) FMH_TRY(call.scratch.get(&d_slabs, splits * tiles * (size_t)kPcaTile * kPcaTile));

  GrmCodeArgs a{};
  set_plane_rows(a, m);
  a.nvec = nvec;
  a.groups = groups;
  a.row_begin = row_begin;
  a.rows = d_rows;
  a.flags = d_flags;
  a.rank = d_rank;
  a.K = (uint32_t)K;
  a.words = (uint32_t)words;
  a.n_items = (uint64_t)words * groups;
  a.spad = n_pad;
  a.plane_words = kwords * n_pad;
  a.code = d_code;

  KernelTimer<4> stages;
  FMH_TRY(call.start());
  FMH_TRY(stages.start(st));
  HIP_TRY(hipMemsetAsync(d_code, 0, 2 * kwords * n_pad * sizeof(unsigned long long), st));  // the padding samples' and padding words' codes
  if (has_flags) {
    PlaneRows planes{};
    set_plane_rows(planes, m);
    hipLaunchKernelGGL(plane_flags_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, planes, row_begin, d_rows, (uint32_t)K, d_flags);
    HIP_TRY(hipGetLastError());
  }
  {
    size_t grid = 0;
    FMH_TRY(persistent_grid(reinterpret_cast<const void*>(grm_codes_kernel), kGrmCodeThreads, 0, (size_t)std::min<uint64_t>(a.n_items, (uint64_t)1 << 31),
                            call.ws->cus, &grid, 2 * 64 * 4 * sizeof(uint4)));
    hipLaunchKernelGGL(grm_codes_kernel, dim3((unsigned)grid), dim3(kGrmCodeThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  FMH_TRY(stages.mark(1, st));
  hipLaunchKernelGGL(grm_gram_kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(d_code), d_vals,
                     (uint32_t)n_pad, (uint32_t)kwords, (uint32_t)nt, (uint32_t)words_per_split, (uint32_t)n, d_call, d_slabs);
  HIP_TRY(hipGetLastError());
  FMH_TRY(stages.mark(2, st));
  if (splits > 1) {
    const size_t threads = tiles * (size_t)kPcaTile * kPcaTile;
    hipLaunchKernelGGL(pca_slab_reduce_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, d_slabs, (uint32_t)tiles, (uint32_t)splits,
                       (uint32_t)nt, (uint32_t)n, 1.0, d_call);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(grm_accumulate_kernel, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, st, d_call, n * n, out->d_products);
  HIP_TRY(hipGetLastError());
  FMH_TRY(stages.stop(st));
  FMH_TRY(call.finish());
  for (int i = 0; i < 3; ++i) FMH_TRY(stages.elapsed(i, &g_grm_stage_ms[i]));

  // ---- N: kinship's `both` over the usable rows ----
  if (out->d_pair_sites) {
    std::vector<uint8_t> keep(row_count, 0);
    for (size_t u = 0; u < K; ++u) keep[rows[u]] = 1;
    DeviceScratch scratch(m->device, st);
    unsigned long long* d_tables = nullptr;
    FMH_TRY(scratch.get(&d_tables, 3 * n * n));
    HIP_TRY(hipMemsetAsync(d_tables, 0, 3 * n * n * sizeof(unsigned long long), st));
    const fmh_kinship_out tables{out->d_pair_sites, d_tables, d_tables + n * n, d_tables + 2 * n * n};
    FMH_TRY(fmh_kinship_counts(m, h_samples_or_null, n, row_begin, row_count, keep.data(), &tables, nullptr, stream));
    scratch.settled = true;  // fmh_kinship_counts has synchronised the stream
  }
  return FMH_OK;
}

// ---- host only (no device).  The operation order is the header's; the unit is built with -ffp-contract=off ------------------------------
extern "C" int fmh_grm_values(const uint32_t* h_called, const uint32_t* h_allele_count, size_t rows, uint32_t method, uint8_t* h_usable, double* h_p,
                              double* h_z, double* h_scale, uint64_t* h_n_usable) {
  if (method != FMH_GRM_STANDARDIZED && method != FMH_GRM_CENTERED) return fail(FMH_ERR_INVALID, "method is neither FMH_GRM_STANDARDIZED nor FMH_GRM_CENTERED");
  if (rows != 0 && (!h_called || !h_allele_count)) return fail(FMH_ERR_INVALID, "NULL argument");
  fmh_host::grm_values(h_called, h_allele_count, rows, method, h_usable, h_p, h_z, h_scale, h_n_usable);
  return FMH_OK;
}

extern "C" int fmh_grm_finish(const double* h_products, const uint64_t* h_pair_sites_or_null, size_t n, const fmh_grm_params* params, uint64_t n_usable,
                              double scale, double* h_matrix) {
  if (!params) return fail(FMH_ERR_INVALID, "NULL params");
  if (const char* refused = fmh_host::grm_check_params(*params)) return fail(FMH_ERR_INVALID, "%s", refused);
  if (n == 0) return FMH_OK;
  if (!h_products || !h_matrix) return fail(FMH_ERR_INVALID, "NULL argument");
  if (params->denominator == FMH_GRM_PAIRS && !h_pair_sites_or_null) return fail(FMH_ERR_INVALID, "denominator FMH_GRM_PAIRS needs the pair counts");
  fmh_host::grm_finish(h_products, h_pair_sites_or_null, n, *params, n_usable, scale, h_matrix);
  return FMH_OK;
}

extern "C" int fmh_grm_host(const uint8_t* h_dosage, size_t K, size_t n, uint32_t method, double* h_products, uint64_t* h_pair_sites_or_null,
                            uint64_t* h_n_usable, double* h_scale) {
  if (method != FMH_GRM_STANDARDIZED && method != FMH_GRM_CENTERED) return fail(FMH_ERR_INVALID, "method is neither FMH_GRM_STANDARDIZED nor FMH_GRM_CENTERED");
  if (n == 0) return fail(FMH_ERR_INVALID, "n is 0");
  if (!h_products || (K != 0 && !h_dosage)) return fail(FMH_ERR_INVALID, "NULL argument");
  fmh_host::grm_host(h_dosage, K, n, method, h_products, h_pair_sites_or_null, h_n_usable, h_scale);
  return FMH_OK;
}

extern "C" int fmh_grm_eigen(int device, double* d_matrix, size_t n, size_t n_components, double* h_eigenvalues, double* h_eigenvectors) {
  if (!d_matrix || !h_eigenvalues || !h_eigenvectors) return fail(FMH_ERR_INVALID, "NULL argument");
  if (n == 0) return fail(FMH_ERR_INVALID, "n is 0");
  if (n_components == 0 || n_components > n) return fail(FMH_ERR_INVALID, "n_components %zu outside 1..%zu", n_components, n);
  if (n > 46340) return fail(FMH_ERR_UNSUPPORTED, "the eigen solver takes at most 46 340 samples (n * n must fit a 32-bit index), got %zu", n);
  std::vector<double> top, lambda;
  FMH_TRY(pca_eigen_top(device, d_matrix, n, n_components, lambda, top));
  for (size_t k = 0; k < n_components; ++k) {
    h_eigenvalues[k] = lambda[k];
    fmh_host::grm_fix_sign(&top[k * n], n, 1);
    for (size_t i = 0; i < n; ++i) h_eigenvectors[i * n_components + k] = top[k * n + i];
  }
  return FMH_OK;
}
