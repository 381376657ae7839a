// ldscore.hip — LD scores: fmh_ld_scores (participants, partner ranges and the item table on the host; the MFMA tile kernel that adds every
// pair term into its rows' fixed-point sums) and the host-only fmh_ld_scores_host, fmh_ld_score_values and fmh_ldsc_regress.  Kernel in
// ldscore_kernels.hpp, host arithmetic in ldscore_host.hpp; definition in include/ferromic_hip.h, scheme in DESIGN.md section 3.26.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "abi_internal.hpp"
#include "geno_ld_call.hpp"
#include "ldscore_host.hpp"
#include "ldscore_kernels.hpp"
#include "stat_call.hpp"

using namespace fmh;
using namespace fmhi;
using namespace fmh_host;

namespace {

constexpr size_t kRowBytes = 28;  // of a launch's scratch per kept row: row, position, sum, hom-alt count, Q, counted
constexpr size_t kItemBytes = sizeof(uint2);

template <bool MISSING, bool ADJUST> int launch_items(const LdScoreArgs& a, size_t n_items, int cus, hipStream_t st) {
  size_t grid = 0;
  FMH_TRY(persistent_grid(reinterpret_cast<const void*>(ldscore_kernel<MISSING, ADJUST>), kLdScoreThreads, 0, n_items, cus, &grid, ldscore_lds_bytes(MISSING)));
  hipLaunchKernelGGL((ldscore_kernel<MISSING, ADJUST>), dim3((unsigned)grid), dim3(kLdScoreThreads), 0, st, a);
  HIP_TRY(hipGetLastError());
  return FMH_OK;
}

}  // namespace

extern "C" int fmh_ld_scores(const fmh_matrix* m, const uint32_t* h_samples_or_null, size_t n_samples, size_t row_begin, size_t row_count,
                             const uint8_t* h_keep_or_null, const uint32_t* h_positions_or_null, const fmh_ldscore_params* params, int64_t* h_q,
                             uint32_t* h_partners_or_null, uint32_t* h_counted, void* stream) {
  // ---- every refusal, before any launch ----
  if (!m) return fail(FMH_ERR_INVALID, "NULL matrix");
  if (!params) return fail(FMH_ERR_INVALID, "NULL params");
  if (!h_q) return fail(FMH_ERR_INVALID, "NULL h_q");
  if (!h_counted) return fail(FMH_ERR_INVALID, "NULL h_counted");
  if (n_samples == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  FMH_TRY(check_samples(h_samples_or_null, n_samples, m->samples));
  FMH_TRY(check_rows(row_begin, row_count, m->variants));
  const fmh_ldscore_params& P = *params;
  if (const char* refused = ld_score_check_params(P)) return fail(FMH_ERR_INVALID, "%s (flags %u)", refused, P.flags);
  const uint32_t* x = h_positions_or_null ? h_positions_or_null + row_begin : nullptr;
  for (size_t k = 1; x && k < row_count; ++k)
    if (x[k] < x[k - 1]) return fail(FMH_ERR_INVALID, "the positions descend at row entry %zu of the range", k);
  FMH_TRY(check_genotype_matrix(m, "the LD scores take"));
  if (row_count >= 0xFFFFFFFFull) return fail(FMH_ERR_UNSUPPORTED, "a range of %zu rows: fewer than 2^32 - 1 are taken (split the rows)", row_count);

  // ---- participants and their partner ranges ----
  std::vector<uint32_t> rows, px, lo, hi;
  for (size_t r = 0; r < row_count; ++r) {
    if (h_keep_or_null && !h_keep_or_null[r]) continue;
    rows.push_back((uint32_t)r);
    px.push_back(x ? x[r] : (uint32_t)r);
  }
  const size_t K = rows.size();
  ld_score_ranges(px, P.window, lo, hi);
  if (const size_t k = ld_score_crowded_row(lo, hi); k != K)
    return fail(FMH_ERR_UNSUPPORTED, "row entry %u of the range has %u partners in its window: at most 2^22 are taken (narrow the window)", rows[k], hi[k] - lo[k]);

  // ---- items: tile pairs (I, J >= I) with a partner pair; hi ascends, so tile I reaches the tile of its last row's last partner ----
  const size_t n_tiles = (K + kLdScoreTile - 1) / kLdScoreTile;
  size_t n_items = 0;
  for (size_t I = 0; I < n_tiles; ++I) n_items += (hi[std::min(K, (I + 1) * kLdScoreTile) - 1] - 1) / kLdScoreTile - I + 1;
  if (n_items > ((size_t)1 << 31)) return fail(FMH_ERR_UNSUPPORTED, "more than 2^31 work items (%zu tile pairs): split the rows", n_items);
  const long long budget = options().ldscore_budget_bytes.load(std::memory_order_relaxed);
  if (K && (budget < 0 || (size_t)budget < K * kRowBytes + kItemBytes))
    return fail(FMH_ERR_UNSUPPORTED, "the sums of %zu kept rows and one work item need %zu bytes of scratch, above FMH_LDSCORE_BUDGET_BYTES = %lld", K,
                K * kRowBytes + kItemBytes, budget);

  for (size_t r = 0; r < row_count; ++r) {
    h_q[r] = 0;
    h_counted[r] = 0;
    if (h_partners_or_null) h_partners_or_null[r] = 0;
  }
  if (K == 0) return FMH_OK;  // no kept row: no launch

  std::vector<uint2> items;
  items.reserve(n_items);
  for (size_t I = 0; I < n_tiles; ++I)
    for (size_t J = I; J <= (hi[std::min(K, (I + 1) * kLdScoreTile) - 1] - 1) / kLdScoreTile; ++J) items.push_back(make_uint2((uint32_t)I, (uint32_t)J));
  const size_t chunk_items = std::min(n_items, ((size_t)budget - K * kRowBytes) / kItemBytes);

  const bool missing = m->pc || m->p1 || m->p2;
  const ColumnMask mask = column_mask(m, h_samples_or_null, n_samples);
  StatCall call;
  FMH_TRY(call.begin(m->device, stream));
  hipStream_t st = call.st;
  LdScoreArgs a{};
  set_plane_rows(a, m);
  uint32_t *d_rows = nullptr, *d_x = nullptr, *d_mask = nullptr, *d_sum = nullptr, *d_hom = nullptr, *d_counted = nullptr;
  unsigned long long* d_q = nullptr;
  uint2* d_items = nullptr;
  FMH_TRY(call.upload(rows.data(), K, &d_rows));
  FMH_TRY(call.upload(px.data(), K, &d_x));
  FMH_TRY(call.upload(mask.words.data(), mask.words.size(), &d_mask));
  FMH_TRY(call.scratch.get(&d_sum, K));
  FMH_TRY(call.scratch.get(&d_hom, K));
  FMH_TRY(call.zeroed(K, &d_q));
  FMH_TRY(call.zeroed(K, &d_counted));
  FMH_TRY(call.scratch.get(&d_items, chunk_items));
  a.row_begin = row_begin;
  a.rows = d_rows; a.x = d_x; a.mask = d_mask; a.vec0 = mask.vec0; a.vec1 = mask.vec1;
  a.K = (uint32_t)K; a.n = (uint32_t)n_samples; a.window = P.window;
  a.items = d_items; a.row_sum = d_sum; a.row_hom = d_hom; a.q = d_q; a.counted = d_counted;

  for (size_t i0 = 0; i0 < n_items; i0 += chunk_items) {
    const size_t count = std::min(chunk_items, n_items - i0);
    FMH_TRY(call.start());
    if (i0 == 0 && !missing) {
      ClumpArgs sums{};
      set_plane_rows(sums, m);
      sums.row_begin = row_begin; sums.rows = d_rows; sums.mask = d_mask; sums.vec0 = mask.vec0; sums.vec1 = mask.vec1; sums.K = (uint32_t)K;
      hipLaunchKernelGGL(clump_row_sums_kernel, dim3((unsigned)wave_grid(K, call.ws->cus)), dim3(kClumpThreads), 0, st, sums, d_sum, d_hom);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(d_items, items.data() + i0, count * sizeof(uint2), hipMemcpyHostToDevice, st));
    a.n_items = (uint32_t)count;
    const bool adjust = P.flags & FMH_LDSCORE_ADJUST;
    FMH_TRY(missing ? (adjust ? launch_items<true, true>(a, count, call.ws->cus, st) : launch_items<true, false>(a, count, call.ws->cus, st))
                    : (adjust ? launch_items<false, true>(a, count, call.ws->cus, st) : launch_items<false, false>(a, count, call.ws->cus, st)));
    FMH_TRY(call.finish());  // the item table of the next chunk overwrites this one's
  }
  std::vector<unsigned long long> q(K);
  std::vector<uint32_t> counted(K);
  HIP_TRY(hipMemcpyAsync(q.data(), d_q, K * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(counted.data(), d_counted, K * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (size_t k = 0; k < K; ++k) {
    h_q[rows[k]] = (int64_t)q[k];
    h_counted[rows[k]] = counted[k];
    if (h_partners_or_null) h_partners_or_null[rows[k]] = hi[k] - lo[k];
  }
  return FMH_OK;
}

// ---- host only (no device) -------------------------------------------------------------------------------------------------------------------
extern "C" int fmh_ld_scores_host(const uint8_t* h_dosage, const uint32_t* h_x_or_null, size_t K, size_t n, const fmh_ldscore_params* params,
                                  int64_t* h_q, uint32_t* h_partners_or_null, uint32_t* h_counted) {
  if (!params) return fail(FMH_ERR_INVALID, "NULL params");
  if (K != 0 && !h_q) return fail(FMH_ERR_INVALID, "NULL h_q");
  if (K != 0 && !h_counted) return fail(FMH_ERR_INVALID, "NULL h_counted");
  if (n == 0) return fail(FMH_ERR_INVALID, "n_samples is 0");
  if (K != 0 && !h_dosage) return fail(FMH_ERR_INVALID, "NULL dosage");
  for (size_t i = 0; i < K * n; ++i)
    if (h_dosage[i] > 3) return fail(FMH_ERR_INVALID, "dosage %u (row %zu, sample %zu) is not 0, 1, 2 or 3", h_dosage[i], i / n, i % n);
  if (const char* refused = ld_score_check_params(*params)) return fail(FMH_ERR_INVALID, "%s (flags %u)", refused, params->flags);
  for (size_t k = 1; h_x_or_null && k < K; ++k)
    if (h_x_or_null[k] < h_x_or_null[k - 1]) return fail(FMH_ERR_INVALID, "the positions descend at row %zu", k);
  if (K >= 0xFFFFFFFFull) return fail(FMH_ERR_UNSUPPORTED, "%zu rows: fewer than 2^32 - 1 are taken", K);
  ld_scores_host(h_dosage, h_x_or_null, K, n, *params, h_q, h_partners_or_null, h_counted);
  return FMH_OK;
}

extern "C" int fmh_ld_score_values(const int64_t* h_q, const uint32_t* h_counted, size_t K, double* h_score) {
  if (K != 0 && (!h_q || !h_counted || !h_score)) return fail(FMH_ERR_INVALID, "a NULL sum, count or output with %zu rows", K);
  ld_score_values(h_q, h_counted, K, h_score);
  return FMH_OK;
}

extern "C" int fmh_ldsc_regress(const double* h_chi2, const double* h_score, const double* h_w_score_or_null, size_t K, double N, double M, uint64_t blocks,
                                const double* fixed_intercept_or_null, fmh_ldsc_out* out) {
  if (!out) return fail(FMH_ERR_INVALID, "NULL out");
  if (K != 0 && (!h_chi2 || !h_score)) return fail(FMH_ERR_INVALID, "NULL chi2 or score with %zu sites", K);
  if (const char* refused = ldsc_regress(h_chi2, h_score, h_w_score_or_null, K, N, M, blocks, fixed_intercept_or_null, out))
    return fail(FMH_ERR_INVALID, "%s (%zu sites, N %g, M %g, %llu blocks)", refused, K, N, M, (unsigned long long)blocks);
  return FMH_OK;
}
